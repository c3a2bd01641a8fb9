#!/usr/bin/env python3
"""Generate tests/golden/voxel_hostile.npz and tests/golden/mesh_hostile.npz: the two geometry steps
either side of ICP -- open3d::VoxelDownSample and the point -> mesh distance inside
feh::MeasureSurfaceError -- run through the COMPILED REFERENCE (oracle/_ref: Open3D's DownSample.cpp,
libigl's AABB) on inputs chosen to be hostile to a GPU restatement.

The inputs are NOT stored: every family is a recipe (a Philox seed and a few parameters, built below with
nothing but f64 +, -, *, / so that it comes back bit for bit on every machine); the fixture keeps a CRC of
every input array, and tests/test_voxel_hostile.py / tests/test_mesh_hostile.py regenerate the inputs and
check it.  Stored are the recorded results only:

  voxel_hostile.npz   per family  <name>_p / _n / _c   Open3D's points / normals / colours, rows lexsorted by point
                                  <name>_crc           CRCs of xyz, normals, colours
  mesh_hostile.npz    per family  <name>_d2 / _face / _cl   libigl's squared distance, face and closest point
                                  <name>_ex            the EXACT squared distance (tests/exact_geometry.py, rounded
                                                       once to f64) of the first <name>_ex.size queries
                                  <name>_ties          [share of rows whose libigl face differs from the oracle's,
                                                        share whose closest point differs]: libigl keeps the first
                                                        face it meets on an exact tie, the oracle the lowest index
                                  <name>_crc           CRCs of V, F, P
                      needle_table                     per needle thickness: the error of libigl's DISTANCE against the
                                                       exact one, in units of eps * max|coordinate| (of the mesh
                                                       and the query)
                      large_crc                        CRCs of V, F, P of large_case() (nothing else of it is recorded)
                      mse_<pair>_d2 / _crc             libigl's squared distances of the Philox samples that
                                                       measure_surface_error draws (seed and count in MSE_PAIRS)

Non-finite COORDINATES are out of scope for the voxel step: the reference casts floor(NaN) to int, which is
undefined behaviour, so there is nothing to record.  (NaN NORMALS are defined -- AddPoint skips them -- and are
in every voxel family; non-finite mesh QUERIES are tested on the GPU against the library's own two searches.)

    python tests/golden/gen_hostile.py

Needs oracle/_ref (built where the reference tree is); about five minutes, most of it exact rational arithmetic.
Writes both files byte for byte the same on every run."""
import os
import sys
import zlib
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

EPS = 2.0 ** -52
INT_MAX = 2147483647.0


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def crcs(*arrays):
    return np.array([crc(a) for a in arrays], np.uint32)


def rng_of(seed):
    return np.random.Generator(np.random.Philox(seed))


def lexsorted(p, *others):
    k = np.lexsort((p[:, 2], p[:, 1], p[:, 0]))
    return (p[k],) + tuple(o[k] for o in others)


# ---------------------------------------------------------------------------------------------------------
# voxel families: name -> (xyz, normals, colours, voxel)
# ---------------------------------------------------------------------------------------------------------
def _attrs(rng, n):
    """Normals with NaN rows and rows with a single NaN component (DownSample.cpp:55-58 skips both), colours."""
    nrm = rng.random((n, 3)) * 2.0 - 1.0
    col = rng.random((n, 3))
    nrm[::7] = np.nan
    nrm[3::11, 1] = np.nan
    return nrm, col


def _wide_cloud():
    rng = rng_of(901)
    return np.concatenate([rng.random((3000, 3)) * 1000.0, 500.0 + (rng.random((500, 3)) * 2.0 - 1.0) * 1e-4])


def _limit_cloud(seed, slack):
    """A cloud whose extent + voxel is voxel * INT_MAX * (1 + slack): slack < 0 is just inside the reference's limit
    (DownSample.cpp:191), slack > 0 just over it (an empty cloud on both sides)."""
    rng = rng_of(seed)
    voxel = 1e-6
    span = voxel * INT_MAX * (1.0 + slack) - voxel
    p = rng.random((400, 3)) * span
    p[0] = 0.0
    p[1] = span
    p[2] = [span, 0.0, span]
    p[3:40] = p[40:77] + voxel * 0.25                   # some voxels hold two points
    return p, voxel


VOXEL_FAMILIES = ("faces", "negative", "one_voxel_20k", "identical_3000", "signed_zeros", "flat_axis", "offset_1e6",
                  "n1", "n2", "inside_limit", "over_limit", "wide_2e-4", "wide_1e-6", "n2047", "n2048", "n2049",
                  "n1048577")
# the grids of 4e18 cells or more (ordered by three 32-bit sorts in voxel.hip)
VOXEL_WIDE = ("inside_limit", "wide_2e-4", "wide_1e-6")


def voxel_case(name):
    if name == "faces":
        # voxel 0.25, minimum at 0: voxel faces at -0.125 + 0.25 k.  Points exactly on faces, 1 ulp above and below.
        rng = rng_of(11)
        k = rng.integers(1, 12, (200, 3)).astype(np.float64)
        on = -0.125 + 0.25 * k
        p = np.concatenate([[[0.0, 0.0, 0.0]], on, np.nextafter(on, np.inf), np.nextafter(on, -np.inf),
                            np.where(rng.random((200, 3)) < 0.5, on, np.nextafter(on, -np.inf))])
        voxel = 0.25
    elif name == "negative":
        rng = rng_of(12)
        p = -10.0 - rng.random((1500, 3)) * 40.0
        voxel = 8.0
    elif name == "one_voxel_20k":
        rng = rng_of(13)
        mag = np.array([1.0, 1e-3, 1e-6, 1e-9, 1e-12])[rng.integers(0, 5, (20000, 1))]
        p = rng.random((20000, 3)) * mag
        voxel = 4.0
    elif name == "identical_3000":
        p = np.tile(np.array([[0.1, -7.3, 1e5 / 3.0]]), (3000, 1))
        voxel = 0.01
    elif name == "signed_zeros":
        rng = rng_of(15)
        pool = np.array([0.0, -0.0, 5e-324, -5e-324, 0.25, -0.25, 0.5, 1e-300])
        p = pool[rng.integers(0, len(pool), (800, 3))]
        voxel = 0.5
    elif name == "flat_axis":
        rng = rng_of(16)
        p = rng.random((1200, 3)) * np.array([3.0, 2.0, 0.0]) + np.array([0.0, 0.0, 0.37])
        voxel = 0.3
    elif name == "offset_1e6":
        rng = rng_of(17)
        p = 1e6 + rng.random((2000, 3)) * 3.0
        voxel = 0.7
    elif name == "n1":
        p = np.array([[1.5, -2.5, 1e-3]])
        voxel = 0.05
    elif name == "n2":
        p = np.array([[1.5, -2.5, 1e-3], [1.5, -2.5, 1e-3 + 0.05]])
        voxel = 0.05
    elif name == "inside_limit":
        p, voxel = _limit_cloud(18, -1e-9)
    elif name == "over_limit":
        p, voxel = _limit_cloud(19, 1e-9)
    elif name == "wide_2e-4":
        p, voxel = _wide_cloud(), 2e-4
    elif name == "wide_1e-6":
        p, voxel = _wide_cloud(), 1e-6
    elif name in ("n2047", "n2048", "n2049", "n1048577"):
        # the block edges of the exclusive scan that numbers the voxels (2048 entries per block, 2^20 per level)
        n = int(name[1:])
        p = rng_of(20 + n).random((n, 3)) - 0.5
        voxel = 0.2 if n < 4096 else 0.15
    else:
        raise KeyError(name)
    nrm, col = _attrs(rng_of(zlib.crc32(name.encode())), len(p))
    return np.ascontiguousarray(p), nrm, col, voxel


# ---------------------------------------------------------------------------------------------------------
# mesh families: name -> (V, F, P)
# ---------------------------------------------------------------------------------------------------------
# an exactly orthogonal-in-the-rationals rotation (rows of (1,-2,2; 2,-1,-2; 2,2,1) / 3): no libm in the recipe
ROT = np.array([[1.0, -2.0, 2.0], [2.0, -1.0, -2.0], [2.0, 2.0, 1.0]]) / 3.0


def _unit(rng, n):
    d = rng.random((n, 3)) * 2.0 - 1.0
    d[(np.abs(d) < 1e-3).all(1)] = [1.0, 0.0, 0.0]
    return d / np.sqrt((d * d).sum(1))[:, None]


def queries(rng, V, F, nq):
    """Queries on faces, on edges, on vertices, off the surface by 1e-9 .. 1 times the extent, 1e3 extents away,
    and exact duplicates of all of those -- nq rows, shuffled."""
    used = V[np.unique(F)]
    lo, hi = used.min(0), used.max(0)
    ext = float((hi - lo).max()) or 1.0
    n1 = nq // 5
    f = rng.integers(0, len(F), 4 * n1)
    a, b, c = V[F[f, 0]], V[F[f, 1]], V[F[f, 2]]
    u = rng.random((4 * n1, 2))
    fold = u.sum(1) > 1.0
    u[fold] = 1.0 - u[fold]
    onface = a + u[:, :1] * (b - a) + u[:, 1:] * (c - a)
    parts = [onface[:n1],
             (a + u[:, :1] * (b - a))[n1:n1 + n1 // 2], (b + u[:, 1:] * (c - b))[n1 + n1 // 2:2 * n1],      # edges
             a[2 * n1:2 * n1 + n1 // 3], b[2 * n1 + n1 // 3:2 * n1 + 2 * (n1 // 3)], c[2 * n1 + 2 * (n1 // 3):3 * n1]]
    off = ext * np.array([1e-9, 1e-7, 1e-5, 1e-3, 1e-1, 1.0])[rng.integers(0, 6, (n1, 1))]
    parts.append(onface[3 * n1:] + _unit(rng, n1) * off)
    nfar = max(nq // 20, 1)
    parts.append(0.5 * (lo + hi) + _unit(rng, nfar) * (1e3 * ext))
    P = np.concatenate(parts)
    ndup = nq - len(P)
    assert ndup > 0
    P = np.concatenate([P, P[rng.integers(0, len(P), ndup)]])
    return np.ascontiguousarray(P[rng.permutation(len(P))])


def needle_soup(seed, thickness, offset, nf):
    """nf needles of length ~0.3 and width thickness * length in the unit cube at `offset`.  thickness 0: the third
    vertex is computed ON the segment (the triangle keeps whatever area rounding leaves it)."""
    rng = rng_of(seed)
    a = rng.random((nf, 3)) + offset
    d = _unit(rng, nf) * (0.1 + 0.4 * rng.random((nf, 1)))
    w = _unit(rng, nf)
    w = w - d * ((w * d).sum(1) / (d * d).sum(1))[:, None]
    length = np.sqrt((d * d).sum(1))[:, None]
    w = w / np.sqrt((w * w).sum(1))[:, None] * length
    b = a + d
    c = a + d * rng.random((nf, 1)) + w * thickness
    V = np.concatenate([a, b, c])
    F = np.stack([np.arange(nf), nf + np.arange(nf), 2 * nf + np.arange(nf)], 1).astype(np.int32)
    return V, F


def grid_mesh(seed, n, bump):
    """n x n quads (2 n^2 faces) over the unit square, z = bump * noise."""
    rng = rng_of(seed)
    g = np.arange(n + 1) / float(n)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = (rng.random(x.shape) - 0.5) * bump
    V = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v00 = (i * (n + 1) + j).ravel()
    v01, v10, v11 = v00 + 1, v00 + n + 1, v00 + n + 2
    F = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]).astype(np.int32)
    return V, F


def random_soup(seed, nf, scale=1.0):
    rng = rng_of(seed)
    a = rng.random((nf, 3))
    V = np.concatenate([a, a + (rng.random((nf, 3)) - 0.5) * 0.2, a + (rng.random((nf, 3)) - 0.5) * 0.2]) * scale
    F = np.stack([np.arange(nf), nf + np.arange(nf), 2 * nf + np.arange(nf)], 1).astype(np.int32)
    return V, F


NEEDLE_THICKNESS = (1.0, 1e-3, 1e-4, 1e-6, 1e-8, 1e-12, 0.0)
NEEDLE_FAMILIES = tuple("needle_t%g_o%g" % (t, o) for t in NEEDLE_THICKNESS for o in (0.0, 100.0))
NF_EDGES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
NP_EDGES = (1, 63, 64, 65, 4095, 4096, 4097)
MESH_FAMILIES = NEEDLE_FAMILIES + ("flat_grid", "planar_inplane", "bumpy_grid", "bumpy_rot_1e3", "shared_centroid",
                                   "giants_over_small", "far_vertex", "dup_zero_area", "pm1e6") + \
    tuple("nf%d" % n for n in NF_EDGES) + ("np_edges",)
# queries with an exact yardstick per family (Fractions are slow)
N_EXACT = {"needle": 300, "nf": 16, "np_edges": 64, "other": 64}


def n_exact(name):
    return N_EXACT["needle" if name.startswith("needle") else "nf" if name.startswith("nf") else
                   name if name in N_EXACT else "other"]


def mesh_case(name):
    seed = zlib.crc32(name.encode())
    rng = rng_of(seed)
    nq = 300
    if name.startswith("needle"):
        t, o = name[len("needle_t"):].split("_o")
        V, F = needle_soup(seed + 1, float(t), float(o), 240)
    elif name == "flat_grid":
        V, F = grid_mesh(seed + 1, 24, 0.0)
    elif name == "planar_inplane":
        # an axis-aligned planar mesh queried IN its plane: every leaf box has no thickness, every bound is an equality
        V, F = grid_mesh(seed + 1, 24, 0.0)
        V[:, 2] = 0.625
        P = queries(rng, V, F, nq)
        P[:, 2] = 0.625
        return V, F, P
    elif name == "bumpy_grid":
        V, F = grid_mesh(seed + 1, 24, 0.05)
    elif name == "bumpy_rot_1e3":
        V, F = grid_mesh(seed + 1, 24, 0.05)
        V = V @ ROT.T + np.array([1e3, -1e3, 1e3])
    elif name == "shared_centroid":
        # 200 faces with one centroid: one Morton code, leaves that all overlap
        a = rng.random((200, 3)) - 0.5
        b = rng.random((200, 3)) - 0.5
        g = np.array([0.3, 0.2, 0.1])
        V = np.concatenate([a + g, b + g, g - a - b])
        F = np.stack([np.arange(200), 200 + np.arange(200), 400 + np.arange(200)], 1).astype(np.int32)
    elif name == "giants_over_small":
        V, F = grid_mesh(seed + 1, 24, 0.05)
        big = np.array([[-50.0, -50.0, 0.2], [50.0, -50.0, 0.2], [0.0, 80.0, 0.2],
                        [-50.0, -50.0, -0.3], [0.0, 80.0, -0.3], [50.0, -50.0, -0.3]])
        F = np.concatenate([F, len(V) + np.array([[0, 1, 2], [3, 4, 5]])]).astype(np.int32)
        V = np.concatenate([V, big])
        P = queries(rng, V, F[:-2], nq)                      # near the small faces, under the giants
        return V, F, P
    elif name == "far_vertex":
        # an unreferenced vertex sets the Morton box and the 2^-40 inflation, the faces share one cell
        V, F = grid_mesh(seed + 1, 24, 0.05)
        V = np.concatenate([V, [[1e9, -1e9, 1e9]]])
    elif name == "dup_zero_area":
        V, F = grid_mesh(seed + 1, 16, 0.05)
        k = rng.integers(0, len(V), (60, 2)).astype(np.int32)
        mid = 0.5 * (V[k[:, 0]] + V[k[:, 1]])                # collinear third vertices
        zero = np.concatenate([np.stack([k[:20, 0], k[:20, 0], k[:20, 0]], 1), np.stack([k[20:40, 0], k[20:40, 1], k[20:40, 0]], 1),
                               np.stack([k[40:, 0], k[40:, 1], len(V) + np.arange(20)], 1)])
        V = np.concatenate([V, mid[40:]])
        F = np.concatenate([F[:300], zero, F, F[100:200]]).astype(np.int32)
    elif name == "pm1e6":
        s = np.where(rng.random((300, 3)) < 0.5, -1e6, 1e6)
        V = s + (rng.random((300, 3)) - 0.5) * 10.0
        F = rng.integers(0, 300, (400, 3)).astype(np.int32)
    elif name.startswith("nf"):
        nf = int(name[2:])
        V, F = random_soup(77, 4097)
        F = np.ascontiguousarray(F[:nf])
        nq = 120
    elif name == "np_edges":
        V, F = grid_mesh(seed + 1, 24, 0.05)
        nq = max(NP_EDGES)
    else:
        raise KeyError(name)
    V = np.ascontiguousarray(V, np.float64)
    F = np.ascontiguousarray(F, np.int32)
    return V, F, queries(rng, V, F, nq)


def large_case():
    """The one large case: a soup of 204,800 needles against 100,000 queries (BVH against brute force only)."""
    V, F = needle_soup(5150, 1e-6, 0.0, 204800)
    rng = rng_of(5151)
    f = rng.integers(0, len(F), 100000)
    P = V[F[f, 0]] + (V[F[f, 1]] - V[F[f, 0]]) * rng.random((100000, 1)) + _unit(rng, 100000) * \
        np.array([0.0, 1e-9, 1e-6, 1e-3, 1e-1])[rng.integers(0, 5, (100000, 1))]
    return V, F, np.ascontiguousarray(P)


# ---------------------------------------------------------------------------------------------------------
# the samples measure_surface_error draws: Philox4x32-10 keyed by the seed, counter (i, 0|1) -- mesh.hip
# ---------------------------------------------------------------------------------------------------------
def philox4x32(c0, c1, c2, c3, k0, k1):
    M0, M1, m32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & m32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & m32, np.uint64(k1) & m32
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def philox_uniforms(n, seed):
    """The (r, a, b) of sample i as sample_mesh_kernel draws them."""
    i = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, np.uint64)
    w0 = philox4x32(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), z, z, seed & 0xFFFFFFFF, seed >> 32)
    w1 = philox4x32(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), z + np.uint64(1), z, seed & 0xFFFFFFFF, seed >> 32)

    def u53(hi, lo):
        return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.stack([u53(w0[0], w0[1]), u53(w0[2], w0[3]), u53(w1[0], w1[1])], 1)


# (source family, target family, samples, seed): the samples lie on the source, the distances go to the target
MSE_PAIRS = {"needles": ("needle_t0.0001_o0", "needle_t1e-06_o0", 3000, 7),
             "grids": ("bumpy_grid", "giants_over_small", 5000, 11)}


def mse_samples(oracle, pair):
    src, tgt, n, seed = MSE_PAIRS[pair]
    Vs, Fs, _ = mesh_case(src)
    Vt, Ft, _ = mesh_case(tgt)
    pts = oracle.sample_mesh(Vs, Fs, philox_uniforms(n, seed), quirks=False)
    return Vs, Fs, Vt, Ft, pts, n, seed


# ---------------------------------------------------------------------------------------------------------
def exact_d2(P, V, F):
    import exact_geometry
    return exact_geometry.point_mesh_sqdist(P, V, F)


def coordinate_scale(P, V, F):
    """max |coordinate| over the referenced vertices and the query itself, per query."""
    return np.maximum(np.abs(V[np.unique(F)]).max(), np.abs(P).max(1))


def distance_error_units(d2_f64, d2_exact, scales):
    """|sqrt(d2_f64) - sqrt(d2_exact)| in units of eps * scale (one scale per query), to 40 digits."""
    getcontext().prec = 60
    out = []
    for a, e, scale in zip(d2_f64, d2_exact, scales):
        fa = Fraction(float(a))
        da = (Decimal(fa.numerator) / Decimal(fa.denominator)).sqrt()
        de = (Decimal(e.numerator) / Decimal(e.denominator)).sqrt()
        out.append(float(abs(da - de) / (Decimal(EPS) * Decimal(float(scale)))))
    return np.array(out)


def needle_table(rec):
    """Rows (thickness, queries, queries whose distance is off by more than 64 units, worst error in units, the same as
    a share of the mesh extent), one per NEEDLE_THICKNESS, from the RECORDED arrays of a fixture (`rec[name + "_d2"]`:
    libigl's squared distances, `rec[name + "_ex"]`: the exact ones as stored, rounded once to f64) -- so that the
    table can be recomputed from the fixture exactly."""
    table = {}
    for name in NEEDLE_FAMILIES:
        V, F, P = mesh_case(name)
        ex = rec[name + "_ex"]
        ne = len(ex)
        scale = coordinate_scale(P[:ne], V, F)
        err = distance_error_units(rec[name + "_d2"][:ne], [Fraction(float(e)) for e in ex], scale)
        t = float(name[len("needle_t"):].split("_o")[0])
        row = table.setdefault(t, [t, 0, 0, 0.0, 0.0])
        row[1] += ne
        row[2] += int((err > 64).sum())
        row[3] = max(row[3], float(err.max()))
        row[4] = max(row[4], float((err * EPS * scale).max()) / float(np.ptp(V, axis=0).max()))
    return np.array([table[t] for t in NEEDLE_THICKNESS])


def gen_voxel(ref):
    out = {}
    for name in VOXEL_FAMILIES:
        p, nrm, col, voxel = voxel_case(name)
        rp, rn, rc = ref.voxel_down_sample(p, voxel, nrm, col)
        rp, rn, rc = lexsorted(rp, rn, rc)
        out[name + "_p"], out[name + "_n"], out[name + "_c"] = rp, rn, rc
        out[name + "_voxel"] = np.float64(voxel)
        out[name + "_crc"] = crcs(p, nrm, col)
        print("voxel %-16s n=%8d voxel=%g -> %d voxels" % (name, len(p), voxel, len(rp)))
    return out


def gen_mesh(ref, oracle):
    out = {}
    for name in MESH_FAMILIES:
        V, F, P = mesh_case(name)
        d2, face, cl = ref.point_mesh_sqdist(P, V, F)
        od2, oface, ocl = oracle.point_mesh_sqdist(P, V, F)
        ne = n_exact(name)
        ex, _ = exact_d2(P[:ne], V, F)
        out[name + "_d2"], out[name + "_face"] = d2, face
        out[name + "_cl"] = cl
        out[name + "_ex"] = np.array([float(e) for e in ex])
        out[name + "_ties"] = np.array([np.mean(face != oface), np.mean((cl != ocl).any(1))])
        out[name + "_crc"] = crcs(V, F, P)
        scale = coordinate_scale(P[:ne], V, F)
        err = distance_error_units(d2[:ne], ex, scale)
        print("mesh %-22s nf=%5d np=%5d ties face %.3f closest %.4f | d vs exact: worst %.3g units, %d of %d above 64"
              % (name, len(F), len(P), out[name + "_ties"][0], out[name + "_ties"][1], err.max(), int((err > 64).sum()), ne))
    out["needle_table"] = needle_table(out)
    V, F, P = large_case()
    out["large_crc"] = crcs(V, F, P)
    for pair in MSE_PAIRS:
        Vs, Fs, Vt, Ft, pts, n, seed = mse_samples(oracle, pair)
        out["mse_%s_d2" % pair] = ref.point_mesh_sqdist(pts, Vt, Ft)[0]
        out["mse_%s_crc" % pair] = crcs(pts)
    return out


def save(path, arrays):
    """np.savez_compressed with fixed member times: the same bytes on every run."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def main():
    from oracle.oracle import Oracle, Ref
    ref, oracle = Ref(), Oracle()
    save(os.path.join(HERE, "voxel_hostile.npz"), gen_voxel(ref))
    save(os.path.join(HERE, "mesh_hostile.npz"), gen_mesh(ref, oracle))


if __name__ == "__main__":
    main()
