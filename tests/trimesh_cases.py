"""The inputs of the TriangleMesh tests, built from seeds (the fixture tests/golden/trimesh.npz stores only what the compiled
reference made of them): CASES[name] = (mesh, [program, ...]) with a mesh of tests/trimesh_spec.py and programs of its run().
Each case is the smallest shape at which a kernel of trimesh.hip can still go wrong; tests/golden/gen_trimesh.py asserts, on
the reference, the properties that make it bite."""
import functools

import numpy as np

import trimesh_spec as T

NAN, INF = float("nan"), float("inf")
ULP1 = float(np.nextafter(1.0, 2.0))


def _grid(n, step=0.125, seed=0):
    """an n x n quad grid over a bumpy height field: (n + 1)^2 vertices, 2 n^2 triangles"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    z = np.round(rng.uniform(-1.0, 1.0, i.shape) * 64.0) / 256.0
    v = np.stack([i * step, j * step, z], axis=-1).reshape(-1, 3)
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    quad = np.stack([a, a + n + 1, a + n + 2, a + 1], axis=1)
    t = np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    return v, t.astype(np.int32)


def _attrs(nv, nt, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(nv, 3)), rng.uniform(size=(nv, 3)), rng.normal(size=(nt, 3))


def soup():
    """a 20 x 20 grid as triangle soup (three private vertices per triangle; welding gives back 441), the row y = 0 as -0.0
    in every second triangle, and extras: two bit-identical NaN vertices, +inf twice and -inf, two equal denormals and another,
    a pair that differs in z by one ulp"""
    gv, gt = _grid(20, seed=1)
    v = gv[gt.reshape(-1)].copy()
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    odd = np.repeat(np.arange(len(t)) % 2 == 1, 3)
    v[odd & (v[:, 1] == 0.0), 1] = -0.0
    extra = np.array([[NAN, 1.0, 2.0], [NAN, 1.0, 2.0], [INF, 0.5, 0.5], [INF, 0.5, 0.5], [-INF, 0.5, 0.5],
                      [5e-324, 9.0, 9.0], [5e-324, 9.0, 9.0], [1e-323, 9.0, 9.0], [7.0, 7.0, 1.0], [7.0, 7.0, ULP1]])
    n0 = len(v)
    v = np.concatenate([v, extra])
    t = np.concatenate([t, n0 + np.array([[0, 2, 5], [1, 3, 6], [4, 7, 8], [4, 7, 9], [2, 3, 8]], np.int32)])
    vn, vc, _ = _attrs(len(v), len(t), 11)
    return T.mesh(v, t, vn, vc), [[("rdv",)], [("purge",)], [("cvn", 1)], [("ctn", 1), ("purge",)]]


def keys():
    """the three rotations of a triangle, its flip, (0,1,0), (0,0,1), (1,0,0), and triangles that only coincide or degenerate
    once vertex 6 (a copy of 3) is welded"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 0], [3, 2, 1], [2, 3, 1], [2, 2, 0], [5, 5, 5]], np.float64)
    t = [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [0, 1, 0], [0, 0, 1], [1, 0, 0], [3, 4, 5], [6, 4, 5], [4, 5, 6], [3, 4, 6],
         [5, 4, 3], [0, 1, 0]]
    _, vc, tn = _attrs(len(v), len(t), 12)
    return T.mesh(v, t, None, vc, tn), [[("rdt",)], [("rdv",), ("rdt",)], [("rnmt",)], [("rnmv",)], [("purge",)]]


def fan():
    """1,000 triangles around vertex 0 whose normals' magnitudes spread over 2^+-30: the order of the f64 sum shows"""
    rng = np.random.default_rng(13)
    n = 1000
    scale = np.exp2(rng.integers(-15, 16, n).astype(np.float64))
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    a = np.stack([np.cos(ang), np.sin(ang), rng.uniform(-0.5, 0.5, n)], axis=1) * scale[:, None]
    b = np.stack([np.cos(ang + 0.3), np.sin(ang + 0.3), rng.uniform(-0.5, 0.5, n)], axis=1) * scale[:, None]
    v = np.concatenate([np.zeros((1, 3)), a, b])
    i = np.arange(n)
    t = np.stack([np.zeros(n, np.int64), 1 + i, 1 + n + i], axis=1)
    # alone; normalised; on triangle normals already there and normalised; on vertex normals already there
    return T.mesh(v, t), [[("cvn", 0)], [("cvn", 1)], [("ctn", 1), ("cvn", 0)], [("cvn", 0), ("cvn", 0)], [("cvn", 0), ("cvn", 1)]]


def normalize():
    """zero, NaN in x only, NaN in y only, a squared norm that overflows, one that underflows to zero, plain ones: as given
    vertex normals and, through degenerate, huge and tiny triangles, as triangle normals"""
    vn = np.array([[0, 0, 0], [NAN, 1, 2], [1, NAN, 2], [1e200, 1e200, 0], [1e-200, 1e-200, 0], [3, 4, 12], [-0.0, 0, 0], [INF, 1, 1],
                   [1, 2, INF], [1e-170, 0, 0], [0, 0, NAN], [1, 1, 1]], np.float64)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1e160, 0, 0], [0, 1e160, 0], [1e-170, 0, 0], [0, 1e-170, 0], [0.5, 0.25, 3.0],
                  [1e155, 0, 1], [0, 1e155, 1], [NAN, 0, 0], [2, 2, 2]], np.float64)
    t = [[0, 1, 2], [0, 0, 1], [0, 3, 4], [0, 5, 6], [1, 2, 7], [0, 8, 9], [10, 1, 2], [7, 7, 7], [3, 4, 7], [11, 8, 4]]
    return T.mesh(v, t, vn), [[("norm",)], [("ctn", 1)], [("ctn", 0)], [("cvn", 1)], [("cvn", 0), ("norm",), ("norm",)]]


def tile(n):
    """nv = nt = n around compact.h's tile of 256: lattice vertices (so some coincide) and random triangles (so some repeat,
    as rotations too, and some are degenerate), every attribute"""
    rng = np.random.default_rng(1000 + n)
    v = rng.integers(0, 7, (n, 3)).astype(np.float64) * 0.5
    t = rng.integers(0, n, (n, 3))
    for k in range(0, n - 3, 7):
        t[k] = np.roll(t[k + 3], 1)                          # a repeat, rotated
    t[5::11, 1] = t[5::11, 0]                                # degenerate
    vn, vc, tn = _attrs(n, n, n)
    half = rng.permutation(n)[:n // 2]
    return T.mesh(v, t, vn, vc, tn), [[("purge",)], [("rdv",)], [("rdt",)], [("cvn", 1)], [("select", np.sort(half))],
                                      [("crop", (0.5, 0.0, 0.5), (2.5, 3.0, 2.0))]]


def big():
    """a 400 x 400 grid, 320,000 triangles, every third one repeated as a rotation (426,667 > 262,144: more than one scan chunk
    of 1,024 tiles), and a band of 3,000 vertices no triangle uses in its middle"""
    gv, gt = _grid(400, step=1.0 / 64.0, seed=2)
    band = np.stack([np.arange(3000) * 0.25, np.full(3000, -5.0), np.zeros(3000)], axis=1)
    at = 80000
    v = np.concatenate([gv[:at], band, gv[at:]])
    gt = np.where(gt >= at, gt + 3000, gt)
    rep = np.roll(gt[::3], 1, axis=1)
    t = np.concatenate([gt[:200000], rep, gt[200000:]])
    return T.mesh(v, t), [[("purge",)], [("cvn", 1)]]


def tiny():
    cases = {}
    some = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float64)
    progs = lambda nv: [[("purge",)], [("cvn", 1)], [("ctn", 1)], [("norm",)], [("select", np.arange(nv))], [("select", np.zeros(0, np.int64))],
                        [("crop", (-9.0, -9.0, -9.0), (9.0, 9.0, 9.0))], [("transform", _pose(5))]]
    cases["empty"] = T.mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32)), progs(0)
    cases["loose"] = T.mesh(some, np.zeros((0, 3), np.int32), some + 1.0, some * 0.1), progs(5)      # Purge removes them all
    cases["one"] = T.mesh(some[:3], [[0, 1, 2]]), progs(3)
    cases["degenerate"] = T.mesh(some[:2], [[0, 0, 1]]), progs(2)
    return cases


def _pose(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    M = np.eye(4)
    M[:3, :3] = q * rng.uniform(0.5, 2.0)
    M[:3, 3] = rng.normal(size=3)
    M[3] = rng.normal(size=4)                                # (the reference drops the fourth row: so must we)
    return M


def crop():
    """a 10 x 10 grid at multiples of 0.25 with one NaN vertex: bounds exactly on vertex coordinates (inclusive), a NaN bound,
    min > max in one component, a box that cuts through triangles"""
    v, t = _grid(10, step=0.25, seed=3)
    v[60, 2] = NAN
    vn, vc, tn = _attrs(len(v), len(t), 14)
    m = T.mesh(v, t, vn, vc, tn)
    return m, [[("crop", (0.5, 0.5, -1.0), (1.5, 1.75, 1.0))], [("crop", (0.5, NAN, -1.0), (1.5, 1.75, 1.0))],
               [("crop", (0.5, 0.5, -1.0), (1.5, 0.25, 1.0))], [("crop", (0.6, 0.3, -0.2), (1.9, 2.2, 0.2))],
               [("crop", (-INF, -INF, -INF), (INF, INF, INF))], [("crop", (0.5, 0.5, 1.0), (0.5, 0.5, 1.0))]]


def select():
    """duplicate indices; every vertex of a triangle but one; everything; nothing"""
    v, t = _grid(10, step=0.25, seed=4)
    vn, vc, tn = _attrs(len(v), len(t), 15)
    m = T.mesh(v, t, vn, vc, tn)
    nv = len(v)
    some = np.array([0, 1, 11, 12, 12, 1, 0, 0, 23, 22, 11, 5], np.int64)
    return m, [[("select", some)], [("select", np.arange(1, nv))], [("select", np.arange(nv))], [("select", np.zeros(0, np.int64))],
               [("select", np.arange(nv)[::-1].repeat(2))]]


def transform():
    v, t = _grid(4, step=0.5, seed=5)
    vn, vc, tn = _attrs(len(v), len(t), 16)
    hostile = _pose(7)
    hostile[0, 3], hostile[1, 3] = INF, NAN
    hostile[2, 0] = -0.0
    return T.mesh(v, t, vn, vc, tn), [[("transform", _pose(6))], [("transform", hostile)], [("transform", np.zeros((4, 4)))],
                                      [("ctn", 0), ("cvn", 0), ("transform", _pose(8))]]


@functools.lru_cache(maxsize=None)
def load():
    """-> {name: (mesh, programs)}; built once and left unchanged"""
    cases = dict(soup=soup(), keys=keys(), fan=fan(), normalize=normalize(), crop=crop(), select=select(), transform=transform(), big=big())
    for n in (255, 256, 257, 513):
        cases["tile%d" % n] = tile(n)
    cases.update(tiny())
    return cases


NAMES = ("soup", "keys", "fan", "normalize", "tile255", "tile256", "tile257", "tile513", "big", "empty", "loose", "one", "degenerate",
         "crop", "select", "transform")
# the fixture stores a result's rows in full where it has at most this many (vertices + triangles), else counts and SHA-256 only
FULL_ROWS = 150


@functools.lru_cache(maxsize=None)
def spec(name, p):
    """the specification's result of program p of a case, computed once -> (mesh, removed)"""
    m, programs = load()[name]
    return T.run(m, programs[p])


def items():
    return [(name, p) for name in NAMES for p in range(len(load()[name][1]))]


def encode(m, program):
    """a mesh and a program as the stream of doubles the reference harness (tests/golden/gen_trimesh.py) and the shim driver
    (tests/cpp/trimesh_driver.cpp) read"""
    out = [float(len(m["vertices"])), float(len(m["triangles"])), float(m["vertex_normals"] is not None),
           float(m["vertex_colors"] is not None), float(m["triangle_normals"] is not None)]
    parts = [np.array(out)]
    for k in T.ATTRS:
        if m[k] is not None:
            parts.append(np.asarray(m[k], np.float64).reshape(-1))
    parts.append(np.array([float(len(program))]))
    for op, *arg in program:
        parts.append(np.array([float(T.OPS.index(op))]))
        if op in ("ctn", "cvn"):
            parts.append(np.array([float(arg[0])]))
        elif op == "select":
            parts.append(np.concatenate([[float(len(arg[0]))], np.asarray(arg[0], np.float64).reshape(-1)]))
        elif op == "crop":
            parts.append(np.concatenate([np.asarray(arg[0], np.float64), np.asarray(arg[1], np.float64)]))
        elif op == "transform":
            parts.append(np.asarray(arg[0], np.float64).reshape(-1))
    return np.concatenate(parts).astype("<f8").tobytes()


def bits(a):
    """what is compared: the rows' bits (uint64 for f64 rows, the int32 indices as they are), every NaN as ONE pattern -- the
    sign and payload of a NaN an operation MAKES belong to the hardware (x86's inf - inf is a negative quiet NaN, gfx950's a
    positive one), not to the reference"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64:
        return a
    a = a.copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def raw_rows(m):
    """the bytes a SHA-256 is taken of: every attribute's rows in ATTRS' order, as bits() gives them"""
    return b"".join(bits(m[k]).tobytes() for k in T.ATTRS if m[k] is not None)
