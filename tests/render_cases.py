"""The scenes of the mesh renderer's tests: every case is a dict(V, F, w, h, K, E, z_near, z_far, encoding) that
tests/render_spec.py, render_host and TriMesh.render all take.  SPEC_SCENES are the general scenes that test_render_spec.py
pins against exact rational arithmetic, TIE_SCENES the ones whose arithmetic is exact in f64, CULL_SCENES degenerate triangles
and triangles at z_near (where the screen box of the rule decides), LARGE_SCENES the ones for the large path of render.hip,
CASES everything (by name), INVALID the argument sets every entry point refuses.  stride() is the one scene too large for
the numpy rule; hostile_depth() and stepped_depth() are depth images for the edge rule."""
import numpy as np

K_ANCHOR = (20.3, 19.7, 15.37, 11.61)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose(t, axis=(0, 0, 1), angle=0.0):
    E = np.eye(4)
    E[:3, :3] = rotation(axis, angle) if angle else np.eye(3)
    E[:3, 3] = t
    return E


def icosphere(subdivisions=1):
    p = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                mid[k] = len(V) - 1
            return mid[k]

        for a, b, c in F:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = out
    return np.asarray(V, np.float64), np.asarray(F, np.int32)


def torus(R=1.0, r=0.4, nu=12, nv=8):
    V, F = [], []
    for i in range(nu):
        for j in range(nv):
            u, v = 2 * np.pi * i / nu, 2 * np.pi * j / nv
            V.append(((R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)))
            a, b = i * nv + j, i * nv + (j + 1) % nv
            c, d = ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv
            F += [(a, c, b), (b, c, d)]
    return np.asarray(V, np.float64), np.asarray(F, np.int32)


def box(hx=0.5, hy=0.4, hz=0.3):
    V = np.array([(sx * hx, sy * hy, sz * hz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    F = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                  (1, 5, 7), (1, 7, 3)], np.int32)
    return V, F


def case(V, F, w, h, K, E, z_near=0.05, z_far=10.0, encoding=0):
    return dict(V=np.ascontiguousarray(V, np.float64).reshape(-1, 3), F=np.ascontiguousarray(F, np.int32).reshape(-1, 3), w=w, h=h,
                K=tuple(float(x) for x in K), E=np.ascontiguousarray(E, np.float64), z_near=z_near, z_far=z_far, encoding=encoding)


def with_(c, **kw):
    out = dict(c)
    out.update(kw)
    return out


SPHERE = icosphere(1)

# ---- the general scenes: the spec against exact rationals ----
SPEC_SCENES = {
    "sphere_anchor": case(*SPHERE, 32, 24, K_ANCHOR, pose((0.1234567, -0.0765432, 3.0))),
    "sphere_tilted": case(*SPHERE, 32, 24, K_ANCHOR, pose((-0.2134567, 0.1365432, 2.6), (1.0, 2.0, 3.0), 0.7)),
    "torus_rotated": case(*torus(), 32, 24, K_ANCHOR, pose((0.0934567, 0.0565432, 3.4), (2.0, -1.0, 0.5), 1.1)),
    "box_rotated": case(*box(), 32, 24, K_ANCHOR, pose((-0.0834567, 0.0465432, 2.2), (1.0, 1.0, -0.3), 0.9)),
}

# ---- the tie scenes: fx = fy = 16, integer cx, cy, vertices on z = 1 that project onto pixel centres: exact in f64 ----
K_TIE = (16.0, 16.0, 8.0, 6.0)


def on_pixel(u, v, z=1.0):
    return ((u - K_TIE[2]) / K_TIE[0] * z, (v - K_TIE[3]) / K_TIE[1] * z, z)


SQUARE_V = np.array([on_pixel(4, 2), on_pixel(12, 2), on_pixel(12, 10), on_pixel(4, 10)], np.float64)
TIE_SCENES = {
    "tie_square": case(SQUARE_V, [(0, 1, 2), (0, 2, 3)], 17, 13, K_TIE, np.eye(4)),
    "tie_square_swapped": case(SQUARE_V, [(0, 2, 3), (0, 1, 2)], 17, 13, K_TIE, np.eye(4)),
    "tie_square_one_reversed": case(SQUARE_V, [(0, 1, 2), (0, 3, 2)], 17, 13, K_TIE, np.eye(4)),
    "tie_two_copies": case(SQUARE_V, [(0, 1, 2), (0, 2, 3), (0, 1, 2), (0, 2, 3)], 17, 13, K_TIE, np.eye(4)),
}


def scaled(K, s):
    return tuple(x * s for x in K)


def _crowd():
    """one triangle over the whole 64 x 48 image at z = 3, and 2048 triangles of under a pixel between z = 1.5 and 4.5"""
    rng = np.random.default_rng(7)
    K = scaled(K_ANCHOR, 2.0)
    V = [(-30.0, -30.0, 3.0), (60.0, -30.0, 3.0), (-30.0, 60.0, 3.0)]
    F = [(0, 1, 2)]
    for _ in range(2048):
        z = rng.uniform(1.5, 4.5)
        u, v = rng.uniform(-2, 66), rng.uniform(-2, 50)
        base = len(V)
        for _ in range(3):
            du, dv = rng.uniform(-0.6, 0.6, 2)
            V.append(((u + du - K[2]) / K[0] * z, (v + dv - K[3]) / K[1] * z, z + rng.uniform(-0.01, 0.01)))
        F.append((base, base + 1, base + 2))
    return case(V, F, 64, 48, K, np.eye(4))


def _planes():
    """triangles against the planes: one straddling z_near, one with a vertex at z <= 0, one wholly behind the camera, one
    beyond z_far, and an ordinary one"""
    V = [(-0.5, -0.4, 0.02), (0.6, -0.3, 1.5), (-0.2, 0.7, 2.5),          # straddles z_near = 0.05
         (0.3, 0.2, -0.7), (0.9, 0.1, 1.2), (0.4, 0.8, 1.9),              # a vertex behind the camera
         (-0.3, -0.2, -1.0), (0.3, -0.2, -2.0), (0.0, 0.4, -1.5),         # wholly behind
         (-2.0, -2.0, 11.0), (2.0, -2.0, 12.0), (0.0, 2.0, 11.5),         # beyond z_far = 10
         (-0.9, -0.6, 2.0), (-0.1, -0.5, 2.2), (-0.6, 0.3, 2.1)]          # ordinary
    return case(V, np.arange(15).reshape(-1, 3), 32, 24, K_ANCHOR, np.eye(4))


def _at_zero():
    """two vertices exactly at z = 0 (on the camera's plane), before an ordinary triangle"""
    V = [(0.1, 0.1, 0.0), (0.5, -0.6, 0.9), (-0.7, 0.2, 0.0), (-0.9, -0.6, 2.0), (0.9, -0.5, 2.2), (-0.6, 0.6, 2.1)]
    return case(V, np.arange(6).reshape(-1, 3), 32, 24, K_ANCHOR, np.eye(4))


def _degenerate():
    """a zero-area triangle, one with a repeated index, one with a NaN and one with an infinite vertex, beside a real one"""
    V = [(-0.5, -0.5, 2.0), (0.5, -0.5, 2.0), (0.0, 0.5, 2.5),
         (-0.4, 0.1, 1.5), (0.0, 0.1, 1.5), (0.4, 0.1, 1.5),               # collinear
         (np.nan, 0.0, 1.0), (np.inf, 0.0, 1.0), (0.2, 0.3, -np.inf)]
    F = [(0, 1, 2), (3, 4, 5), (0, 0, 2), (1, 1, 1), (0, 1, 6), (0, 7, 2), (8, 1, 2)]
    return case(V, F, 32, 24, K_ANCHOR, np.eye(4))


def _in_plane():
    """the camera centre lies in the first triangle's plane (y = 0 in camera space); the second is ordinary"""
    V = [(-1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (0.0, 0.0, 3.0), (-0.5, 0.25, 2.0), (0.5, 0.25, 2.0), (0.0, 0.75, 2.0)]
    return case(V, [(0, 1, 2), (3, 4, 5)], 32, 24, (20.0, 20.0, 16.0, 12.0), np.eye(4))


# ---- the cull scenes: degenerate triangles and triangles at z_near, where the screen box of the set-up decides what is drawn
# (tests/render_spec.py says why).  32 x 24, K_ANCHOR, the identity pose; 32 triangles of one family, then an ordinary one ----
ORDINARY = [(-0.9, -0.6, 2.0), (-0.1, -0.5, 2.2), (-0.6, 0.3, 2.1)]
Z_NEAR = np.float64(0.05)
# vertices on a line through the camera centre (A, 1.875 A, 2.877 A as f64 rounds them): without its box, the f64 rule draws
# 114 pixels of this one and exact arithmetic none
THROUGH_EYE = [(-1.9497018957993624, 1.9116441622785438, 3.161161949725916),
               (-3.655993544165771, 3.584629389287803, 5.9276690991378835),
               (-5.6083898302206, 5.498915347942429, 9.093199616167162)]


def _in_view(rng, z, margin=4.0):
    """a camera-space point at depth z that projects into the 32 x 24 image or up to `margin` pixels beside it"""
    u, v = rng.uniform(-margin, 31 + margin), rng.uniform(-margin, 23 + margin)
    return np.array([(u - K_ANCHOR[2]) / K_ANCHOR[0] * z, (v - K_ANCHOR[3]) / K_ANCHOR[1] * z, z])


def _cull_scene(triangles):
    V = [p for t in triangles for p in t] + ORDINARY
    return case(V, np.arange(len(V)).reshape(-1, 3), 32, 24, K_ANCHOR, np.eye(4))


def _sliver_through_eye():
    rng = np.random.default_rng(11)
    T = [THROUGH_EYE]
    for _ in range(31):
        A = _in_view(rng, rng.uniform(1.0, 3.3))
        T.append([A, A * rng.uniform(1.3, 2.0), A * rng.uniform(2.2, 3.0)])
    return _cull_scene(T)


def _sliver_collinear():
    """three points of one line that misses the camera centre, the third as f64 rounds A + t (B - A)"""
    rng = np.random.default_rng(12)
    T = []
    for _ in range(32):
        A, B = _in_view(rng, rng.uniform(1.0, 4.0)), _in_view(rng, rng.uniform(1.0, 4.0))
        T.append([A, B, A + rng.uniform(-0.5, 1.5) * (B - A)])
    return _cull_scene(T)


def _sliver_tiny():
    rng = np.random.default_rng(13)
    T = []
    for _ in range(32):
        A = _in_view(rng, rng.uniform(1.0, 4.0), 0.0)
        T.append([A, A + 1e-9 * rng.uniform(-1, 1, 3), A + 1e-9 * rng.uniform(-1, 1, 3)])
    return _cull_scene(T)


def _under_near():
    """every vertex at z_near (1 - u), 0 < u <= 6e-16: one to four ulps under z_near, never on it"""
    rng = np.random.default_rng(14)
    T = []
    for _ in range(32):
        tri = []
        for _ in range(3):
            z = min(Z_NEAR * (1.0 - rng.uniform(0.0, 6e-16)), np.nextafter(Z_NEAR, 0.0))
            tri.append(_in_view(rng, z, 12.0))
        T.append(tri)
    return _cull_scene(T)


def _astride_near_by_an_ulp():
    """one and two vertices exactly at z_near, the others one ulp under it: the whole image is the box"""
    rng = np.random.default_rng(15)
    under = np.nextafter(Z_NEAR, 0.0)
    T = [[_in_view(rng, z, 12.0) for z in zs] for zs in ((Z_NEAR, under, under), (under, Z_NEAR, Z_NEAR))]
    return _cull_scene(T)


CULL_SCENES = {
    "sliver_through_eye": _sliver_through_eye(),
    "sliver_collinear": _sliver_collinear(),
    "sliver_tiny": _sliver_tiny(),
    "under_near": _under_near(),
    "astride_near_by_an_ulp": _astride_near_by_an_ulp(),
}

# ---- the large path (render.hip): a triangle whose box has more than SMALL_AREA pixels is cut into items of CHUNK box pixels,
# through an ordered compaction over tiles of TILE triangles whose passes stride beyond STRIDE triangles ----
SMALL_AREA, CHUNK, TILE = 64, 4096, 256
STRIDE = 2048 * TILE


def camera(w, h):
    """K_ANCHOR's field of view on a w x h image"""
    m = max(w, h)
    return (20.3 / 32 * m, 19.7 / 32 * m, 15.37 / 32 * w, 11.61 / 24 * h)


# it straddles z_near, so its box is the whole image whatever the camera: the plane z = 2.87 or so behind the sphere's cap
STRADDLER = [(-30.0, -30.0, 4.3), (60.0, -30.0, 4.2), (-30.0, 60.0, 0.02)]


def _chunk_scene(w, h):
    """the sphere (80 triangles) and the straddling triangle behind it, as triangle 80"""
    V, F = SPHERE
    t = (0.1234567, -0.0765432, 3.0)
    return case(np.concatenate([V, np.asarray(STRADDLER) - t]), np.concatenate([F, [[len(V), len(V) + 1, len(V) + 2]]]), w, h,
                camera(w, h), pose(t))


# name: (w, h); w h is the straddler's box area: SMALL_AREA exactly, the first large area, one item short of a full chunk, one
# full item, a second item of one pixel, a second item of 2403 pixels (nine full rounds of 256 lanes, then a break at lane 99;
# a prime row length), four items
CHUNK_SIZES = {"chunk_8x8": (8, 8), "chunk_13x5": (13, 5), "chunk_65x63": (65, 63), "chunk_64x64": (64, 64),
               "chunk_241x17": (241, 17), "chunk_97x67": (97, 67), "chunk_130x100": (130, 100)}
CHUNK_SCENES = {name: _chunk_scene(w, h) for name, (w, h) in CHUNK_SIZES.items()}


def _plane_triangle(rng, z0=(3.0, 3.05), tilt=0.05):
    """a triangle of 120 units a side in the plane z = z0 + a x + b y: it fills any frame, and its box is the whole image"""
    z0, a, b = rng.uniform(*z0), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt)
    return [(x, y, z0 + a * x + b * y) for x, y in ((-40.0, -40.0), (80.0, -40.0), (-40.0, 80.0))]


def _speck(rng, K, w, h, z=(1.5, 2.5), size=1.5):
    """a triangle of a few pixels in front of the planes"""
    z = rng.uniform(*z)
    u, v = rng.uniform(0, w - 1), rng.uniform(0, h - 1)
    out = []
    for _ in range(3):
        du, dv = rng.uniform(-size, size, 2)
        out.append(((u + du - K[2]) / K[0] * z, (v + dv - K[3]) / K[1] * z, z + rng.uniform(-0.01, 0.01)))
    return out


def _behind(rng):
    return [(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3.0, -0.5)) for _ in range(3)]


MANY_LARGE_KINDS = np.random.default_rng(21).permutation(["large"] * 600 + ["small"] * 100 + ["culled"] * 60)


def _many_large():
    """600 frame-filling triangles (two items each: 1200 items), 100 of a few pixels and 60 culled ones, interleaved by a
    seeded permutation: 760 triangles in three compaction tiles.  The planes' depths differ at every pixel (random tilts)"""
    rng = np.random.default_rng(22)
    w, h = 97, 67
    K = camera(w, h)
    make = {"large": lambda: _plane_triangle(rng), "small": lambda: _speck(rng, K, w, h), "culled": lambda: _behind(rng)}
    V = [p for kind in MANY_LARGE_KINDS for p in make[kind]()]
    return case(V, np.arange(len(V)).reshape(-1, 3), w, h, K, np.eye(4))


LARGE_SCENES = dict(CHUNK_SCENES)
LARGE_SCENES["many_large"] = _many_large()

STRIDE_TRIANGLES = STRIDE + 300
_STRIDE = []


def stride():
    """-> the case, the indices of its large triangles, those of its small ones.  2048 x 256 + 300 triangles, nearly all
    of them random triples of 100 vertices behind the camera; 80 frame-filling and 120 small triangles with vertices of their
    own are scattered through the index range, 6 and 10 of them beyond 2048 x 256.  Built once (read-only)"""
    if not _STRIDE:
        rng = np.random.default_rng(31)
        w, h = 97, 67
        K = camera(w, h)
        V = [p for _ in range(34) for p in _behind(rng)][:100]
        F = rng.integers(0, len(V), (STRIDE_TRIANGLES, 3)).astype(np.int32)
        at = np.concatenate([rng.choice(STRIDE, 184, replace=False), STRIDE + rng.choice(300, 16, replace=False)])
        large, small = np.sort(np.concatenate([at[:74], at[184:190]])), np.sort(np.concatenate([at[74:184], at[190:]]))
        for t in np.sort(at):
            tri = _plane_triangle(rng) if t in large else _speck(rng, K, w, h)
            F[t] = (len(V), len(V) + 1, len(V) + 2)
            V += tri
        c = case(V, F, w, h, K, np.eye(4))
        for a in (c["V"], c["F"], large, small):
            a.setflags(write=False)
        _STRIDE.append((c, large, small))
    return _STRIDE[0]


CASES = dict(SPEC_SCENES)
CASES.update(TIE_SCENES)
CASES.update({
    "sphere_1x1": case(*SPHERE, 1, 1, (20.3, 19.7, 0.37, 0.11), pose((0.1234567, -0.0765432, 3.0))),
    "sphere_17x13": case(*SPHERE, 17, 13, scaled(K_ANCHOR, 0.53), pose((0.1234567, -0.0765432, 3.0))),
    "sphere_64x48": case(*SPHERE, 64, 48, scaled(K_ANCHOR, 2.0), pose((0.1234567, -0.0765432, 3.0))),
    "sphere_close_64x48": case(*SPHERE, 64, 48, scaled(K_ANCHOR, 2.0), pose((0.05, -0.03, 1.4), (0.3, 1.0, 0.2), 0.4)),
    "empty_mesh": case(SPHERE[0], np.zeros((0, 3), np.int32), 17, 13, K_ANCHOR, np.eye(4)),
    "no_vertices": case(np.zeros((0, 3)), np.zeros((0, 3), np.int32), 17, 13, K_ANCHOR, np.eye(4)),
    "crowd": _crowd(),
    "planes": _planes(),
    "at_zero": _at_zero(),
    "degenerate": _degenerate(),
    "inside_box": case(*box(1.0, 0.8, 1.2), 32, 24, K_ANCHOR, pose((0.1, -0.05, 0.2), (0.2, 1.0, 0.1), 0.5)),
    "in_plane": _in_plane(),
    "negative_focal": case(*SPHERE, 32, 24, (-20.3, 19.7, 15.37, 11.61), pose((0.1234567, -0.0765432, 3.0))),
})
CASES.update({
    "sphere_anchor_depth_buffer": with_(CASES["sphere_anchor"], encoding=1),
    "crowd_depth_buffer": with_(CASES["crowd"], encoding=1),
    "planes_depth_buffer": with_(CASES["planes"], encoding=1),
    "tie_two_copies_depth_buffer": with_(CASES["tie_two_copies"], encoding=1),
})
OLD_NAMES = list(CASES)                                  # the scenes whose picture the box of the rule does not change
CASES.update(CULL_SCENES)
CASES.update(LARGE_SCENES)
NAMES = list(CASES)

# ---- what every entry point refuses: (name, the changed arguments of sphere_anchor) ----
_E_NAN = pose((0.1, 0.0, 3.0)); _E_NAN[1, 2] = np.nan
INVALID = [
    ("w_zero", dict(w=0)), ("h_zero", dict(h=0)), ("w_negative", dict(w=-3)), ("h_negative", dict(h=-1)),
    ("fx_zero", dict(K=(0.0, 19.7, 15.37, 11.61))), ("fy_zero", dict(K=(20.3, 0.0, 15.37, 11.61))),
    ("z_near_zero", dict(z_near=0.0)), ("z_near_negative", dict(z_near=-0.05)),
    ("z_far_equal", dict(z_near=1.0, z_far=1.0)), ("z_far_below", dict(z_near=1.0, z_far=0.5)),
    ("fx_nan", dict(K=(np.nan, 19.7, 15.37, 11.61))), ("cy_inf", dict(K=(20.3, 19.7, 15.37, np.inf))),
    ("z_near_nan", dict(z_near=np.nan)), ("z_far_inf", dict(z_far=np.inf)), ("extrinsic_nan", dict(E=_E_NAN)),
    ("encoding_unknown", dict(encoding=2)),
]


def spec(c, unboxed=False):
    """-> depth, index, mask, edges of tests/render_spec.py (edges of the metric depth, whatever the encoding)"""
    import render_spec as S
    args = (c["V"], c["F"], c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"])
    depth, index, mask, _ = S.render(*args, c["encoding"], unboxed=unboxed)
    metric = depth if c["encoding"] == S.METRIC else S.render(*args, unboxed=unboxed)[0]
    return depth, index, mask, S.edges(metric)


def boxes(c):
    """-> the box of the rule per triangle: (x0, y0, x1, y1), or None where it draws nothing"""
    import render_spec as S
    P = S.camera_points(c["V"], c["E"])
    return [S.setup_box(P[a], P[b], P[d], c["w"], c["h"], c["K"], c["z_near"]) for a, b, d in c["F"]]


def box_area(b):
    return 0 if b is None else (b[2] - b[0] + 1) * (b[3] - b[1] + 1)


def items(b):
    """the items of the large path a triangle with box b becomes"""
    return -(-box_area(b) // CHUNK) if box_area(b) > SMALL_AREA else 0


_SPEC = {}


def spec_of(name):
    """the spec's images of a case, computed once and shared (read-only)"""
    if name not in _SPEC:
        out = spec(CASES[name])
        for a in out:
            a.setflags(write=False)
        _SPEC[name] = out
    return _SPEC[name]


def host(lib, c):
    return lib.render_host(c["V"], c["F"], c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"], c["encoding"])


def hostile_depth():
    """a 12 x 16 depth image (interior: rows 5, 6, columns 5 .. 10) with holes, and a NaN, an infinity, a negative, -0.0, a
    denormal and -inf each as the centre of an interior pixel and as a neighbour of one; two infinities opposite each other
    around (5, 9): a NaN delta"""
    rng = np.random.default_rng(3)
    d = rng.uniform(0.5, 0.8, (12, 16)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.2] = 0.0
    d[3, 3], d[7, 9], d[5, 5] = np.nan, np.inf, -1.0
    denormal = np.float32(1e-45)
    assert 0.0 < denormal < np.finfo(np.float32).tiny
    d[5, 6], d[5, 8], d[6, 6], d[6, 9], d[6, 7] = np.nan, -0.0, denormal, -np.inf, np.inf               # centres
    d[4, 7], d[4, 10], d[7, 5], d[7, 7], d[4, 4], d[7, 11] = np.nan, -0.0, denormal, -np.inf, -1.0, np.inf   # neighbours only
    d[4, 8], d[6, 10], d[5, 9] = np.inf, np.inf, 0.7                     # NW and SE of (5, 9)
    return d


def stepped_depth(w, h, seed):
    """depths 1, 1.5 and 2 and a few holes, pixel by pixel: an edge nearly everywhere"""
    rng = np.random.default_rng(seed)
    d = (1.0 + 0.5 * rng.integers(0, 3, (h, w))).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.05] = 0.0
    return d


# w x h: no interior (w or h <= 10) three times, one interior pixel, rows that cross the blocks of 256 pixels both ways
EDGE_SHAPES = ((1, 1), (10, 40), (40, 10), (11, 11), (11, 300), (300, 11))


def stride_host(lib):
    """render_host's images of the stride scene, computed once and shared (read-only)"""
    if len(_STRIDE) < 2:
        out = host(lib, stride()[0])
        for a in out:
            a.setflags(write=False)
        _STRIDE.append(out)
    return _STRIDE[1]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
