"""The scenes of the mesh renderer's tests: every case is a dict(V, F, w, h, K, E, z_near, z_far, encoding) that
tests/render_spec.py, render_host and TriMesh.render all take.  SPEC_SCENES are the general scenes that test_render_spec.py
pins against exact rational arithmetic, TIE_SCENES the ones whose arithmetic is exact in f64, CASES everything (by name),
INVALID the argument sets every entry point refuses."""
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


def spec(c):
    """-> depth, index, mask, edges of tests/render_spec.py (edges of the metric depth, whatever the encoding)"""
    import render_spec as S
    depth, index, mask, _ = S.render(c["V"], c["F"], c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"], c["encoding"])
    metric = depth if c["encoding"] == S.METRIC else S.render(c["V"], c["F"], c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"])[0]
    return depth, index, mask, S.edges(metric)


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
