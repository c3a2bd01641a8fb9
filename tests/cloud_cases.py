"""The inputs of the PointCloud tests, built from seeds (the fixture tests/golden/cloud.npz stores only what the compiled
reference made of them): load()[name] = (cloud, [program, ...]) with a cloud of tests/cloud_spec.py and programs of its run().
Each case is the smallest shape at which a kernel of cloud.hip can still go wrong; tests/golden/gen_cloud.py asserts, on the
reference, the properties that make it bite."""
import functools

import numpy as np

import cloud_spec as S

NAN, INF = float("nan"), float("inf")
CHUNK = 16384                                                # the library's kHostChunk


def _attrs(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)), rng.uniform(size=(n, 3))


def _pose(seed, junk_row=True):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    M = np.eye(4)
    M[:3, :3] = q * rng.uniform(0.5, 2.0)
    M[:3, 3] = rng.normal(size=3)
    if junk_row:
        M[3] = rng.normal(size=4)                            # (the reference drops the fourth row: so must we)
    return M


def tile(n):
    """n points around compact.h's tile of 256 on a lattice of quarters, x alternating 0.25 / 0.75, one NaN point in the
    middle of the last tile, normals and colours: crops that keep every second row, every row, none, rows on the bounds
    themselves, and an inverted bound"""
    rng = np.random.default_rng(2000 + n)
    p = rng.integers(0, 8, (n, 3)).astype(np.float64) * 0.25
    p[:, 0] = np.where(np.arange(n) % 2 == 0, 0.25, 0.75)
    p[n - 3, 1] = NAN
    p[256::256] = (0.25, 0.5, 0.25)                          # the first row of every later tile lies ON the fifth crop's bounds
    nrm, col = _attrs(n, n)
    big = (9.0, 9.0, 9.0)
    return S.cloud(p, nrm, col), [[("crop", (0.5, -9.0, -9.0), big)],                       # every second row
                                  [("crop", (-9.0, -9.0, -9.0), big)],                     # all but the NaN point
                                  [("crop", (-INF, -INF, -INF), (INF, INF, INF))],         # ... which fails an infinite box too
                                  [("crop", (2.0, 2.0, 2.0), big)],                        # none
                                  [("crop", (0.25, 0.5, 0.25), (0.25, 1.25, 1.75))],       # the bounds are lattice values: included
                                  [("crop", (0.0, 1.0, 0.0), (9.0, 0.5, 9.0))],            # inverted in y
                                  [("crop", (0.0, NAN, 0.0), big)]]                        # a NaN bound fails every test


def big():
    """524,288 + 257 points (2,050 tiles: the grid cap of 2,048 workgroups strides, the scan carries over 1,024 tiles), points
    alone (12.6 MB), through crop, transform, bounds and uniform (k = 7)"""
    rng = np.random.default_rng(31)
    n = 524288 + 257
    p = np.round(rng.uniform(-4.0, 4.0, (n, 3)) * 4096.0) / 4096.0
    return S.cloud(p), [[("crop", (-3.0, -3.5, -4.0), (3.5, 3.0, 3.75)), ("transform", _pose(32)), ("bounds",), ("uniform", 7), ("bounds",)]]


def sums(n, seed):
    """n points whose magnitudes spread over 2^+-30: the order of an f64 sum shows in its last bits"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)) * np.exp2(rng.integers(-30, 31, (n, 1)).astype(np.float64))
    return S.cloud(p), [[("meancov",)], [("mahal",)]]


def planar():
    """every z is 0: a singular covariance, whose inverse is inf and NaN"""
    rng = np.random.default_rng(33)
    p = rng.normal(size=(300, 3))
    p[:, 2] = 0.0
    return S.cloud(p), [[("meancov",)], [("mahal",)]]


def one():
    return S.cloud([[0.5, -2.0, 3.0]], [[0.0, 0.0, 2.0]], [[0.1, 0.2, 0.3]]), [
        [("meancov",)], [("mahal",)], [("bounds",)], [("norm",)], [("crop", (0.5, -2.0, 3.0), (0.5, -2.0, 3.0))],
        [("uniform", 5)], [("append", None)], [("transform", _pose(34))], [("orient_cam", (0.5, -2.0, 3.0))]]


def empty():
    e = S.cloud(np.zeros((0, 3)))
    return e, [[("meancov",)], [("mahal",)], [("bounds",)], [("norm",)], [("paint", (0.1, 0.2, 0.3))],
               [("crop", (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))], [("uniform", 2)], [("select", np.zeros(0, np.int64))],
               [("append", None)], [("transform", _pose(35))]]


def _bounds_case(x):
    """a cloud whose three coordinates are rotations of one hostile column: every axis sees it"""
    x = np.asarray(x, np.float64)
    return S.cloud(np.stack([x, np.roll(x, 1), np.roll(x, 2)], axis=1)), [[("bounds",)]]


def bounds_cases():
    rng = np.random.default_rng(36)
    body = rng.normal(size=40)
    last = rng.normal(size=256 + 37)                         # 293 rows: the last wave of the second tile is partial
    last[-1] = 77.0
    low = last.copy()
    low[-1] = -77.0
    return {
        "bounds_nan_first": _bounds_case(np.concatenate([[NAN], body])),
        "bounds_nan_middle": _bounds_case(np.concatenate([body[:20], [NAN, NAN], body[20:]])),
        "bounds_all_nan": _bounds_case(np.full(7, NAN)),
        "bounds_zero_pos_first": _bounds_case([0.0, -0.0, 0.0, -0.0]),
        "bounds_zero_neg_first": _bounds_case([-0.0, 0.0, -0.0, 0.0]),
        "bounds_inf": _bounds_case(np.concatenate([body[:10], [INF, -INF, NAN], body[10:]])),
        "bounds_last_max": _bounds_case(last),
        "bounds_last_min": _bounds_case(low),
    }


def select():
    """duplicates, reversed, nothing, more indices than points"""
    p = np.arange(60, dtype=np.float64).reshape(20, 3) * 0.5
    nrm, col = _attrs(20, 37)
    n = 20
    return S.cloud(p, nrm, col), [[("select", np.array([3, 3, 0, 19, 3, 7, 7], np.int64))], [("select", np.arange(n)[::-1])],
                                  [("select", np.zeros(0, np.int64))], [("select", np.arange(3 * n) % n)],
                                  [("select", np.arange(600) * 7 % n)]]


def uniform():
    n = 23
    p = np.arange(3 * n, dtype=np.float64).reshape(n, 3) * 0.25
    nrm, col = _attrs(n, 38)
    return S.cloud(p, nrm, col), [[("uniform", k)] for k in (0, 1, 2, n - 1, n, n + 1)]


KINDS = ("empty", "plain", "normals", "colors", "both")


def _kind(kind, n, seed):
    if kind == "empty":
        return S.cloud(np.zeros((0, 3)))
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    nrm, col = _attrs(n, seed + 1)
    return S.cloud(p, nrm if kind in ("normals", "both") else None, col if kind in ("colors", "both") else None)


def append_cases():
    """every combination of (empty, plain, normals, colours, both) on both sides, and the cloud onto itself"""
    out = {}
    for i, lhs in enumerate(KINDS):
        out["append_" + lhs] = _kind(lhs, 5, 40 + 2 * i), [[("append", _kind(rhs, 4, 60 + 2 * j))] for j, rhs in enumerate(KINDS)] + [[("append", None)]]
    return out


def transform():
    rng = np.random.default_rng(39)
    p = rng.normal(size=(70, 3))
    nrm, col = _attrs(70, 39)
    nan_t, inf_t = _pose(41, False), _pose(42, False)
    nan_t[1, 3] = NAN
    inf_t[0, 3], inf_t[2, 3], inf_t[2, 0] = INF, -INF, -0.0
    affine = _pose(43, False)
    affine[:3, :3] = rng.normal(size=(3, 3))
    return S.cloud(p, nrm, col), [[("transform", affine)], [("transform", nan_t)], [("transform", inf_t)], [("transform", _pose(44, True))],
                                  [("transform", _pose(45)), ("transform", _pose(46)), ("bounds",)]]


def normals():
    """zero, underflowing, overflowing, infinite and NaN normals, the camera on a point, a normal at right angles to the
    reference, -0.0"""
    nrm = np.array([[0, 0, 0], [1e-200, 1e-200, 0], [1e200, 1e200, 0], [NAN, 1, 2], [1, NAN, 2], [3, 4, 12], [-0.0, 0, 0],
                    [INF, 1, 1], [0, 0, 0], [-3, -4, -12], [1e-170, 0, 0], [0, 1, 0], [0, 0, NAN], [1, 1, 1], [0, -0.0, 0],
                    [-1e-200, 0, -1e-200]], np.float64)
    rng = np.random.default_rng(47)
    p = np.round(rng.normal(size=(len(nrm), 3)) * 8.0) / 8.0
    p[8] = (0.5, -1.25, 2.0)                                 # a zero normal here, and the camera below
    p[14] = (0.0, 0.0, 0.0)                                  # a zero normal here too: camera - point underflows in the squared norm below
    p[15] = (NAN, 0.0, 1.0)
    cam = (0.5, -1.25, 2.0)
    return S.cloud(p, nrm), [[("norm",)], [("orient_dir", (0.0, 0.0, 1.0))], [("orient_dir", (-1.0, 2.0, -0.5))], [("orient_dir", (0.0, 0.0, 0.0))],
                             [("orient_dir", (NAN, 0.0, 1.0))], [("orient_cam", cam)], [("orient_cam", (0.0, 0.0, 0.0))],
                             [("orient_cam", (1e-200, 0.0, -1e-200))], [("orient_cam", (INF, 0.0, 0.0))],
                             [("norm",), ("orient_cam", cam), ("norm",)], [("paint", (0.25, 0.5, 1.0)), ("norm",)]]


@functools.lru_cache(maxsize=None)
def load():
    """-> {name: (cloud, programs)}; built once and left unchanged"""
    cases = dict(big=big(), planar=planar(), one=one(), empty=empty(), select=select(), uniform=uniform(), transform=transform(),
                 normals=normals())
    for n in (255, 256, 257, 513):
        cases["tile%d" % n] = tile(n)
    for n in SUM_SIZES:
        cases["sums%d" % n] = sums(n, 3000 + n)
    cases.update(bounds_cases())
    cases.update(append_cases())
    return cases


SUM_SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
NAMES = (("tile255", "tile256", "tile257", "tile513", "big") + tuple("sums%d" % n for n in SUM_SIZES) + ("planar", "one", "empty")
         + ("bounds_nan_first", "bounds_nan_middle", "bounds_all_nan", "bounds_zero_pos_first", "bounds_zero_neg_first", "bounds_inf",
            "bounds_last_max", "bounds_last_min", "select", "uniform") + tuple("append_" + k for k in KINDS) + ("transform", "normals"))
# the fixture stores a result in full where it has at most this many rows (and its results this many doubles), else the counts
# and the SHA-256 only
FULL_ROWS = 100


@functools.lru_cache(maxsize=None)
def spec(name, p, chunk=None):
    """the specification's result of program p of a case, computed once -> (cloud, results)"""
    c, programs = load()[name]
    return S.run(c, programs[p], chunk)


def items():
    return [(name, p) for name in NAMES for p in range(len(load()[name][1]))]


def _encode_cloud(c):
    parts = [np.array([float(len(c["points"])), float(c["normals"] is not None), float(c["colors"] is not None)])]
    parts += [np.asarray(c[k], np.float64).reshape(-1) for k in S.ATTRS if c[k] is not None]
    return parts


def encode(c, program):
    """a cloud and a program as the stream of doubles the reference harness (tests/golden/gen_cloud.py) and the shim driver
    (tests/cpp/cloud_driver.cpp) read"""
    parts = _encode_cloud(c) + [np.array([float(len(program))])]
    for op, *arg in program:
        parts.append(np.array([float(S.OPS.index(op))]))
        if op in ("transform", "paint", "orient_dir", "orient_cam"):
            parts.append(np.asarray(arg[0], np.float64).reshape(-1))
        elif op == "append":
            parts += [np.array([1.0])] if arg[0] is None else [np.array([0.0])] + _encode_cloud(arg[0])
        elif op == "select":
            parts.append(np.concatenate([[float(len(arg[0]))], np.asarray(arg[0], np.float64).reshape(-1)]))
        elif op in ("uniform", "voxel"):
            parts.append(np.array([float(arg[0])]))
        elif op == "crop":
            parts.append(np.concatenate([np.asarray(arg[0], np.float64), np.asarray(arg[1], np.float64)]))
        elif op == "normals":
            parts.append(np.array([float(arg[0]), float(arg[1])]))          # Hybrid: radius, max_nn
    return np.concatenate(parts).astype("<f8").tobytes()


def bits(a):
    """what is compared: the f64 values' bits, every NaN as ONE pattern -- the sign and payload of a NaN an operation MAKES
    belong to the hardware (x86's inf - inf is a negative quiet NaN, gfx950's a positive one), not to the reference"""
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def flat_results(results):
    return np.concatenate([np.zeros(0)] + [np.asarray(r, np.float64).reshape(-1) for r in results])


def raw_rows(c, results):
    """the bytes a SHA-256 is taken of: every attribute's rows in ATTRS' order, then the results, as bits() gives them"""
    return b"".join(bits(c[k]).tobytes() for k in S.ATTRS if c[k] is not None) + bits(flat_results(results)).tobytes()
