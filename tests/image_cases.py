"""The named cases of the Image operations: what tests/golden/gen_image.py records from the compiled reference
(tests/golden/image.npz), tests/test_image_spec.py replays on the numpy specification (tests/image_spec.py) and
tests/test_image.py on the library.

A case is (inputs, program): the inputs are registers 0 .. k - 1, and each step of the program reads registers and appends
its result(s) as new ones (the two in-place steps change a register).  Everything that is compared is the list of registers
after the last step, and the results of the float_value_at steps.  A step is (op, arguments ...):

  ("to_float", r, type) ("depth_to_float", r, scale, trunc) ("from_float", r, bytes) ("filter", r, type)
  ("filter_separable", r, dx, dy) ("filter_horizontal", r, kernel) ("flip", r) ("downsample", r) ("dilate", r, k) ("copy", r)
  ("linear_transform", r, scale, offset) ("clip_intensity", r, min, max)          in place
  ("pyramid", r, levels, gauss)              appends its levels (none for an input that is not 1 x float)
  ("filter_pyramid", first, count, type)     over the registers first .. first + count - 1; appends count images
  ("distance_multiplier", intrinsic, w, h)
  ("float_value_at", r, uv)                  appends nothing; ok and value go to the results
  ("rgbd", color, depth, format, scale, trunc, convert)    appends color, depth (two empty images for different sizes)

Each case is the smallest shape at which a kernel can still go wrong: the shapes straddle a wave of 64 and the 64-wide
transpose tile in both directions (65 x 33, 33 x 65) and two tiles plus a remainder (130 x 67); the values hold NaN, both
infinities, -0.0, fp32 denormals and FLT_MAX next to each other within the reach of a 7-tap kernel.

SPEC_ONLY are the cases in which the reference has undefined behaviour (include/visma_icp.h states what the library does
instead): they are not in the fixture, tests/test_image_spec.py checks them against the header's words."""
import hashlib
import struct

import numpy as np

import image_spec as S

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FULL_BYTES = 4096                # registers of at most that many bytes are stored in full; larger ones by SHA-256 only
OPS = ("to_float", "depth_to_float", "from_float", "filter", "filter_separable", "filter_horizontal", "flip", "downsample", "dilate",
       "linear_transform", "clip_intensity", "pyramid", "filter_pyramid", "distance_multiplier", "float_value_at", "rgbd", "copy")
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 2), (65, 33), (33, 65), (130, 67))       # w x h
TAPS9 = [0.013, 0.07, 0.11, 0.2, 0.3, 0.17, 0.09, 0.04, 0.007]                                 # no weight is dyadic
TAPS71 = [((i * 37) % 19 - 9) / 97.0 for i in range(71)]
SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 1e-40, -3e-42, 1.4e-45, FLT_MAX, FLT_MAX, -FLT_MAX, 0.0, 1.0)


def hostile(w, h, seed):
    """values in [-2, 2] with the specials sprinkled in: next to each other along a row, and the same run down a column"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-2.0, 2.0, (h, w)).astype(F32)
    flat = a.reshape(-1)
    if flat.size >= 3 * len(SPECIALS):
        at = flat.size // 3
        flat[at:at + len(SPECIALS)] = np.array(SPECIALS, F32)            # along a row (and across its end in narrow images)
        if h > len(SPECIALS):
            a[h // 2 - 6:h // 2 - 6 + len(SPECIALS), w - 1] = np.array(SPECIALS, F32)      # down the last column
    elif flat.size > 1:
        flat[::2] = np.array(SPECIALS, F32)[:len(flat[::2])]
    return a


def shape_program(w, h):
    p = [("filter", 0, t) for t in range(5)]
    p += [("flip", 0), ("downsample", 0), ("filter_horizontal", 0, [0.7]), ("filter_horizontal", 0, TAPS9),
          ("filter_horizontal", 0, [0.25, 0.25, 0.25, 0.25]), ("filter_separable", 0, TAPS9, [0.1, 0.7, 0.2]),
          ("filter_separable", 0, [0.5, 0.5], [1.0]),
          ("copy", 0), ("linear_transform", 13, 1.7, -0.3), ("copy", 0), ("clip_intensity", 14, -0.5, 0.5)]
    if (w, h) == (65, 33):                                   # a kernel longer than a row, from the device buffer
        p += [("filter_horizontal", 0, TAPS71), ("filter_separable", 0, TAPS71, TAPS71), ("filter_separable", 0, [0.3], TAPS71)]
    return p


def _cases():
    c = {}
    for i, (w, h) in enumerate(SHAPES):
        c["shape_%dx%d" % (w, h)] = ([hostile(w, h, 100 + i)], shape_program(w, h))
    # FLT_MAX next to FLT_MAX: the down-sampler's sum and Sobel's 2 * FLT_MAX overflow, the Gaussians do not
    v = np.zeros((4, 16), F32)
    v[:, :] = np.array([0.5, FLT_MAX, FLT_MAX, FLT_MAX, 1.0, np.nan, 2.0, 1e-40, 1e-40, -0.0, -0.0, np.inf, 3.0, -np.inf, 1.4e-45, -1.4e-45], F32)
    v[2:, 5] = 7.0
    c["values"] = ([v], [("filter", 0, t) for t in range(5)] + [("downsample", 0), ("filter_horizontal", 0, TAPS9),
                                                                ("copy", 0), ("linear_transform", 8, 0.5, 0.0), ("copy", 0), ("clip_intensity", 9, 1e-40, 1.0)])
    # the nine channel x width combinations (and two channels: all zero), both intensity types, and as a depth
    rng = np.random.default_rng(7)
    for ch in (1, 2, 3):
        for dt in (np.uint8, np.uint16, F32):
            shape = (3, 5) if ch == 1 else (3, 5, ch)
            if dt == F32:
                a = rng.uniform(0.0, 3.0, shape).astype(F32)
                a.reshape(-1)[:4] = np.array([np.nan, 1e-40, -0.0, FLT_MAX], F32)
            else:
                a = rng.integers(0, np.iinfo(dt).max + 1, shape).astype(dt)
                a.reshape(-1)[:2] = (0, np.iinfo(dt).max)
            c["convert_%dx%d" % (ch, np.dtype(dt).itemsize)] = ([a], [("to_float", 0, S.EQUAL), ("to_float", 0, S.WEIGHTED),
                                                                      ("depth_to_float", 0, 1000.0, 3.0)])
    below = np.nextafter(F32(3.0), F32(0.0))
    c["depth_trunc"] = ([np.array([[3.0, below, 2.5, np.nan, np.inf, -1.0]], F32), np.array([[3000, 2999, 3001, 0, 65535, 1]], np.uint16)],
                        [("depth_to_float", 0, 1.0, 3.0), ("depth_to_float", 1, 1000.0, 3.0), ("depth_to_float", 0, 0.5, 6.0)])
    # CreateImageFromFloatImage where the cast is defined: the scaled values -0.5, 0.999 and 1.0 (truncation toward zero,
    # the first to 0), the last representable values, and an input that is not 1 x float
    f8 = np.array([[-0.5 / 255, 0.999 / 255, 1.0 / 255, 0.5, 0.999, 1.0, 0.0, -0.0, 0.25, 1e-40, 254.9 / 255, -0.9 / 255]], F32)
    f16 = np.array([[-0.5, 0.999, 1.0, 65535.0, 65534.9, 1234.5, 0.0, -0.0, -0.999, 1e-40, 255.9, 65535.99]], F32)
    c["from_float"] = ([f8, f16, np.zeros((2, 2), np.uint8)], [("from_float", 0, 1), ("from_float", 1, 2), ("from_float", 2, 1), ("from_float", 2, 2)])
    # the five RGB-D formats with and without the intensity conversion, and images of different sizes
    color = rng.integers(0, 256, (4, 6, 3)).astype(np.uint8)
    depth = rng.integers(0, 9000, (4, 6)).astype(np.uint16)
    depth.reshape(-1)[:3] = (4000, 3999, 20000)              # at and either side of the Redwood / TUM truncation (4 m at 1000 / 5000)
    sun = (rng.integers(0, 8000, (4, 6)).astype(np.uint16) << 3) | rng.integers(1, 8, (4, 6)).astype(np.uint16)
    sun.reshape(-1)[0] = 0xFFFF; sun.reshape(-1)[1] = 7
    swapped = rng.integers(100, 1000, (4, 6)).astype(np.uint16)
    swapped.reshape(-1)[:4] = (0, 1087, 1093, 65535)
    nyu = swapped.byteswap()
    gray = rng.uniform(0.0, 1.0, (4, 6)).astype(F32)
    prog = []
    for fmt, d in ((0, 1), (1, 1), (2, 1), (3, 2), (4, 3)):
        prog += [("rgbd", 0, d, fmt, 1000.0, 3.0, 1), ("rgbd", 0, d, fmt, 1000.0, 3.0, 0)]
    prog += [("rgbd", 4, 1, 0, 500.0, 2.0, 0), ("rgbd", 5, 1, 2, 1000.0, 3.0, 1), ("rgbd", 0, 6, 0, 1000.0, 3.0, 1)]
    c["rgbd"] = ([color, depth, sun, nyu, gray, np.zeros((4, 5, 3), np.uint8), depth.astype(F32)], prog)
    # dilate: a 255 in a corner with a 254 next to it, a few more, windows up to larger than the image
    d = np.zeros((33, 65), np.uint8)
    d[0, 0] = 255; d[0, 1] = 254; d[1, 0] = 254; d[32, 64] = 255; d[16, 40] = 255; d[20, 3] = 1
    c["dilate_65x33"] = ([d, d.astype(F32)], [("dilate", 0, k) for k in (-1, 0, 1, 3, 40)] + [("dilate", 1, 1)])
    c["dilate_7x1"] = ([np.array([[255, 254, 0, 0, 0, 0, 0]], np.uint8)], [("dilate", 0, k) for k in (-1, 0, 1, 3, 40)])
    # FloatValueAt: the corners, the clamp to w - 2, one ulp outside on each side, the interior; three channels: always false
    a = rng.uniform(-1.0, 1.0, (4, 5)).astype(F32)
    a[1, 1] = 1e-40
    up = lambda x: float(np.nextafter(x, np.inf))
    dn = lambda x: float(np.nextafter(x, -np.inf))
    uv = [(0.0, 0.0), (4.0, 3.0), (4.0, 0.0), (0.0, 3.0), (up(4.0), 1.0), (1.0, up(3.0)), (dn(0.0), 1.0), (1.0, dn(0.0)), (dn(4.0), dn(3.0)),
          (-0.0, -0.0), (1.5, 1.5), (2.25, 0.75), (3.0, 2.0), (3.999, 2.999), (0.1, 2.9), (np.inf, 1.0), (1.0, -np.inf), (1e300, 1.0)]
    c["value_at"] = ([a, np.zeros((4, 5, 3), F32), np.zeros((4, 5), np.uint16)], [("float_value_at", r, uv) for r in (0, 1, 2)])
    # pyramids: 33 -> 16 -> 8 -> 4 rows; more levels than the size allows (down to 0 x 0); an input without levels
    c["pyramid"] = ([hostile(65, 33, 31), np.zeros((4, 4), np.uint8)],
                    [("pyramid", 0, 4, 1), ("pyramid", 0, 4, 0), ("pyramid", 1, 3, 1), ("pyramid", 0, 9, 1), ("filter_pyramid", 2, 4, 1),
                     ("filter_pyramid", 10, 9, 4), ("pyramid", 0, 0, 1)])
    c["multiplier"] = ([], [("distance_multiplier", [525.0, 525.5, 3.2, 2.4], 7, 5), ("distance_multiplier", [0.7, 1e-3, -4.0, 1e4], 65, 3),
                            ("distance_multiplier", [1.0, 1.0, 0.0, 0.0], 0, 0)])
    # a front end: TUM frame -> pyramid -> Gaussian5 per level -> linear transform -> clip -> 8 bits
    color = rng.integers(0, 256, (17, 33, 3)).astype(np.uint8)
    depth = rng.integers(0, 30000, (17, 33)).astype(np.uint16)
    prog = [("rgbd", 0, 1, 2, 0.0, 0.0, 1), ("pyramid", 2, 3, 1), ("pyramid", 3, 3, 0), ("filter_pyramid", 4, 3, 1), ("filter_pyramid", 7, 3, 1)]
    for r in range(10, 16):
        prog += [("linear_transform", r, 4.0, -1.5), ("clip_intensity", r, 0.0, 1.0), ("from_float", r, 1)]
    c["front_end"] = ([color, depth], prog)
    return c


def _spec_only():
    c = {}
    bad8 = np.array([[np.nan, -1.0, -300.0, 2.0, np.inf, -np.inf, 1.01, -1.0 / 255]], F32)
    bad16 = np.array([[np.nan, -1.0, -70000.0, 65536.0, np.inf, -np.inf, 1e9, 65535.5]], F32)
    c["from_float_saturated"] = ([bad8, bad16], [("from_float", 0, 1), ("from_float", 1, 2)])
    swapped = np.array([[1088, 1089, 1090, 1091, 1092, 1087]], np.uint16)
    c["nyu_saturated"] = ([np.zeros((1, 6, 3), np.uint8), swapped.byteswap()], [("rgbd", 0, 1, 4, 0.0, 0.0, 1)])
    uv = [(0.0, 0.0), (0.5, 0.0), (np.nan, 1.0), (1.0, np.nan)]
    c["value_at_undefined"] = ([np.ones((4, 1), F32), np.ones((1, 4), F32), np.ones((3, 3), F32)], [("float_value_at", r, uv) for r in (0, 1, 2)])
    return c


_CACHE = {}


def load():
    if "cases" not in _CACHE:
        _CACHE["cases"] = _cases()
        _CACHE["spec_only"] = _spec_only()
    return _CACHE["cases"]


def spec_only():
    load()
    return _CACHE["spec_only"]


NAMES = tuple(_cases())
SPEC_ONLY = tuple(_spec_only())


def case(name):
    return load()[name] if name in load() else spec_only()[name]


class SpecOps:
    """the operations on numpy arrays; tests/test_image.py has the same interface over the library"""
    def upload(self, a): return a.copy()
    def download(self, r): return r
    def close(self, r): pass
    def empty(self): return S.EMPTY
    def to_float(self, r, t): return S.to_float(r, t)
    def depth_to_float(self, r, s, t): return S.depth_to_float(r, s, t)
    def from_float(self, r, b): return S.from_float(r, b)
    def filter(self, r, t): return S.filter(r, t)
    def filter_separable(self, r, dx, dy): return S.filter_separable(r, dx, dy)
    def filter_horizontal(self, r, k): return S.filter_horizontal(r, k)
    def flip(self, r): return S.flip(r)
    def downsample(self, r): return S.downsample(r)
    def dilate(self, r, k): return S.dilate(r, k)
    def copy(self, r): return r.copy()
    def linear_transform(self, r, s, o): r[...] = S.linear_transform(r, s, o)
    def clip_intensity(self, r, lo, hi): r[...] = S.clip_intensity(r, lo, hi)
    def pyramid(self, r, n, g): return S.pyramid(r, n, bool(g))
    def filter_pyramid(self, rs, t): return S.filter_pyramid(rs, t)
    def distance_multiplier(self, k, w, h): return S.distance_multiplier(k, w, h)
    def float_value_at(self, r, uv): return S.float_value_at(r, uv)
    def rgbd(self, c, d, fmt, s, t, conv): return S.rgbd(c, d, fmt, s, t, bool(conv))


def run(ops, inputs, program):
    """-> the registers as arrays, the results (f64: ok and value per float_value_at step)"""
    regs = [ops.upload(a) for a in inputs]
    results = []
    for op, *arg in program:
        if op in ("to_float", "depth_to_float", "from_float", "filter", "filter_separable", "filter_horizontal", "flip", "downsample",
                  "dilate", "copy"):
            regs.append(getattr(ops, op)(regs[arg[0]], *arg[1:]))
        elif op in ("linear_transform", "clip_intensity"):
            getattr(ops, op)(regs[arg[0]], *arg[1:])
        elif op == "pyramid":
            regs += ops.pyramid(regs[arg[0]], arg[1], arg[2])
        elif op == "filter_pyramid":
            regs += ops.filter_pyramid(regs[arg[0]:arg[0] + arg[1]], arg[2])
        elif op == "distance_multiplier":
            regs.append(ops.distance_multiplier(*arg))
        elif op == "float_value_at":
            ok, value = ops.float_value_at(regs[arg[0]], np.asarray(arg[1], np.float64))
            results += [np.asarray(ok, np.float64), np.asarray(value, np.float64)]
        elif op == "rgbd":
            c, d = ops.rgbd(regs[arg[0]], regs[arg[1]], *arg[2:])
            regs += [ops.empty() if c is None else c, ops.empty() if d is None else d]
        else:
            raise ValueError(op)
    out = [ops.download(r) for r in regs]
    for r in regs:
        ops.close(r)
    return out, np.concatenate([np.zeros(0)] + results)


def spec(name):
    if ("spec", name) not in _CACHE:
        _CACHE[("spec", name)] = run(SpecOps(), *case(name))
    return _CACHE[("spec", name)]


def bits(a):
    """what is compared: the bytes, every fp32 NaN as ONE pattern -- the sign and payload of a NaN an operation MAKES belong
    to the hardware, not to the reference (tests/cloud_cases.py: bits)"""
    a = np.ascontiguousarray(a)
    if a.dtype == F32:
        b = a.view(np.uint32).copy()
        b[np.isnan(a)] = 0x7FC00000
        return b
    if a.dtype == np.float64:
        a = a.copy()
        a[np.isnan(a)] = np.nan
        return a.view(np.uint64)
    return a


def infos(regs):
    return np.array([S.info(r) for r in regs], np.int64).reshape(-1, 4)


def digest(regs, results):
    h = hashlib.sha256()
    for r in regs:
        h.update(bits(r).tobytes())
    h.update(bits(results).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def same(got, want, label):
    """registers and results: format, shape and bits"""
    regs, res = got
    wregs, wres = want
    assert infos(regs).tolist() == infos(wregs).tolist(), (label, infos(regs).tolist(), infos(wregs).tolist())
    for k, (a, b) in enumerate(zip(regs, wregs)):
        assert a.dtype == b.dtype and a.shape == b.shape, (label, k, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, (label, "register", k, len(bad), bad[:5].tolist(), [a[tuple(i)] for i in bad[:5]], [b[tuple(i)] for i in bad[:5]])
    assert res.shape == wres.shape, (label, res.shape, wres.shape)
    bad = np.nonzero(bits(res) != bits(wres))[0]
    assert len(bad) == 0, (label, "results", bad[:5], res[bad[:5]], wres[bad[:5]])


# ---- what the reference harness of tests/golden/gen_image.py reads ------------------------------------------------------------
def encode(inputs, program):
    """little-endian: doubles for every number, raw bytes for pixels"""
    out = []
    d = lambda *v: out.append(struct.pack("<%dd" % len(v), *[float(x) for x in v]))
    vec = lambda v: (d(len(v)), d(*v) if len(v) else None)
    d(len(inputs))
    for a in inputs:
        d(*S.info(a))
        out.append(np.ascontiguousarray(a).tobytes())
    d(len(program))
    for op, *arg in program:
        d(OPS.index(op))
        if op in ("filter_separable",):
            d(arg[0]); vec(arg[1]); vec(arg[2])
        elif op == "filter_horizontal":
            d(arg[0]); vec(arg[1])
        elif op == "distance_multiplier":
            d(*arg[0]); d(arg[1], arg[2])
        elif op == "float_value_at":
            d(arg[0]); vec(np.asarray(arg[1], np.float64).reshape(-1))
        else:
            d(*arg)
    return b"".join(out)


def encode_image(a):
    """one image as encode() writes it: its format as four doubles, then the raw pixels"""
    return struct.pack("<4d", *[float(x) for x in S.info(a)]) + np.ascontiguousarray(a).tobytes()


def decode(raw):
    """what a harness of this format writes back (tests/golden/gen_image.py's, tests/cpp/image_driver.cpp's) -> registers, results"""
    at = [0]

    def take(n):
        out = raw[at[0]:at[0] + n]
        assert len(out) == n
        at[0] += n
        return out

    dtypes = {1: np.uint8, 2: np.uint16, 4: np.float32}
    regs = []
    for _ in range(int(np.frombuffer(take(4), "<i4")[0])):
        w, h, ch, b = np.frombuffer(take(16), "<i4").tolist()
        if ch == 0:
            assert (w, h, b) == (0, 0, 0)
            regs.append(S.EMPTY)
            continue
        a = np.frombuffer(take(w * h * ch * b), dtypes[b]).copy()
        regs.append(a.reshape((h, w) if ch == 1 else (h, w, ch)))
    results = np.frombuffer(take(8 * int(np.frombuffer(take(4), "<i4")[0])), "<f8").copy()
    assert at[0] == len(raw)
    return regs, results
