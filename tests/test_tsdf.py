"""TSDF integration on the GPU (visma_icp_tsdf_* and visma_icp_point_cloud_from_*; tsdf.hip).

The yardstick is the numpy specification tests/tsdf_spec.py; tests/golden/tsdf.npz (tests/golden/gen_tsdf.py) pins it to
the compiled reference: every volume (tsdf, weight, colour) bit for bit, through SHA-256 digests of the whole volume and
three probe planes in full (resolution 21: the whole volume in full); extracted points, colours and the voxel cloud bit for
bit; normals bit for bit too (the specification reaches that; tsdf_spec.NORMAL_TOL = 1e-11 per component is the bound that
would hold for any evaluation order); the clouds from a depth frame bit for bit with the identity extrinsic and within
1e-12 relative with another.

Cases U21, U32, U67: four 40 x 30 frames into a uniform volume whose columns are unaligned with a tail (21), aligned (32),
longer than a wave (67).  E: an all-zero depth frame.  P: point clouds from a depth and an RGB-D frame.  The larger shape
(640 x 480 into 128^3) is checked against the specification, which the CPU tests have pinned by then.

S: scalable volumes with units of 8 and 16, strides 4 and 1, one with sdf_trunc above the unit length; their rows are
compared after sorting (the reference's order is a hash map's) and, unsorted, against the specification's documented order."""
import ctypes as C
import os

import numpy as np
import pytest

import tsdf_scene as scene
import tsdf_spec as S
from oracle_engine import OracleEngine

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, STATE = 1, 5
RESOLUTIONS = (21, 32, 67)
COLOR_TYPES = (S.COLOR_NONE, S.COLOR_RGB8, S.COLOR_GRAY32)
N_FRAMES = 4


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "tsdf.npz"))
    return {k: g[k] for k in g.files}


def frames_of(golden):
    return [(golden["f%d_depth" % i], golden["f%d_rgb" % i], golden["f%d_gray" % i], golden["f%d_extrinsic" % i]) for i in range(N_FRAMES)]


def color_of(frame, color_type):
    return {S.COLOR_NONE: None, S.COLOR_RGB8: frame[1], S.COLOR_GRAY32: frame[2]}[color_type]


@pytest.fixture(scope="module")
def spec_volumes(golden):
    """the specification's volumes of U21 / U32 / U67 x colour type after the first and after the last frame: computed once,
    shared and left unchanged.  -> {(R, color_type): [stage 0, stage 1]}, a stage = (tsdf, weight, color)"""
    out = {}
    for R in RESOLUTIONS:
        for t in COLOR_TYPES:
            vol = S.new_volume(float(golden["length"]), R, float(golden["u%d_sdf_trunc" % R]), t, golden["origin"])
            stages = []
            for i, fr in enumerate(frames_of(golden)):
                S.integrate(vol, fr[0], color_of(fr, t), golden["intrinsic"], fr[3])
                if i in (0, N_FRAMES - 1):
                    stages.append((vol["tsdf"].copy(), vol["weight"].copy(), None if vol["color"] is None else vol["color"].copy()))
            out[(R, t)] = stages
    return out


def spec_final(golden, spec_volumes, R, t):
    vol = S.new_volume(float(golden["length"]), R, float(golden["u%d_sdf_trunc" % R]), t, golden["origin"])
    vol["tsdf"], vol["weight"], vol["color"] = spec_volumes[(R, t)][1]
    return vol


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def planes(R):
    return (R // 2, R // 3, (2 * R) // 3)


def probe(a, R, axis):
    a = a.reshape((R, R, R) + a.shape[1:])
    return np.take(a, planes(R)[axis], axis=axis)


def check_volume(golden, R, stage, t, tsdf, weight, color):
    """a volume against the fixture: the digests of the whole, the probe planes (or the whole, for 21) in full"""
    pre = "u%d_s%d_" % (R, stage)
    assert np.array_equal(S.digest(tsdf, np.float32), golden[pre + "tsdf_sha"]), (R, stage, "tsdf")
    assert np.array_equal(S.digest(weight, np.float32), golden[pre + "weight_sha"]), (R, stage, "weight")
    if pre + "tsdf_full" in golden:
        assert same_bits(tsdf, golden[pre + "tsdf_full"]) and np.array_equal(weight, golden[pre + "weight_full"].astype(np.float32))
    elif pre + "tsdf_p0" in golden:                                   # (the first stage of 21: the digests alone)
        for ax in range(3):
            assert same_bits(probe(tsdf, R, ax), golden[pre + "tsdf_p%d" % ax]), (R, stage, ax)
            assert np.array_equal(probe(weight, R, ax), golden[pre + "weight_p%d" % ax].astype(np.float32)), (R, stage, ax)
    if t == S.COLOR_NONE:
        assert color is None
        return
    assert color.shape == (R ** 3, 3)
    assert np.array_equal(S.digest(color, np.float32), golden[pre + "t%d_color_sha" % t]), (R, stage, "color")
    want = (lambda c: c) if t == S.COLOR_RGB8 else (lambda c: np.repeat(c[..., None], 3, axis=-1))
    if pre + "t%d_color_full" % t in golden:
        assert same_bits(color, want(golden[pre + "t%d_color_full" % t]))
    elif pre + "t%d_color_p0" % t in golden:
        for ax in range(3):
            assert same_bits(probe(color, R, ax), want(golden[pre + "t%d_color_p%d" % (t, ax)])), (R, stage, ax)


def e1_rows(golden, stride, pts):
    """the rows of a cloud built with frame 1's extrinsic that the fixture holds (stride 1: the count and every 8th row)"""
    want = golden["p_s%d_e1_points" % stride]
    if stride == 1:
        assert len(pts) == int(golden["p_s1_e1_n"])
        pts = pts[::8]
    assert pts.shape == want.shape
    return pts, want


S_CASES = ("s0", "s1", "s2")


def s_config(golden, name):
    R, stride, vl, trunc, t, nf = golden[name + "_config"]
    return int(R), int(stride), float(vl), float(trunc), int(t), int(nf)


def unit_digest(tsdf, weight, color):
    return S.digest(np.concatenate([tsdf, weight] + ([] if color is None else [color.ravel()])), np.float32)


def check_units(golden, name, keys, unit_of):
    """the final units of a scalable case against the fixture: the set, every unit's volume through its digest (the first 8
    bytes per unit, all 32 of all units through one digest), a few units in full.  unit_of(key) -> tsdf, weight, color"""
    want = golden["%s_units_f%d" % (name, s_config(golden, name)[5] - 1)]
    assert np.array_equal(np.asarray(keys, np.int32).reshape(-1, 3), want)            # (sorted: the library's order)
    sha = np.stack([unit_digest(*unit_of(tuple(k))) for k in want.tolist()])
    assert np.array_equal(sha[:, :8], golden[name + "_unit_sha8"]), np.flatnonzero((sha[:, :8] != golden[name + "_unit_sha8"]).any(1))[:5]
    assert np.array_equal(S.digest(sha, np.uint8), golden[name + "_units_sha"])
    for i, k in enumerate(golden[name + "_probe_units"].tolist()):
        tsdf, weight, color = unit_of(tuple(k))
        assert same_bits(tsdf, golden[name + "_probe_tsdf"][i]) and np.array_equal(weight, golden[name + "_probe_weight"][i].astype(np.float32))
        if color is not None:
            assert same_bits(color, golden[name + "_probe_color"][i])


def check_scalable_extraction(golden, name, pc, vx):
    """the two extractions against the fixture after the rows are sorted the way the fixture's are (by point)"""
    t = s_config(golden, name)[4]
    pts, nrm, col = S.sort_rows(*pc)
    n = int(golden[name + "_pc_n"])
    assert pts.shape == (n, 3) and nrm.shape == (n, 3)
    assert np.array_equal(S.digest(pts, np.float64), golden[name + "_pc_points_sha"])
    at = golden[name + "_pc_at"]
    assert same_bits(pts[at], golden[name + "_pc_points"])
    dn = float(np.max(np.abs(nrm[at] - golden[name + "_pc_normals"]), initial=0.0))               # (initial: a cloud may be empty)
    assert dn <= S.NORMAL_TOL, dn
    assert same_bits(nrm[at], golden[name + "_pc_normals"]), dn        # (the specification reaches bit for bit)
    if t == S.COLOR_NONE:
        assert col is None
    else:
        assert np.array_equal(S.digest(col, np.float64), golden[name + "_pc_colors_sha"]) and same_bits(col[at], golden[name + "_pc_colors"])
    vp, vc = S.sort_rows(*vx)
    assert len(vp) == int(golden[name + "_vx_n"])
    assert np.array_equal(S.digest(vp, np.float64), golden[name + "_vx_points_sha"])
    assert np.array_equal(S.digest(vc, np.float64), golden[name + "_vx_colors_sha"])
    return dn


def check_extraction(golden, R, t, pc, vx):
    """ExtractPointCloud and ExtractVoxelPointCloud of a final volume against the fixture -> the normals' largest deviation"""
    pts, nrm, col = pc
    n = int(golden["u%d_pc_n" % R])
    assert pts.shape == (n, 3) and nrm.shape == (n, 3)
    assert np.array_equal(S.digest(pts, np.float64), golden["u%d_pc_points_sha" % R])        # count, points and order
    at = golden["u%d_pc_at" % R]
    assert same_bits(pts[at], golden["u%d_pc_points" % R])
    dn = float(np.max(np.abs(nrm[at] - golden["u%d_pc_normals" % R]), initial=0.0))                 # (initial: a cloud may be empty)
    assert dn <= S.NORMAL_TOL, dn
    assert same_bits(nrm[at], golden["u%d_pc_normals" % R]), dn               # (the specification reaches bit for bit: so must the library)
    if t == S.COLOR_NONE:
        assert col is None
    else:
        assert col.shape == (n, 3)
        assert np.array_equal(S.digest(col, np.float64), golden["u%d_t%d_pc_colors_sha" % (R, t)])
        assert same_bits(col[at], golden["u%d_t%d_pc_colors" % (R, t)])
    vp, vc = vx
    assert len(vp) == int(golden["u%d_vx_n" % R]) and len(vc) == len(vp)
    assert np.array_equal(S.digest(vp, np.float64), golden["u%d_vx_points_sha" % R])
    assert np.array_equal(S.digest(vc, np.float64), golden["u%d_vx_colors_sha" % R])
    return dn, bool(same_bits(nrm[at], golden["u%d_pc_normals" % R]))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_tsdf_create_uniform", "visma_icp_tsdf_destroy", "visma_icp_tsdf_reset", "visma_icp_tsdf_integrate",
               "visma_icp_tsdf_extract_point_cloud", "visma_icp_tsdf_get_point_cloud", "visma_icp_tsdf_extract_voxel_point_cloud",
               "visma_icp_tsdf_get_voxel_point_cloud", "visma_icp_tsdf_get_volume", "visma_icp_point_cloud_from_depth",
               "visma_icp_point_cloud_from_rgbd"]
NEW_SYMBOLS += ["visma_icp_tsdf_create_scalable", "visma_icp_tsdf_get_units"]
NEW_METHODS = ["tsdf_uniform", "tsdf_scalable", "point_cloud_from_depth", "point_cloud_from_rgbd"]
VOLUME_METHODS = ["integrate", "extract_point_cloud", "extract_voxel_point_cloud", "reset", "volume", "units", "close"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in NEW_METHODS:
        assert callable(getattr(lib.Context, name, None)), name
    for name in VOLUME_METHODS:
        assert callable(getattr(lib.TsdfVolume, name, None)), name
    assert (lib.TSDF_COLOR_NONE, lib.TSDF_COLOR_RGB8, lib.TSDF_COLOR_GRAY32) == COLOR_TYPES


@pytest.fixture()
def hctx(lib, oracle):
    eng = OracleEngine(oracle)
    ctx = eng.context()
    ctx.engine = eng
    yield ctx
    ctx.close()


def test_argument_checks(lib, hctx):
    """every argument error comes before anything reaches a device (a context on the oracle engine has none: a call that
    passes its checks ends at that engine's "not supported", VISMA_ICP_ERR_STATE)"""
    L, h = hctx.L, hctx._h
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    vol = C.c_void_p()
    org = np.zeros(3); porg = org.ctypes.data_as(dp)

    def create(length=1.0, R=8, trunc=0.1, t=0, origin=porg, out=C.byref(vol), ctx=h):
        return L.visma_icp_tsdf_create_uniform(ctx, length, R, trunc, t, origin, out)

    assert create(ctx=None) == INVALID
    assert create(out=None) == INVALID
    assert create(R=0) == INVALID and create(R=-3) == INVALID
    assert create(length=0.0) == INVALID and create(length=-1.0) == INVALID and create(length=float("nan")) == INVALID
    assert create(trunc=0.0) == INVALID and create(trunc=float("inf")) == INVALID
    assert create(t=3) == INVALID and create(t=-1) == INVALID
    bad = np.array([0.0, np.nan, 0.0])
    assert create(origin=bad.ctypes.data_as(dp)) == INVALID
    assert create(R=1291) == INVALID and create(R=1 << 20) == INVALID          # a volume too large for memory
    assert create() == STATE and not vol.value                                  # every check passed; this engine has no volumes
    assert b"not supported" in L.visma_icp_last_error(h)
    assert create(origin=None) == STATE

    def scalable(vl=0.05, trunc=0.1, t=0, R=16, stride=4, units=0, out=C.byref(vol), ctx=h):
        return L.visma_icp_tsdf_create_scalable(ctx, vl, trunc, t, R, stride, units, out)

    assert scalable(ctx=None) == INVALID and scalable(out=None) == INVALID
    assert scalable(R=0) == INVALID and scalable(R=257) == INVALID
    assert scalable(vl=0.0) == INVALID and scalable(vl=float("nan")) == INVALID and scalable(trunc=-1.0) == INVALID
    assert scalable(t=5) == INVALID
    assert scalable(stride=0) == INVALID and scalable(stride=-1) == INVALID
    assert scalable(units=-1) == INVALID and scalable(units=(1 << 20) + 1) == INVALID
    assert scalable() == STATE and not vol.value and scalable(units=3, R=8, stride=1, t=2) == STATE

    # a volume the context does not know
    fake = C.c_void_p(0x1000)
    n = C.c_int64(7)
    w, hh = 8, 6
    img = np.ones((hh, w), np.float32); pi = img.ctypes.data_as(fp)
    k = np.array([7.0, 7.0, 3.5, 2.5]); pk = k.ctypes.data_as(dp)
    E = np.eye(4).ravel().copy(); pE = E.ctypes.data_as(dp)
    for v in (None, fake):
        assert L.visma_icp_tsdf_destroy(h, v) == INVALID
        assert L.visma_icp_tsdf_reset(h, v) == INVALID
        assert L.visma_icp_tsdf_integrate(h, v, w, hh, pi, None, pk, w, hh, pE) == INVALID
        assert L.visma_icp_tsdf_extract_point_cloud(h, v, C.byref(n)) == INVALID
        assert L.visma_icp_tsdf_get_point_cloud(h, v, None, None, None, 0) == INVALID
        assert L.visma_icp_tsdf_extract_voxel_point_cloud(h, v, C.byref(n)) == INVALID
        assert L.visma_icp_tsdf_get_voxel_point_cloud(h, v, None, None, 0) == INVALID
        assert L.visma_icp_tsdf_get_volume(h, v, None, None, None, None) == INVALID
        assert L.visma_icp_tsdf_get_units(h, v, None, 0, C.byref(n)) == INVALID
    assert L.visma_icp_tsdf_reset(None, fake) == INVALID

    # the point clouds from a frame
    pts = np.zeros((w * hh, 3)); pp = pts.ctypes.data_as(dp)
    rgb = np.zeros((hh, w, 3), np.uint8); prgb = rgb.ctypes.data_as(C.c_void_p)

    def depth(w=w, h_=hh, d=pi, k=pk, E=pE, stride=1, p=pp, cap=w * hh, out=C.byref(n), ctx=h):
        return L.visma_icp_point_cloud_from_depth(ctx, w, h_, d, k, E, stride, p, cap, out)

    def rgbd(w=w, h_=hh, d=pi, c=prgb, t=1, k=pk, E=pE, p=pp, cap=w * hh, out=C.byref(n), ctx=h):
        return L.visma_icp_point_cloud_from_rgbd(ctx, w, h_, d, c, t, k, E, p, pp, cap, out)

    assert depth(ctx=None) == INVALID and rgbd(ctx=None) == INVALID
    assert depth(out=None) == INVALID
    assert depth(d=None) == INVALID and depth(k=None) == INVALID
    assert depth(w=0) == INVALID and depth(h_=0) == INVALID
    assert depth(stride=0) == INVALID and depth(stride=-2) == INVALID
    assert depth(cap=w * hh - 1) == INVALID and depth(stride=4, cap=3) == INVALID     # 2 x 2 strided pixels
    assert depth(stride=2**31 - 1, cap=0) == INVALID and depth(stride=2**31 - 1, cap=1) == STATE   # (the ceilings are formed in 64 bits)
    zero_f = np.array([0.0, 7.0, 3.5, 2.5]); nan_f = np.array([7.0, np.nan, 3.5, 2.5])
    assert depth(k=zero_f.ctypes.data_as(dp)) == INVALID and depth(k=nan_f.ctypes.data_as(dp)) == INVALID
    assert rgbd(c=None) == INVALID                                              # a colour pointer missing
    assert rgbd(t=0) == INVALID and rgbd(t=3) == INVALID
    assert depth() == STATE and depth(E=None) == STATE and depth(p=None, cap=0) == STATE and depth(stride=4, cap=4) == STATE
    assert rgbd() == STATE and rgbd(t=2) == STATE


def test_specification_volumes_equal_the_reference_bit_for_bit(golden, spec_volumes):
    for R in RESOLUTIONS:
        for t in COLOR_TYPES:
            for stage in (0, 1):
                check_volume(golden, R, stage, t, *spec_volumes[(R, t)][stage])
        w = np.unique(spec_volumes[(R, 0)][1][1])
        assert w[0] == 0 and w[-1] == N_FRAMES


def test_specification_extractions_equal_the_reference(golden, spec_volumes):
    for R in RESOLUTIONS:
        for t in COLOR_TYPES:
            vol = spec_final(golden, spec_volumes, R, t)
            dn, exact = check_extraction(golden, R, t, S.extract_point_cloud(vol), S.extract_voxel_point_cloud(vol))
            print("U%d colour type %d: normals within %.3g of the reference%s" % (R, t, dn, " (bit for bit)" if exact else ""))


def test_specification_point_clouds_equal_the_reference(golden):
    fr = frames_of(golden)[0]
    k, E1 = golden["intrinsic"], golden["p_extrinsic"]
    for stride in (1, 4):
        pts, _ = S.point_cloud_from_depth(fr[0], k, None, stride)
        assert same_bits(pts, golden["p_s%d_id_points" % stride])
        pts, _ = S.point_cloud_from_depth(fr[0], k, E1, stride)
        pts, want = e1_rows(golden, stride, pts)
        rel = float(np.max(np.linalg.norm(pts - want, axis=1) / np.linalg.norm(want, axis=1)))
        assert rel <= S.POINT_TOL, rel
    pts, col = S.point_cloud_from_depth(fr[0], k, None, 1, color=fr[1])
    assert same_bits(pts, golden["p_s1_id_points"]) and same_bits(col, golden["p_rgb_id_colors"])
    pts, col = S.point_cloud_from_depth(fr[0], k, None, 1, color=fr[2])
    assert same_bits(pts, golden["p_s1_id_points"]) and same_bits(col, golden["p_gray_id_colors"].astype(np.float64))


@pytest.fixture(scope="module")
def spec_scalable(golden):
    """the specification's scalable volumes of S with the unit sets after every frame: computed once, shared, unchanged"""
    out = {}
    frames = frames_of(golden)
    for name in S_CASES:
        R, stride, vl, trunc, t, nf = s_config(golden, name)
        sv = S.new_scalable(vl, trunc, t, R, stride)
        sets = []
        for fr in frames[:nf]:
            S.scalable_integrate(sv, fr[0], color_of(fr, t), golden["intrinsic"], fr[3])
            sets.append(sorted(sv["units"]))
        out[name] = (sv, sets)
    return out


@pytest.mark.parametrize("name", S_CASES)
def test_specification_scalable_equals_the_reference(golden, spec_scalable, name):
    sv, sets = spec_scalable[name]
    for i, keys in enumerate(sets):
        assert np.array_equal(np.array(keys, np.int32), golden["%s_units_f%d" % (name, i)]), (name, i)
    check_units(golden, name, sets[-1], lambda k: (sv["units"][k]["tsdf"], sv["units"][k]["weight"], sv["units"][k]["color"]))
    dn = check_scalable_extraction(golden, name, S.scalable_extract_point_cloud(sv), S.scalable_extract_voxel_point_cloud(sv))
    print("%s: %d units, normals within %.3g of the reference" % (name, len(sets[-1]), dn))


def test_specification_empty_frame(golden):
    """E: an all-zero depth frame leaves a fresh and a filled volume as they were; an empty volume extracts to nothing"""
    fr = frames_of(golden)[0]
    zero = np.zeros_like(fr[0])
    vol = S.new_volume(float(golden["length"]), 21, float(golden["u21_sdf_trunc"]), S.COLOR_RGB8, golden["origin"])
    S.integrate(vol, zero, fr[1], golden["intrinsic"], fr[3])
    assert not vol["tsdf"].any() and not vol["weight"].any() and not vol["color"].any()
    assert len(S.extract_point_cloud(vol)[0]) == int(golden["e_fresh_pc_n"]) == 0
    assert len(S.extract_voxel_point_cloud(vol)[0]) == int(golden["e_fresh_vx_n"]) == 0
    S.integrate(vol, fr[0], fr[1], golden["intrinsic"], fr[3])
    before = (vol["tsdf"].copy(), vol["weight"].copy(), vol["color"].copy())
    S.integrate(vol, zero, fr[1], golden["intrinsic"], fr[3])
    assert int(golden["e_filled_unchanged"]) == 1
    assert same_bits(vol["tsdf"], before[0]) and same_bits(vol["weight"], before[1]) and same_bits(vol["color"], before[2])


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def lib_volume(ctx, golden, R, t):
    return ctx.tsdf_uniform(float(golden["length"]), R, float(golden["u%d_sdf_trunc" % R]), t, golden["origin"])


@pytest.mark.gpu
@pytest.mark.parametrize("t", COLOR_TYPES)
@pytest.mark.parametrize("R", RESOLUTIONS)
def test_volumes_and_extractions_equal_the_reference(lib, ctx, golden, R, t):
    """tests 1 and 2: the volume after the first and after the last frame bit for bit, weights included; count, points,
    colours and order of ExtractPointCloud bit for bit, normals within 1e-11; the voxel cloud equal"""
    vol = lib_volume(ctx, golden, R, t)
    for i, fr in enumerate(frames_of(golden)):
        vol.integrate(fr[0], color_of(fr, t), golden["intrinsic"], fr[3])
        if i in (0, N_FRAMES - 1):
            check_volume(golden, R, 0 if i == 0 else 1, t, *vol.volume())
    dn, exact = check_extraction(golden, R, t, vol.extract_point_cloud(), vol.extract_voxel_point_cloud())
    print("U%d colour type %d: normals within %.3g of the reference%s" % (R, t, dn, " (bit for bit)" if exact else ""))
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", S_CASES)
def test_scalable_volumes_equal_the_reference(lib, ctx, golden, spec_scalable, name):
    """test 3: the unit set after each frame; every unit's volume bit for bit; the extractions equal the fixture's once sorted
    the same way; the library's own order is the documented one (units lexicographic, the reference's order within a unit:
    the specification's order); the pool starts below the first frame's unit count and grows twice, the contents survive"""
    R, stride, vl, trunc, t, nf = s_config(golden, name)
    first = len(golden[name + "_units_f0"])
    initial = max(2, first // 4)
    assert 2 * initial < first < len(golden["%s_units_f%d" % (name, nf - 1)])      # frame 0 grows the pool, a later frame again
    vol = ctx.tsdf_scalable(vl, trunc, t, R, stride, initial_units=initial)
    assert len(vol.units()) == 0
    for i, fr in enumerate(frames_of(golden)[:nf]):
        vol.integrate(fr[0], color_of(fr, t), golden["intrinsic"], fr[3])
        assert np.array_equal(vol.units(), golden["%s_units_f%d" % (name, i)]), (name, i)
    check_units(golden, name, vol.units(), lambda k: vol.volume(k))
    pc, vx = vol.extract_point_cloud(), vol.extract_voxel_point_cloud()
    dn = check_scalable_extraction(golden, name, pc, vx)
    sv = spec_scalable[name][0]
    for got, want in zip(pc + vx, S.scalable_extract_point_cloud(sv) + S.scalable_extract_voxel_point_cloud(sv)):
        assert (got is None and want is None) or same_bits(got, want)                 # the documented order, row for row
    print("%s: %d units from a pool of %d, normals within %.3g of the reference" % (name, len(vol.units()), initial, dn))
    # E on a scalable volume: no unit is opened; Reset() forgets the units, and the same frames give the same volume again
    fr = frames_of(golden)[0]
    vol.integrate(np.zeros_like(fr[0]), color_of(fr, t), golden["intrinsic"], fr[3])
    assert np.array_equal(vol.units(), golden["%s_units_f%d" % (name, nf - 1)])
    vol.reset()
    assert len(vol.units()) == 0 and len(vol.extract_point_cloud()[0]) == 0 and len(vol.extract_voxel_point_cloud()[0]) == 0
    vol.integrate(np.zeros_like(fr[0]), color_of(fr, t), golden["intrinsic"], fr[3])
    assert len(vol.units()) == 0
    for fr in frames_of(golden)[:nf]:
        vol.integrate(fr[0], color_of(fr, t), golden["intrinsic"], fr[3])
    check_units(golden, name, vol.units(), lambda k: vol.volume(k))
    with pytest.raises(lib.IcpError) as e:
        vol.volume((10000, 0, 0))
    assert e.value.code == INVALID
    vol.close()


@pytest.mark.gpu
def test_point_clouds_from_frames_equal_the_reference(lib, ctx, golden):
    """P as recorded"""
    fr = frames_of(golden)[0]
    k, E1 = golden["intrinsic"], golden["p_extrinsic"]
    for stride in (1, 4):
        assert same_bits(ctx.point_cloud_from_depth(fr[0], k, None, stride), golden["p_s%d_id_points" % stride])
        pts, want = e1_rows(golden, stride, ctx.point_cloud_from_depth(fr[0], k, E1, stride))
        rel = float(np.max(np.linalg.norm(pts - want, axis=1) / np.linalg.norm(want, axis=1)))
        print("stride %d, frame 1's extrinsic: within %.3g relative of the reference" % (stride, rel))
        assert rel <= S.POINT_TOL, rel
    pts, col = ctx.point_cloud_from_rgbd(fr[0], fr[1], k)
    assert same_bits(pts, golden["p_s1_id_points"]) and same_bits(col, golden["p_rgb_id_colors"])
    pts, col = ctx.point_cloud_from_rgbd(fr[0], fr[2], k)
    assert same_bits(pts, golden["p_s1_id_points"]) and same_bits(col, golden["p_gray_id_colors"].astype(np.float64))
    assert len(ctx.point_cloud_from_depth(np.zeros_like(fr[0]), k)) == 0


@pytest.mark.gpu
def test_empty_frame_on_a_fresh_and_on_a_filled_volume(lib, ctx, golden):
    """E as recorded"""
    fr = frames_of(golden)[0]
    zero = np.zeros_like(fr[0])
    vol = lib_volume(ctx, golden, 21, S.COLOR_RGB8)
    vol.integrate(zero, fr[1], golden["intrinsic"], fr[3])
    tsdf, weight, color = vol.volume()
    assert not tsdf.any() and not weight.any() and not color.any()
    pts, nrm, col = vol.extract_point_cloud()
    assert len(pts) == int(golden["e_fresh_pc_n"]) == 0 and len(nrm) == 0 and len(col) == 0
    assert len(vol.extract_voxel_point_cloud()[0]) == int(golden["e_fresh_vx_n"]) == 0
    for f in frames_of(golden):
        vol.integrate(f[0], f[1], golden["intrinsic"], f[3])
    before = vol.volume()
    vol.integrate(zero, fr[1], golden["intrinsic"], fr[3])
    after = vol.volume()
    assert all(same_bits(a, b) for a, b in zip(before, after))
    check_volume(golden, 21, 1, S.COLOR_RGB8, *after)
    vol.close()


@pytest.mark.gpu
def test_repeats_reset_two_volumes_and_icp_around(lib, ctx, golden):
    """test 5: the same frames into two volumes give identical bytes; reset gives a volume equal to a new one; two volumes
    on one context do not disturb each other; the ICP runs on the same context before and after equal, to the bit, the same
    two runs on a context without volumes"""
    from visma_amd import synth
    src, tgt, _, _ = synth.make_pair(2000, 6000)
    # the yardstick: the same two runs on a context that never sees a volume (a second run on a context starts from the
    # first one's search state and need not equal it to the bit; it must equal the OTHER context's second run)
    plain = lib.Context(0)
    plain.set_clouds_f64(src, tgt)
    want = [plain.run(None, 0.075, 10, 0.0, 0.0), plain.run(None, 0.075, 10, 0.0, 0.0)]
    plain.close()
    ctx.set_clouds_f64(src, tgt)
    icp0 = ctx.run(None, 0.075, 10, 0.0, 0.0)
    frames = frames_of(golden)
    k = golden["intrinsic"]
    a = lib_volume(ctx, golden, 32, S.COLOR_RGB8)
    b = lib_volume(ctx, golden, 21, S.COLOR_GRAY32)
    c = lib_volume(ctx, golden, 32, S.COLOR_RGB8)
    for fr in frames:                                    # interleaved: a and b take turns
        a.integrate(fr[0], fr[1], k, fr[3])
        b.integrate(fr[0], fr[2], k, fr[3])
    pc_a = a.extract_point_cloud()
    for fr in frames:
        c.integrate(fr[0], fr[1], k, fr[3])
    va, vb, vc = a.volume(), b.volume(), c.volume()
    assert all(same_bits(x, y) for x, y in zip(va, vc))
    check_volume(golden, 32, 1, S.COLOR_RGB8, *va)
    check_volume(golden, 21, 1, S.COLOR_GRAY32, *vb)
    pc_c = c.extract_point_cloud()
    assert all(same_bits(x, y) for x, y in zip(pc_a, pc_c))
    a.reset()
    fresh = lib_volume(ctx, golden, 32, S.COLOR_RGB8)
    assert all(same_bits(x, y) for x, y in zip(a.volume(), fresh.volume())) and not a.volume()[1].any()
    assert len(a.extract_point_cloud()[0]) == 0
    assert all(same_bits(x, y) for x, y in zip(vc, c.volume()))                # c is as it was
    for fr in frames:
        a.integrate(fr[0], fr[1], k, fr[3])
    assert all(same_bits(x, y) for x, y in zip(a.volume(), vc))
    icp1 = ctx.run(None, 0.075, 10, 0.0, 0.0)
    for got, exp in zip((icp0, icp1), want):
        assert np.array_equal(got.transformation_, exp.transformation_) and got.num_correspondences == exp.num_correspondences
        assert got.fitness_ == exp.fitness_ and got.inlier_rmse_ == exp.inlier_rmse_ and got.iterations == exp.iterations
    for v in (a, b, c, fresh):
        v.close()


@pytest.mark.gpu
def test_get_before_extract_and_a_frame_that_does_not_fit(lib, ctx, golden):
    """the call order and the frame checks on a real volume: a get before its extract is STATE, with another n INVALID; a
    frame of another size than the intrinsic's and a missing colour image are INVALID and leave the volume as it was"""
    L, h = ctx.L, ctx._h
    vol = lib_volume(ctx, golden, 21, S.COLOR_RGB8)
    fr = frames_of(golden)[0]
    assert L.visma_icp_tsdf_get_point_cloud(h, vol._v, None, None, None, 0) == STATE
    vol.integrate(fr[0], fr[1], golden["intrinsic"], fr[3])
    before = vol.volume()
    pts, _, _ = vol.extract_point_cloud()
    assert L.visma_icp_tsdf_get_point_cloud(h, vol._v, None, None, None, len(pts) + 1) == INVALID
    with pytest.raises(lib.IcpError) as e:
        vol.integrate(fr[0], fr[1], golden["intrinsic"], fr[3], intrinsic_size=(fr[0].shape[1] + 1, fr[0].shape[0]))
    assert e.value.code == INVALID
    with pytest.raises(lib.IcpError) as e:
        vol.integrate(fr[0], None, golden["intrinsic"], fr[3])
    assert e.value.code == INVALID
    assert all(same_bits(x, y) for x, y in zip(before, vol.volume()))
    vol.close()


@pytest.mark.gpu
def test_larger_shape_equals_the_specification(lib, ctx):
    """test 6: two 640 x 480 RGB8 frames into a uniform 128^3 volume -- the kernels' grid-stride loops (2 M voxels in
    8192 tiles over at most 2048 workgroups) and the scan over more tiles than one workgroup takes at once"""
    frames, k = scene.frames(640, 480, 2)
    R, length, trunc, origin = 128, 1.6, 0.05, (-0.8, -0.75, -0.85)
    spec = S.new_volume(length, R, trunc, S.COLOR_RGB8, origin)
    vol = ctx.tsdf_uniform(length, R, trunc, S.COLOR_RGB8, origin)
    for fr in frames:
        S.integrate(spec, fr[0], fr[1], k, fr[3])
        vol.integrate(fr[0], fr[1], k, fr[3])
    tsdf, weight, color = vol.volume()
    assert same_bits(tsdf, spec["tsdf"]) and same_bits(weight, spec["weight"]) and same_bits(color, spec["color"])
    assert weight.max() == 2.0
    sp, sn, sc = S.extract_point_cloud(spec)
    pts, nrm, col = vol.extract_point_cloud()
    assert len(sp) > 20000
    assert same_bits(pts, sp) and same_bits(col, sc)
    dn = float(np.max(np.abs(nrm - sn)))
    print("128^3: %d points, normals within %.3g of the specification" % (len(pts), dn))
    assert dn <= S.NORMAL_TOL and same_bits(nrm, sn), dn
    vp, vc = S.extract_voxel_point_cloud(spec)
    gp, gc = vol.extract_voxel_point_cloud()
    assert same_bits(gp, vp) and same_bits(gc, vc)
    vol.close()
