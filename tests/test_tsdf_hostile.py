"""TSDF integration and the clouds from a frame on inputs chosen to break them (tsdf.hip), where tests/test_tsdf.py has one
well-behaved scene.  The yardsticks are those of test_tsdf.py: the numpy specification tests/tsdf_spec.py, pinned to the
compiled reference by tests/golden/rgbd_hostile.npz (tests/golden/gen_rgbd_hostile.py); every comparison is bit for bit
(normals too: the specification reaches that), the clouds under an extrinsic within tsdf_spec.POINT_TOL.  No bound is new.

  d      depth values: NaN, +inf, -inf, -1, 1e-40 (a denormal), 1e30 and 0 among ordinary depths, fx != fy and a principal point
         off the centre, into a uniform 21^3 volume of each colour type, and through point_cloud_from_depth / _from_rgbd
         (finite rows bit for bit, the others by class -- NaN, +inf, -inf -- per component)
  c<R>   column lengths 1 .. 7 and 65: every R % 4, columns shorter than a 16-byte vector, one voxel past a wave
  e_*    images of 1 x 1, 7 x 1, 1 x 7; u_f and v_f on either side of 0.0001 and of size - 0.0001 in exact numbers; voxels at
         pz == 0 and pz < 0
  a      64 integrations of two alternating frames: weights reach 64, the fp32 chain is the reference's
  h<i>   scalable volumes on the hostile frames (the rule of include/visma_icp.h: a pixel whose point is not finite or whose
         unit index lies beyond +-2^30 touches no unit): strides 4, 32 (one pixel) and 5, units of 8, 1 and 5 voxels;
         a frame of nothing but such depths
  The host half of that rule (visma_amd/csrc/tsdf_units.h) runs under ASan and UBSan in tests/cpp/tsdf_units_driver.cpp."""
import os
import subprocess
import sys

import numpy as np
import pytest

import packed_npz
import tsdf_scene as scene
import tsdf_spec as S
from test_tsdf import COLOR_TYPES, check_extraction, check_scalable_extraction, check_units, check_volume, color_of, s_config, same_bits

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_tsdf_units  # noqa: E402

COLUMN_CASES = ["c%d" % R for R in (1, 2, 3, 4, 5, 6, 7, 65)]
EDGE_CASES = ["e_" + n for n in scene.EDGE_CASES]
UNIFORM_CASES = ["d"] + COLUMN_CASES + EDGE_CASES + ["a"]
H_CASES = ["h0", "h1", "h2", "h3", "h4"]
P_CASES = (("s1_id", 1, False), ("s4_id", 4, False), ("s1_e", 1, True), ("s4_e", 4, True))


@pytest.fixture(scope="module")
def golden():
    return packed_npz.load(os.path.join(HERE, "golden", "rgbd_hostile.npz"))


def sub(golden, pre):
    """a case's part of the fixture under the key names of tsdf.npz"""
    return {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}


def uniform_case(golden, name):
    """-> the case's fixture, R, frames [(depth, rgb, gray, extrinsic)], intrinsic, length, sdf_trunc, origin"""
    g = sub(golden, name + "_")
    length, origin = float(golden["length"]), golden["origin"]
    if name == "d":
        frames, k = scene.hostile_frames()
        frames, R = frames[:1], 21
    elif name == "a":
        four, k = scene.asymmetric_frames(scene.HOSTILE_W, scene.HOSTILE_H)
        frames, R = [four[0], four[3]] * 32, 8
    elif name.startswith("c"):
        frames, k = scene.asymmetric_frames(scene.HOSTILE_W, scene.HOSTILE_H)
        R = int(name[1:])
    else:
        e = scene.edge_case(name[2:])
        frames, k, R, length, origin = [(e["depth"], e["rgb"], e["gray"], e["extrinsic"])], e["intrinsic"], e["R"], e["length"], e["origin"]
    return g, R, frames, k, length, float(g["u%d_sdf_trunc" % R]), origin


class Memo:
    """the specification's results, computed once per case, shared between the CPU and the GPU tests and left unchanged"""

    def __init__(self, golden):
        self.golden, self.have = golden, {}

    def uniform(self, name, t):
        """-> [stage 0, stage 1 (more than one frame)] (tsdf, weight, color), the surface cloud, the voxel cloud"""
        if (name, t) not in self.have:
            g, R, frames, k, length, trunc, origin = uniform_case(self.golden, name)
            vol = S.new_volume(length, R, trunc, t, origin)
            stages = []
            for i, fr in enumerate(frames):
                S.integrate(vol, fr[0], color_of(fr, t), k, fr[3])
                if i in (0, len(frames) - 1) and len(stages) < (1 if len(frames) == 1 else 2):
                    stages.append((vol["tsdf"].copy(), vol["weight"].copy(), None if vol["color"] is None else vol["color"].copy()))
            self.have[(name, t)] = (stages, S.extract_point_cloud(vol), S.extract_voxel_point_cloud(vol))
        return self.have[(name, t)]

    def scalable(self, name):
        """-> the specification's volume, its unit set after each frame"""
        if name not in self.have:
            R, stride, vl, trunc, t, nf = s_config(self.golden, name)
            frames, k = scene.hostile_frames()
            sv = S.new_scalable(vl, trunc, t, R, stride)
            sets = []
            for fr in frames[:nf]:
                S.scalable_integrate(sv, fr[0], color_of(fr, t), k, fr[3])
                sets.append(sorted(sv["units"]))
            self.have[name] = (sv, sets, S.scalable_extract_point_cloud(sv), S.scalable_extract_voxel_point_cloud(sv))
        return self.have[name]


@pytest.fixture(scope="module")
def spec(golden):
    return Memo(golden)


def point_class(p):
    """per component: 0 finite, 1 NaN, 2 +inf, 3 -inf"""
    return np.isnan(p) * 1 + np.isposinf(p) * 2 + np.isneginf(p) * 3


def check_frame_cloud(pts, want, exact):
    """a cloud from the hostile frame against the reference's: the same rows, finite rows bit for bit (or within POINT_TOL
    relative under an extrinsic), the others by class per component -> the largest relative deviation of a finite row"""
    assert pts.shape == want.shape and np.array_equal(point_class(pts), point_class(want))
    fin = np.isfinite(want).all(1)
    assert 0 < np.count_nonzero(~fin) < len(want)
    if exact:
        assert same_bits(pts[fin], want[fin])
        return 0.0
    rel = float(np.max(np.linalg.norm(pts[fin] - want[fin], axis=1) / np.linalg.norm(want[fin], axis=1)))
    assert rel <= S.POINT_TOL, rel
    return rel


def check_uniform(g, R, t, stages, pc, vx):
    for s, st in enumerate(stages):
        check_volume(g, R, s, t, *st)
    return check_extraction(g, R, t, pc, vx)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_box_expansion_under_the_sanitizers():
    """tests/cpp/tsdf_units_driver.cpp: expand_touched_boxes on INT_MAX / INT_MIN bounds, inverted boxes, the "no box" mark
    and ordinary boxes, compiled with -fsanitize=address,undefined: it returns, with the expected keys"""
    exe = build_tsdf_units.build()[0]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "all passed" in p.stdout and "FAILED" not in p.stdout and "runtime error" not in p.stderr, (p.stdout, p.stderr)
    assert p.stdout.count(": ok") == 12


def test_the_rule_in_the_specification():
    """touched_units: a pixel whose point is not finite or whose index lies beyond +-2^30 touches no unit; the others do"""
    k = np.array([8.0, 8.0, 1.5, 0.5])
    sv = S.new_scalable(0.25, 0.5, S.COLOR_NONE, 4, 1)                  # units of 1.0

    def units(row):
        tr = {}
        return S.touched_units(sv, np.array([row], np.float32), k, np.eye(4), trace=tr), tr.get("dropped_pixels", 0)

    plain, dropped = units([1.0, 1.0, 1.0, 1.0])
    assert dropped == 0 and (0, 0, 0) in plain and (0, 0, 1) in plain
    for bad in (np.inf, 1e30, 3e9 * 1.0):                               # +inf; beyond an int; beyond 2^30 but inside an int: z = 3e9 > 2^31
        got, dropped = units([1.0, bad, 1.0, bad])
        assert got == plain and dropped == 2, bad
    got, dropped = units([1.0, 1.2e9, 1.0, 1.0])                        # floor(1.2e9) is inside an int and beyond 2^30: dropped too
    assert got == plain and dropped == 1
    got, dropped = units([np.nan, -np.inf, -1.0, 0.0])                  # no depth: not even a point
    assert got == [] and dropped == 0
    assert units([np.inf, 1e30, np.inf, 1e38]) == ([], 4)
    edge, dropped = units([0.0, 0.0, 0.0, float(2 ** 30)])       # the last index AT the limit: a box like any other
    assert dropped == 0 and max(key[2] for key in edge) == 2 ** 30


@pytest.mark.parametrize("name", UNIFORM_CASES)
def test_specification_uniform_equals_the_reference(golden, spec, name):
    g, R = uniform_case(golden, name)[:2]
    for t in COLOR_TYPES:
        stages, pc, vx = spec.uniform(name, t)
        check_uniform(g, R, t, stages, pc, vx)
    n = int(g["u%d_pc_n" % R])
    if name in ("c1", "c2", "c3"):
        assert n == 0 and int(g["u%d_vx_n" % R]) > 0                   # nothing between voxels 1 and R - 2; the voxel cloud is there
    if name == "c4":
        assert n > 0                                                  # the first length that can carry a point, and does
    if name == "a":
        assert spec.uniform(name, 0)[0][1][1].max() == 64.0
    if name.startswith("e_"):
        w = spec.uniform(name, 0)[0][0][1].reshape(5, 5, 5)
        assert not w[:, :, :2].any()                                  # pz = -0.25 and pz == 0 exactly: never integrated
        assert w[2, 2, 2:].all() != name.endswith("_out") and w[2, 2, 2:].any() != name.endswith("_out")


def test_specification_frame_clouds_equal_the_reference(golden):
    frames, k = scene.hostile_frames()
    depth, rgb, gray, E = frames[0]
    for name, stride, posed in P_CASES:
        pts, _ = S.point_cloud_from_depth(depth, k, E if posed else None, stride)
        check_frame_cloud(pts, golden["d_p_%s_points" % name], not posed)
    assert len(golden["d_p_s1_id_points"]) == np.count_nonzero(depth > 0)  # +inf, 1e30 and the denormal are rows; NaN, -inf, -1, 0 are not
    pts, col = S.point_cloud_from_depth(depth, k, None, 1, color=rgb)
    check_frame_cloud(pts, golden["d_p_s1_id_points"], True)
    assert same_bits(col, golden["d_p_rgb_id_colors"])
    pts, col = S.point_cloud_from_depth(depth, k, None, 1, color=gray)
    assert same_bits(col, golden["d_p_gray_id_colors"].astype(np.float64))


@pytest.mark.parametrize("name", H_CASES)
def test_specification_scalable_equals_the_reference(golden, spec, name):
    """the unit sets equal the reference's without its junk units (an index beyond +-2^30: gen_rgbd_hostile.py asserts that
    exactly those stem from the dropped pixels); units and extractions as in test_tsdf.py"""
    sv, sets, pc, vx = spec.scalable(name)
    for i, keys in enumerate(sets):
        assert np.array_equal(np.array(keys, np.int32).reshape(-1, 3), golden["%s_units_f%d" % (name, i)]), (name, i)
    check_units(golden, name, sets[-1], lambda k: (sv["units"][k]["tsdf"], sv["units"][k]["weight"], sv["units"][k]["color"]))
    check_scalable_extraction(golden, name, pc, vx)
    junk = golden[name + "_junk_units"]
    assert (np.abs(junk) > S.UNIT_INDEX_LIMIT).any(1).all() and (len(junk) > 0) == (name != "h1")


def test_specification_frame_of_nothing_finite(golden):
    fr, k = scene.non_finite_frame()
    sv = S.new_scalable(0.05, 0.15, S.COLOR_NONE, 8, 1)
    S.scalable_integrate(sv, fr[0], None, k, fr[3])
    assert not sv["units"] and len(S.scalable_extract_point_cloud(sv)[0]) == 0
    ref = golden["hn_ref_units"]
    assert len(ref) > 0 and (np.abs(ref.astype(np.int64)) > S.UNIT_INDEX_LIMIT).any(1).all()   # all the reference opens is junk


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("t", COLOR_TYPES)
@pytest.mark.parametrize("name", UNIFORM_CASES)
def test_uniform_equals_the_reference_and_the_specification(lib, ctx, golden, spec, name, t):
    g, R, frames, k, length, trunc, origin = uniform_case(golden, name)
    h, w = frames[0][0].shape
    vol = ctx.tsdf_uniform(length, R, trunc, t, origin)
    stages = []
    for i, fr in enumerate(frames):
        vol.integrate(fr[0], color_of(fr, t), k, fr[3])
        if i in (0, len(frames) - 1) and len(stages) < (1 if len(frames) == 1 else 2):
            stages.append(vol.volume())
    pc, vx = vol.extract_point_cloud(), vol.extract_voxel_point_cloud()
    vol.close()
    check_uniform(g, R, t, stages, pc, vx)
    want_stages, want_pc, want_vx = spec.uniform(name, t)
    for got, want in zip(stages, want_stages):
        assert all((a is None and b is None) or same_bits(a, b) for a, b in zip(got, want))
    for got, want in zip(pc + vx, want_pc + want_vx):
        assert (got is None and want is None) or same_bits(got, want)
    print("%s, colour type %d: %d x %d into %d^3, %d frames, %d points, %d voxel points, weights up to %d: bit for bit"
          % (name, t, w, h, R, len(frames), len(pc[0]), len(vx[0]), int(stages[-1][1].max())))


@pytest.mark.gpu
def test_frame_clouds_equal_the_reference(lib, ctx, golden):
    frames, k = scene.hostile_frames()
    depth, rgb, gray, E = frames[0]
    for name, stride, posed in P_CASES:
        rel = check_frame_cloud(ctx.point_cloud_from_depth(depth, k, E if posed else None, stride), golden["d_p_%s_points" % name], not posed)
        print("%s: %d rows, finite rows within %.3g relative of the reference (bound %.0e)" % (name, len(golden["d_p_%s_points" % name]), rel, S.POINT_TOL))
    pts, col = ctx.point_cloud_from_rgbd(depth, rgb, k)
    check_frame_cloud(pts, golden["d_p_s1_id_points"], True)
    assert same_bits(col, golden["d_p_rgb_id_colors"])
    pts, col = ctx.point_cloud_from_rgbd(depth, gray, k)
    check_frame_cloud(pts, golden["d_p_s1_id_points"], True)
    assert same_bits(col, golden["d_p_gray_id_colors"].astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", H_CASES)
def test_scalable_equals_the_reference_and_the_specification(lib, ctx, golden, spec, name):
    R, stride, vl, trunc, t, nf = s_config(golden, name)
    frames, k = scene.hostile_frames()
    sv, sets, want_pc, want_vx = spec.scalable(name)
    vol = ctx.tsdf_scalable(vl, trunc, t, R, stride, initial_units=2)
    for i, fr in enumerate(frames[:nf]):
        vol.integrate(fr[0], color_of(fr, t), k, fr[3])
        assert np.array_equal(vol.units(), golden["%s_units_f%d" % (name, i)]), (name, i)
    check_units(golden, name, vol.units(), lambda key: vol.volume(key))
    pc, vx = vol.extract_point_cloud(), vol.extract_voxel_point_cloud()
    check_scalable_extraction(golden, name, pc, vx)
    for got, want in zip(pc + vx, want_pc + want_vx):
        assert (got is None and want is None) or same_bits(got, want)                 # the documented order, row for row
    # the frame of nothing finite changes nothing
    fr, nk = scene.non_finite_frame()
    vol.integrate(fr[0], color_of(fr, t), nk, fr[3])
    assert np.array_equal(vol.units(), golden["%s_units_f%d" % (name, nf - 1)])
    check_units(golden, name, vol.units(), lambda key: vol.volume(key))
    print("%s: units of %d^3, stride %d: %d units, %d points, %d voxel points" % (name, R, stride, len(vol.units()), len(pc[0]), len(vx[0])))
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 4])
def test_frame_of_nothing_finite_opens_no_unit(lib, ctx, stride):
    """+inf, NaN, -inf and 1e30 in every pixel: no unit, no error, empty extractions; an ordinary frame afterwards integrates"""
    fr, k = scene.non_finite_frame()
    vol = ctx.tsdf_scalable(0.05, 0.15, S.COLOR_RGB8, 8, stride, initial_units=2)
    vol.integrate(fr[0], fr[1], k, fr[3])
    assert len(vol.units()) == 0
    pts, nrm, col = vol.extract_point_cloud()
    assert len(pts) == 0 and len(nrm) == 0 and len(vol.extract_voxel_point_cloud()[0]) == 0
    frames, hk = scene.hostile_frames()
    vol.integrate(frames[0][0], frames[0][1], hk, frames[0][3])
    sv = S.new_scalable(0.05, 0.15, S.COLOR_RGB8, 8, stride)
    S.scalable_integrate(sv, frames[0][0], frames[0][1], hk, frames[0][3])
    assert len(sv["units"]) > 0 and np.array_equal(vol.units(), np.array(sorted(sv["units"]), np.int32))
    vol.close()
