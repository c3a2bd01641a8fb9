"""Generate tests/golden/rgbd_hostile.npz: what the compiled reference computes for the hostile inputs of
tests/test_tsdf_hostile.py, tests/test_odometry_hostile.py and tests/test_colormap_hostile.py (inputs chosen to break the
kernels, where tsdf.npz, odometry.npz and colormap.npz hold one well-behaved scene each).  Run once where the reference
checkout exists; the fixture holds DATA only, as a few large arrays (tests/packed_npz.py: it has over a thousand entries).

The harness texts, their builds and their readers are those of tests/golden/gen_tsdf.py, gen_odometry.py and
gen_colormap.py (imported, not copied); each is compiled against the reference in a scratch directory outside the
repository and runs with one OpenMP thread.  The inputs come from tests/tsdf_scene.py (asymmetric_frames, hostile_frames,
non_finite_frame, edge_case), tests/odometry_scene.py (hostile_cases) and tests/colormap_scene.py (boundary_case,
keep_pose_case, seam_case), so the tests rebuild them and the fixture holds results only.  A TSDF or odometry case's keys
are those of tsdf.npz or odometry.npz behind the case's prefix, so that the checks of tests/test_tsdf.py and
tests/test_odometry.py serve both fixtures.

TSDF:

  d_     DEPTH VALUES.  The first hostile frame (NaN, +inf, -inf, -1, 1e-40, 1e30, 0 among ordinary depths; fx != fy, a principal
         point off the centre) into a uniform 21^3 volume, every colour type: the volume in full, both extractions; and
         its point clouds (CreatePointCloudFromDepthImage, stride 1 and 4, identity and the frame's extrinsic;
         CreatePointCloudFromRGBDImage with both colour types) in full, non-finite rows included: d_p_*.
  c<R>_  COLUMN LENGTHS.  R in 1, 2, 3, 4, 5, 6, 7, 65 (every R % 4; columns shorter than a 16-byte vector; one voxel past a
         wave): the four 16 x 12 frames under the asymmetric intrinsic, every colour type.  R <= 3 extracts no surface
         point (asserted); R = 4 carries one (asserted).
  e_<name>_   IMAGE EDGES (tsdf_scene.edge_case): images of 1 x 1, 7 x 1, 1 x 7; a column whose u_f (v_f) lands on either side of
         0.0001 and of w - 0.0001, in exactly representable numbers -- asserted on the reference's weights: the column is
         integrated in the *_in cases and not in the *_out cases; a voxel at pz == 0 exactly and one at pz < 0 (weight 0).
  a_     A LONG RUNNING AVERAGE.  64 integrations of two alternating frames into 8^3: weights reach 64.
  h<i>_  SCALABLE, on the two hostile frames: h0 units of 8, stride 4; h1 a stride beyond the image (one pixel); h2 stride 5
         (divides neither side); h3 units of ONE voxel; h4 units of 5.  The reference converts the floor of a point that is
         not finite or beyond an int to int (undefined; x86-64: INT_MIN) and opens junk units there.  The library's rule
         (include/visma_icp.h): such a pixel touches no unit.  The generator removes the reference's units with an index
         beyond +-2^30 and asserts (1) that the specification, which states the rule, drops exactly the +inf and 1e30 pixels,
         (2) that what is left equals the specification's unit set exactly -- so at most those were removed -- and (3) that
         a removed unit holds no voxel with a weight, so that the extractions are those of the remaining units.
         hn_: the frame of nothing but non-finite depths: every unit the reference opens is junk (hn_ref_units, all removed).

ODOMETRY (o_*: odometry_scene.hostile_cases; per case the processed images, the correspondences and one step per level and
method at the identity, both full runs with their pairs per iteration, and ComputeRGBDOdometry with 1 and 3 threads; the
256 x 128 case through digests).  gen_odometry.check_margins refuses a case with a correspondence decision within 1e-9 of
its boundary, a determinant within a factor 10 of the 1e-6 guard, or a mean that depends on the order of its sum.

COLOR MAP (m_*: per case the visibility lists and the first proxies; the specification's images, masks, lists and proxies
equal the reference's, asserted): m_b vertices on the decisions (also colours after 0 and poses after 2 iterations, with the
case's pose_spread among the reference and the specification's two summation orders); m_k / m_k2 cameras that must keep
their pose (the reference's poses after 1 iteration, m_k_ref_extr_1, with what it did to each camera: m_k_ref_kept,
m_k_ref_finite; pose_spread of the ordinary cameras and of the camera with exactly 6); m_d<k> masks for dilation half-sizes
10, 11, 64; m_v<n>, m_c<n> vertex and camera counts at the seams.  These cases sit ON their boundaries on purpose, in
exactly representable numbers, so no stability-under-scaling check applies to them.

It asserts that every branch a case claims is met, on the specification's trace, and that the specification equals the
reference bit for bit before anything is stored.  The fp32 decisions need no margin (the specification reproduces them
exactly; the edge cases sit ON their boundaries on purpose, in exact numbers); the f64 floors of the scalable cases are
refused within 1e-9 of a boundary, which covers a scaling of the poses by 1 +- 1e-12.  Nothing compiled and no reference
text is kept."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["OMP_NUM_THREADS"] = "1"
import colormap_scene as cscene  # noqa: E402
import colormap_spec as CS  # noqa: E402
import gen_colormap as GC  # noqa: E402
import gen_odometry as GO  # noqa: E402
import gen_tsdf as GT  # noqa: E402
import odometry_scene as oscene  # noqa: E402
import odometry_spec as OS  # noqa: E402
import packed_npz  # noqa: E402
import tsdf_scene as scene  # noqa: E402
import tsdf_spec as S  # noqa: E402

COLUMN_RESOLUTIONS = (1, 2, 3, 4, 5, 6, 7, 65)
LENGTH, ORIGIN = GT.LENGTH, GT.ORIGIN
# name -> (volume_unit_resolution, depth_sampling_stride, voxel_length, sdf_trunc, colour type)
# (the 1e-40 pixel back-projects to the camera centre, whose coordinates are round numbers: the sdf_trunc values keep centre +-
#  sdf_trunc off the unit borders)
H_CASES = {"h0": (8, 4, 0.05, 0.13, 1), "h1": (8, 32, 0.05, 0.13, 2), "h2": (8, 5, 0.05, 0.13, 0), "h3": (1, 1, 0.2, 0.31, 1),
           "h4": (5, 2, 0.06, 0.15, 2)}
LIMIT = S.UNIT_INDEX_LIMIT


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def color_of(fr, t):
    return (None, fr[1], fr[2])[t]


def spec_uniform(R, t, frames, k, length, trunc, origin, trace=None, stages=None):
    vol = S.new_volume(length, R, trunc, t, origin)
    out = []
    for i, fr in enumerate(frames):
        S.integrate(vol, fr[0], color_of(fr, t), k, fr[3], trace=trace)
        if stages is not None and i in stages:
            out.append((vol["tsdf"].copy(), vol["weight"].copy(), None if vol["color"] is None else vol["color"].copy()))
    return vol, out


def record_uniform(fix, pre, R, frames, k, exe, length=LENGTH, trunc=None, origin=ORIGIN, full=True, need_points=None, gmin_floor=1e-3):
    """one uniform case, every colour type, under `pre` with the key names of tsdf.npz -> the specification's trace"""
    h, w = frames[0][0].shape
    res = [GT.run_uniform(exe, R, t, frames, k, length=length, trunc=trunc, origin=origin, w=w, h=h) for t in (0, 1, 2)]
    trunc = res[0]["trunc"]
    fix[pre + "u%d_sdf_trunc" % R] = np.float64(trunc)
    last = len(res[0]["stages"]) - 1
    tr = {}
    for t in (0, 1, 2):
        vol, st = spec_uniform(R, t, frames, k, length, trunc, origin, trace=tr if t == 1 else None, stages=(0, len(frames) - 1))
        for s in range(last + 1):                                      # the specification IS the reference, bit for bit
            ref = res[t]["stages"][s]
            got = st[0] if s == 0 else st[-1]
            assert bits_equal(got[0], ref["tsdf"]) and bits_equal(got[1], ref["weight"]), (pre, R, t, s)
            assert t == 0 or bits_equal(got[2], ref["color"]), (pre, R, t, s, "color")
    for s in range(last + 1):
        for t in (1, 2):
            assert bits_equal(res[t]["stages"][s]["tsdf"], res[0]["stages"][s]["tsdf"])
            assert bits_equal(res[t]["stages"][s]["weight"], res[0]["stages"][s]["weight"])
        g = res[2]["stages"][s]["color"]
        assert bits_equal(g[:, 0], g[:, 1]) and bits_equal(g[:, 0], g[:, 2])
        st = res[0]["stages"][s]
        p = pre + "u%d_s%d_" % (R, s)
        fix[p + "tsdf_sha"] = S.digest(st["tsdf"], np.float32); fix[p + "weight_sha"] = S.digest(st["weight"], np.float32)
        for t in (1, 2):
            fix[p + "t%d_color_sha" % t] = S.digest(res[t]["stages"][s]["color"], np.float32)
        if full and s == last:
            fix[p + "tsdf_full"] = st["tsdf"]; fix[p + "weight_full"] = st["weight"].astype(np.uint8)
            assert st["weight"].max() <= 255
            fix[p + "t1_color_full"] = res[1]["stages"][s]["color"]; fix[p + "t2_color_full"] = res[2]["stages"][s]["color"][:, 0]
    pc = res[0]["pc"]; n = len(pc["points"])
    for t in (1, 2):
        assert bits_equal(res[t]["pc"]["points"], pc["points"]) and bits_equal(res[t]["pc"]["normals"], pc["normals"])
        assert len(res[t]["pc"]["colors"]) == n
    assert len(pc["normals"]) == n and len(pc["colors"]) == 0
    if need_points is not None:
        assert (n > 0) == need_points, (pre, R, n)
    gmin = np.inf
    if n:
        vol = S.new_volume(length, R, trunc, S.COLOR_NONE, origin)
        vol["tsdf"], vol["weight"] = res[0]["stages"][last]["tsdf"].copy(), res[0]["stages"][last]["weight"].copy()
        grad = S.extract_point_cloud(vol, with_gradient=True)[3]
        gmin = float(np.linalg.norm(grad, axis=1).min())
        if gmin < gmin_floor:
            raise SystemExit("%sU%d: an extracted point's unnormalised gradient has norm %.3g, below %.3g: choose another input"
                             % (pre, R, gmin, gmin_floor))
    at = np.arange(0, n, max(1, -(-n // 150)))
    fix[pre + "u%d_pc_n" % R] = np.int64(n); fix[pre + "u%d_pc_at" % R] = at
    fix[pre + "u%d_pc_points_sha" % R] = S.digest(pc["points"], np.float64)
    fix[pre + "u%d_pc_points" % R] = pc["points"][at]; fix[pre + "u%d_pc_normals" % R] = pc["normals"][at]
    for t in (1, 2):
        fix[pre + "u%d_t%d_pc_colors_sha" % (R, t)] = S.digest(res[t]["pc"]["colors"], np.float64)
        fix[pre + "u%d_t%d_pc_colors" % (R, t)] = res[t]["pc"]["colors"][at]
    vx = res[0]["vx"]
    for t in (1, 2):
        assert bits_equal(res[t]["vx"]["points"], vx["points"]) and bits_equal(res[t]["vx"]["colors"], vx["colors"])
    fix[pre + "u%d_vx_n" % R] = np.int64(len(vx["points"]))
    fix[pre + "u%d_vx_points_sha" % R] = S.digest(vx["points"], np.float64); fix[pre + "u%d_vx_colors_sha" % R] = S.digest(vx["colors"], np.float64)
    print("%sU%d: %d extracted points, %d voxel points, weights up to %d, smallest gradient %.3g; %s"
          % (pre, R, n, len(vx["points"]), int(res[0]["stages"][last]["weight"].max()), gmin, {a: b for a, b in tr.items() if b}))
    return tr, res


def point_class(p):
    """per component: 0 finite, 1 NaN, 2 +inf, 3 -inf"""
    return (np.isnan(p) * 1 + (np.isposinf(p)) * 2 + (np.isneginf(p)) * 3).astype(np.uint8)


def tsdf_section(fix, exe):
    hostile, hk = scene.hostile_frames()
    # d_: depth values
    tr, res = record_uniform(fix, "d_", 21, hostile[:1], hk, exe)
    for key in ("behind", "hole", "clamped", "integrated", "depth_nan", "depth_negative", "depth_inf", "depth_huge", "depth_denormal"):
        assert tr[key] > 0, ("d_", key)
    depth, rgb, gray, E = hostile[0]
    n_pos = int(np.count_nonzero(depth > 0))
    for name, stride, ctype, ext in (("s1_id", 1, 0, np.eye(4)), ("s4_id", 4, 0, np.eye(4)), ("s1_e", 1, 0, E), ("s4_e", 4, 0, E),
                                     ("rgb_id", 1, 1, np.eye(4)), ("gray_id", 1, 2, np.eye(4))):
        c = GT.run(exe, "P", scene.HOSTILE_W, scene.HOSTILE_H, hk, [(depth, rgb, gray, ext)], struct.pack("<ii", stride, ctype))
        pc = c.cloud()
        assert c.at == len(c.v) and len(pc["normals"]) == 0 and len(pc["colors"]) == (len(pc["points"]) if ctype else 0)
        pts = pc["points"]
        sp, scol = S.point_cloud_from_depth(depth, hk, None if name.endswith("_id") else ext, stride, color=color_of((depth, rgb, gray), ctype))
        assert len(sp) == len(pts) and np.array_equal(point_class(sp), point_class(pts)), name
        fin = np.isfinite(pts).all(1)
        assert 0 < np.count_nonzero(~fin) < len(pts), name            # rows that are not finite among rows that are
        if name.endswith("_id"):
            assert bits_equal(sp[fin], pts[fin]), name
        else:
            rel = float(np.max(np.linalg.norm(sp[fin] - pts[fin], axis=1) / np.linalg.norm(pts[fin], axis=1)))
            assert rel <= S.POINT_TOL, (name, rel)
        if stride == 1:
            assert len(pts) == n_pos                                  # +inf, 1e30 and the denormal are rows; NaN, -inf, -1, 0 are not
        if ctype:
            assert bits_equal(pts, fix["d_p_s1_id_points"]) and bits_equal(scol, pc["colors"]), name
            fix["d_p_%s_colors" % name] = pc["colors"].astype(np.float32 if ctype == 2 else np.float64)
            assert np.array_equal(fix["d_p_%s_colors" % name].astype(np.float64), pc["colors"])
        else:
            fix["d_p_%s_points" % name] = pts
        print("d_p_%s: %d rows, %d of them not finite" % (name, len(pts), np.count_nonzero(~fin)))

    # c<R>_: column lengths
    frames4, k4 = scene.asymmetric_frames(scene.HOSTILE_W, scene.HOSTILE_H)
    for R in COLUMN_RESOLUTIONS:
        tr, res = record_uniform(fix, "c%d_" % R, R, frames4, k4, exe, full=R <= 7,
                                 need_points=False if R <= 3 else True if R == 4 else None)
        assert tr["integrated"] > 0 and len(res[0]["vx"]["points"]) > 0, R
        if R == 65:
            for key in ("behind", "left", "right", "top", "bottom", "hole", "far_behind", "clamped"):
                assert tr[key] > 0, (R, key)

    # e_: image edges
    for name in scene.EDGE_CASES:
        e = scene.edge_case(name)
        fr = [(e["depth"], e["rgb"], e["gray"], e["extrinsic"])]
        tr, res = record_uniform(fix, "e_%s_" % name, e["R"], fr, e["intrinsic"], exe, length=e["length"], trunc=e["sdf_trunc"],
                                 origin=e["origin"], gmin_floor=0.0)
        w = res[0]["stages"][0]["weight"].reshape(5, 5, 5)
        assert tr["at_camera_plane"] == 25 and tr["behind"] == 50 and not w[:, :, :2].any(), name
        axis_column = w[2, 2, 2:]
        if name.endswith("_out"):
            assert not axis_column.any(), (name, axis_column)
            assert tr["right" if "u_hi" in name else "left" if "u_lo" in name else "bottom" if "v_hi" in name else "top"] >= 3
        else:
            assert axis_column.all(), (name, axis_column)
        if name.endswith("_in") or name in ("1x1", "7x1", "1x7"):
            assert int(fix["e_%s_u5_pc_n" % name]) > 0, name

    # a_: a long running average
    two = [frames4[0], frames4[3]] * 32
    tr, res = record_uniform(fix, "a_", 8, two, k4, exe)
    assert res[0]["stages"][1]["weight"].max() == 64.0

    # h<i>_: scalable volumes on the two hostile frames
    for name, (R, stride, vl, trunc, ctype) in H_CASES.items():
        scalable_case(fix, exe, name, R, stride, vl, trunc, ctype, hostile, hk)
    nf, nk = scene.non_finite_frame()
    c = GT.run(exe, "S", scene.HOSTILE_W, scene.HOSTILE_H, nk, [nf], struct.pack("<iii2d", 8, 0, 1, 0.05, 0.15))
    m = int(c.take(1)[0])
    keys = c.take(3 * m).astype(np.int64).reshape(m, 3)
    assert m > 0 and (np.abs(keys) > LIMIT).any(1).all()               # every unit the reference opens for this frame is junk
    sv = S.new_scalable(0.05, 0.15, 0, 8, 1)
    tr = {}
    S.scalable_integrate(sv, nf[0], None, nk, nf[3], trace=tr)
    assert not sv["units"] and tr["dropped_pixels"] == int(np.count_nonzero(nf[0] > 0)) > 0
    fix["hn_ref_units"] = keys.astype(np.int32)
    print("hn: the reference opens %d junk units, the rule none (%d pixels dropped)" % (m, tr["dropped_pixels"]))


def scalable_case(fix, exe, name, R, stride, vl, trunc, ctype, frames, k):
    nf = len(frames)
    c = GT.run(exe, "S", scene.HOSTILE_W, scene.HOSTILE_H, k, frames, struct.pack("<iii2d", R, ctype, stride, vl, trunc))
    sets = []
    for i in range(nf):
        m = int(c.take(1)[0])
        sets.append(c.take(3 * m).astype(np.int64).reshape(m, 3))
    n3 = R ** 3
    units, junk = {}, []
    for key in map(tuple, sets[-1].tolist()):
        u = dict(tsdf=c.take(n3).astype(np.float32), weight=c.take(n3).astype(np.float32),
                 color=c.take(3 * n3).astype(np.float32).reshape(n3, 3) if ctype else None)
        if max(abs(v) for v in key) > LIMIT:
            assert not u["weight"].any(), (name, key)                 # (3) a removed unit holds nothing
            junk.append(key)
        else:
            units[key] = u
    pc, vx = c.cloud(), c.cloud()
    assert c.at == len(c.v)
    kept = [a[(np.abs(a) <= LIMIT).all(1)] for a in sets]
    kept = [a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))].astype(np.int32) for a in kept]
    tr = {}
    sv = S.new_scalable(vl, trunc, ctype, R, stride)
    for fr in frames:                                                  # the f64 floors first: a set that differs on a boundary is no finding
        S.touched_units(S.new_scalable(vl, trunc, ctype, R, stride), fr[0], k, fr[3], trace=tr)
    if tr["floor_margin"] < 1e-9:
        raise SystemExit("%s: a floor of point / volume_unit_length sits within 1e-9 of its boundary: choose another input" % name)
    tr = {}
    for i, fr in enumerate(frames):
        before = tr.get("dropped_pixels", 0)
        S.scalable_integrate(sv, fr[0], color_of(fr, ctype), k, fr[3], trace=tr)
        strided = fr[0][::stride, ::stride]
        hostile_here = int(np.count_nonzero(np.isposinf(strided) | (strided > 1e20)))
        assert tr["dropped_pixels"] - before == hostile_here, (name, i)          # (1) exactly the +inf and 1e30 pixels are dropped
        assert sorted(sv["units"]) == list(map(tuple, kept[i].tolist())), (name, i)   # (2) what is left is the rule's set, exactly
        assert (len(sets[i]) > len(kept[i])) == (hostile_here > 0), (name, i)
    assert len(kept[0]) > 0
    for key, u in units.items():                                       # the specification IS the reference, unit by unit
        su = sv["units"][key]
        assert bits_equal(su["tsdf"], u["tsdf"]) and bits_equal(su["weight"], u["weight"]), (name, key)
        assert not ctype or bits_equal(su["color"], u["color"]), (name, key)
    grad = S.scalable_extract_point_cloud(sv, with_gradient=True)[3]
    gmin = float(np.linalg.norm(grad, axis=1).min()) if len(grad) else np.inf
    if gmin < 1e-3:
        raise SystemExit("%s: an extracted point's unnormalised gradient has norm below 1e-3: choose another input" % name)
    print("%s: units per frame %s (the reference: %s, %d junk), %d extracted points, %d voxel points, %d pixels dropped, floor margin %.3g, "
          "smallest gradient %.3g" % (name, [len(a) for a in kept], [len(a) for a in sets], len(junk), len(pc["points"]), len(vx["points"]),
                                      tr["dropped_pixels"], tr["floor_margin"], gmin))
    fix[name + "_config"] = np.array([R, stride, vl, trunc, ctype, nf])
    fix[name + "_junk_units"] = np.array(junk, np.int64).reshape(-1, 3)
    for i, a in enumerate(kept):
        fix["%s_units_f%d" % (name, i)] = a
    keys = list(map(tuple, kept[-1].tolist()))
    sha = np.stack([S.digest(np.concatenate([units[q]["tsdf"], units[q]["weight"]] + ([units[q]["color"].ravel()] if ctype else [])),
                             np.float32) for q in keys])
    fix[name + "_unit_sha8"] = sha[:, :8].copy()
    fix[name + "_units_sha"] = S.digest(sha, np.uint8)
    probe_units = keys[::max(1, len(keys) // 3)][:3]
    fix[name + "_probe_units"] = np.array(probe_units, np.int32)
    fix[name + "_probe_tsdf"] = np.stack([units[q]["tsdf"] for q in probe_units])
    fix[name + "_probe_weight"] = np.stack([units[q]["weight"] for q in probe_units]).astype(np.uint8)
    if ctype:
        fix[name + "_probe_color"] = np.stack([units[q]["color"] for q in probe_units])
    pts, nrm, col = S.sort_rows(pc["points"], pc["normals"], pc["colors"] if ctype else None)
    n = len(pts); at = np.arange(0, n, max(1, -(-n // 100)))
    fix[name + "_pc_n"] = np.int64(n); fix[name + "_pc_at"] = at
    fix[name + "_pc_points_sha"] = S.digest(pts, np.float64)
    fix[name + "_pc_points"] = pts[at]; fix[name + "_pc_normals"] = nrm[at]
    if ctype:
        fix[name + "_pc_colors_sha"] = S.digest(col, np.float64); fix[name + "_pc_colors"] = col[at]
    vp, vc = S.sort_rows(vx["points"], vx["colors"])
    fix[name + "_vx_n"] = np.int64(len(vp))
    fix[name + "_vx_points_sha"] = S.digest(vp, np.float64); fix[name + "_vx_colors_sha"] = S.digest(vc, np.float64)


# ---------------------------------------------------------------------------
# odometry (the harness, its build and its reader are those of gen_odometry.py)
# ---------------------------------------------------------------------------
def odometry_cases():
    """name -> (frames, iterations, colour iterations, option): what tests/test_odometry_hostile.py rebuilds"""
    return {name: (fr, its, itc, dict(OS.default_option(), min_depth=md)) for name, (fr, its, itc, md) in oscene.hostile_cases().items()}


def record_odometry(fix, exe, case, frames, its, its_color, opt):
    init = np.eye(4)
    GO.check_margins(case, frames, init, opt, its, [(OS.HYBRID, its), (OS.COLOR, its_color)])
    r = GO.run_case(exe, frames, init, its, its_color, opt)
    digests = frames[0].size > 4096
    fix[case + "_option"] = np.array([opt["max_depth_diff"], opt["min_depth"], opt["max_depth"]])
    fix[case + "_iterations"] = np.array(its, np.int32); fix[case + "_color_iterations"] = np.array(its_color, np.int32)
    for l, L in enumerate(r["levels"]):
        for name in OS.WHICH:
            if name == "src_xyz":
                assert OS.same_image(L[name][..., 2], L["src_depth"])
            if digests:
                fix["%s_l%d_%s_sha" % (case, l, name)] = OS.image_digest(L[name])
            else:
                fix["%s_l%d_%s" % (case, l, name)] = L[name] if name != "src_xyz" else L[name][..., :2]
        if digests:
            fix["%s_l%d_idx_sha" % (case, l)] = S.digest(L["idx"], np.int32)
        else:
            fix["%s_l%d_idx" % (case, l)] = L["idx"]
        fix["%s_l%d_pairs" % (case, l)] = np.int64(np.count_nonzero(L["idx"] >= 0))
    for (l, m, p), st in r["steps"].items():
        if p == "init":
            for key, val in st.items():
                fix["%s_l%d_m%d_%s_%s" % (case, l, m, p, key)] = val
    for run in ("hybrid", "color"):
        fix["%s_%s_poses" % (case, run)] = r[run]["poses"]; fix["%s_%s_counts" % (case, run)] = r[run]["counts"]
        fix["%s_%s_ok" % (case, run)] = r[run]["ok"]
        for th in (1, 3):
            res = r[run + "_result"][th]
            assert res["ok"] == r[run]["ok"]
            fix["%s_%s_T_%d" % (case, run, th)] = res["T"]; fix["%s_%s_info_%d" % (case, run, th)] = res["info"]
    print("%s: %s, pairs at the identity per level %s; hybrid ok %d, pairs per iteration %s; colour ok %d, %s; NaN depths in the processed "
          "source %d" % (case, "x".join(str(v) for v in frames[0].shape[::-1]), [int(fix["%s_l%d_pairs" % (case, l)]) for l in range(len(its))],
                         r["hybrid"]["ok"], r["hybrid"]["counts"].tolist(), r["color"]["ok"], r["color"]["counts"].tolist(),
                         int(np.isnan(r["levels"][0]["src_depth"]).sum())))
    return r


def odometry_section(fix, exe):
    res = {}
    for case, (frames, its, its_color, opt) in odometry_cases().items():
        res[case] = record_odometry(fix, exe, case, frames, its, its_color, opt)
    # every branch a case claims
    r = res["o_const"]
    assert r["hybrid"]["ok"] == 0 and r["color"]["ok"] == 0 and int(fix["o_const_l0_pairs"]) == 63       # singular, with every pixel paired
    assert not r["steps"][(0, 0, "init")]["JTJ"].any()                  # the colour term's J^T J is the zero matrix
    for n in sorted(oscene.FEW_PAIR_BLOCKS):
        assert int(fix["o_n%d_l0_pairs" % n]) == n, n
        assert r["hybrid"]["counts"][0] > 0
    v = res["o_v"]
    for l in range(2):
        L = res["o_v2"]["levels"][l]
        assert np.isnan(L["src_depth"]).any() and np.isnan(L["tgt_depth"]).any() and not np.isnan(L["src_depth"]).all()
        t = L["idx"][L["idx"] >= 0]
        assert np.isnan(L["tgt_depth_dx"].ravel()[t]).any() or np.isnan(L["tgt_depth_dy"].ravel()[t]).any(), l   # the isnan -> 0 of the hybrid term is met
    assert v["hybrid"]["ok"] == 1 and len(v["hybrid"]["counts"]) == 5 and v["color"]["ok"] == 1
    assert res["o_v2"]["hybrid"]["ok"] == 0 and res["o_v2"]["hybrid"]["counts"].tolist() == [6]     # six pairs at level 1, and no solution
    assert res["o_deep"]["levels"][7]["src_gray"].shape == (1, 2) and len(res["o_deep"]["levels"]) == 8
    assert res["o_9x7"]["levels"][1]["src_gray"].shape == (3, 4)


# ---------------------------------------------------------------------------
# color map (the harness, its build and its runner are those of gen_colormap.py)
# ---------------------------------------------------------------------------
SEAM_VERTICES, SEAM_CAMERAS, DILATIONS = (1, 255, 256, 257, 512), (1, 32, 33, 64, 65), (10, 11, 64)


def colormap_stages(fix, exe, name, case, keep_masks=False, stable=True):
    """images, masks, visibility and the first proxies of a case: the specification equals the reference (asserted), the
    fixture keeps the lists and the proxies -> the specification's state.  stable: the decisions (visibility bits, margin
    tests, rounded pixels of the proxies, one iteration and the colours) are the same with every extrinsic entry scaled by
    1 +- 1e-12 -- not asked of the case that sits on its boundaries on purpose"""
    depths, colors, E, K, V, over = case
    option = dict(CS.default_option(), **over)
    n, h, w = depths.shape
    out = GC.run(exe, "stages", depths, colors, E, K, V, option, 0)
    imgs = out[:3 * n * h * w].reshape(n, 3, h, w).astype(np.float32)
    masks = out[3 * n * h * w:4 * n * h * w].reshape(n, h, w).astype(np.uint8)
    at = 4 * n * h * w
    lists = []
    for c in range(n):
        m = int(out[at]); lists.append(np.sort(out[at + 1:at + 1 + m].astype(np.int32))); at += 1 + m
    proxy = out[at:at + len(V)].copy()
    assert at + len(V) == len(out)
    st = CS.State(V, depths, colors, E, K, option)
    for c in range(n):
        for t, im in enumerate((st.gray[c], st.dx[c], st.dy[c])):
            assert bits_equal(im, imgs[c, t]), (name, "image", c, t)
        assert np.array_equal(st.mask[c], masks[c]), (name, "mask", c)
        assert np.array_equal(st.lists[c], lists[c]), (name, "visibility", c, st.lists[c], lists[c])
    assert bits_equal(st.proxy(), proxy), (name, "proxy")
    fix[name + "_vis_n"] = np.array([len(x) for x in lists], np.int64)
    fix[name + "_vis_list"] = np.concatenate(lists).astype(np.int32)
    fix[name + "_proxy0"] = proxy
    if keep_masks:
        fix[name + "_mask"] = masks
    if stable:
        base = GC.decisions(V, depths, colors, E, K, option, 1)
        for f in (1 + 1e-12, 1 - 1e-12):
            other = GC.decisions(V, depths, colors, E * f, K, option, 1)
            assert len(base) == len(other) and all(np.array_equal(a, b) for a, b in zip(base, other)), (name, "an unstable decision", f)
    return st, masks


def colormap_run(exe, case, k):
    depths, colors, E, K, V, over = case
    out = GC.run(exe, "run", depths, colors, E, K, V, dict(CS.default_option(), **over), k)
    n = len(depths)
    return out[:16 * n].reshape(n, 4, 4).copy(), out[16 * n:].reshape(len(V), 3).copy()


def pose_spread(case, ref_E, k, cameras):
    """the largest entry-wise distance among the reference and the specification with sequential and with pairwise sums after
    k iterations, over `cameras` (at least 1e-15), and the pairwise specification's poses"""
    depths, colors, E, K, V, over = case
    spec = {}
    for how in ("sequential", "pairwise"):
        st = CS.State(V, depths, colors, E, K, dict(CS.default_option(), **over))
        st.run(k, how)
        spec[how] = st.E.copy()
    d = lambda a, b: float(np.abs(a[cameras] - b[cameras]).max())
    return max(d(spec["sequential"], ref_E), d(spec["pairwise"], ref_E), d(spec["sequential"], spec["pairwise"]), 1e-15), spec["pairwise"]


def colormap_section(fix, exe):
    # m_b: vertices on the decisions
    case = cscene.boundary_case()
    depths, colors, E, K, V, over = case
    st, _ = colormap_stages(fix, exe, "m_b", case, stable=False)
    seen = st.vis.any(0)
    assert not seen[62:66].any(), "a vertex that is not finite, at a camera centre or behind a camera is visible"
    bad = [12 * 3 + 2, 12 * 3 + 8, 12 * 1 + 9]                          # the grid vertices on the NaN, +inf and -1 pixels of camera 0
    assert not st.vis[0, bad].any() and st.vis[1, bad].all() and st.vis[0, :48].sum() > 30
    u32, v32, _ = CS.project(E[0], K, V)
    in32 = CS.inside(u32, v32, cscene.HW, cscene.HH)
    tr = []
    CS.terms(V, np.arange(len(V) - 4), E[0], K, st.gray[0], st.dx[0], st.dy[0], np.zeros(len(V)), tr)
    in64 = np.concatenate([tr[0], np.zeros(4, bool)])
    # u == 10: inside; one ulp below: outside; above: inside.  u == 22: outside; below: inside; above: outside.  v likewise.
    assert in32[48:60].tolist() == [True, False, True, False, True, False] * 2 and in64[48:60].tolist() == in32[48:60].tolist()
    assert in32[60] and not in64[60] and not in32[61] and in64[61]      # the two that fp32 and f64 decide differently
    ref0 = colormap_run(exe, case, 0)
    ref2 = colormap_run(exe, case, 2)
    assert bits_equal(ref0[0], E) and np.abs(st.colours() - ref0[1]).max() <= 1e-15
    fix["m_b_colors_0"], fix["m_b_extr_2"] = ref0[1], ref2[0]
    spread, _ = pose_spread(case, ref2[0], 2, [0, 1])
    fix["m_b_pose_spread"] = np.float64(spread)
    print("m_b: visible %s, pose spread after 2 iterations %.3g, the poses moved by %.3g" % (fix["m_b_vis_n"], spread, np.abs(ref2[0] - E).max()))

    # m_k: cameras that must keep their pose (m_k2: the same vertices under cameras 0 and 1 alone)
    case, case2 = cscene.keep_pose_case(), cscene.keep_pose_case(False)
    st, _ = colormap_stages(fix, exe, "m_k", case)
    colormap_stages(fix, exe, "m_k2", case2)
    assert fix["m_k_vis_n"].tolist() == [72, 72, 1, 2, 3, 4, 5, 6, 10] and fix["m_k2_vis_n"].tolist() == [72, 72]
    p = st.proxy()
    assert [len(st.terms(c, p)) for c in range(9)] == [72, 72, 1, 2, 3, 4, 5, 6, 10]            # every visible vertex is accepted
    assert not st.dx[cscene.KEEP_CONSTANT].any() and not st.dy[cscene.KEEP_CONSTANT].any()
    ref1, ref1b = colormap_run(exe, case, 1), colormap_run(exe, case2, 1)
    assert bits_equal(ref1[0][:2], ref1b[0])                           # the reference's ordinary cameras do not notice the others either
    fix["m_k_ref_extr_1"] = ref1[0]
    spread, spec_E = pose_spread(case, ref1[0], 1, [0, 1])
    fix["m_k_pose_spread"] = np.float64(spread)
    fix["m_k_pose_spread_7"] = np.float64(pose_spread(case, ref1[0], 1, [7])[0])    # exactly 6 equations for 6 unknowns: ill-conditioned
    fix["m_k_ref_kept"] = np.array([bits_equal(ref1[0][c], case[2][c]) for c in range(9)])
    fix["m_k_ref_finite"] = np.array([bool(np.isfinite(ref1[0][c]).all()) for c in range(9)])
    print("m_k: after 1 iteration the reference's cameras keep their pose: %s; finite: %s; camera 7 (exactly 6): the reference and the "
          "specification %.3g apart; pose spread of cameras 0, 1 %.3g"
          % (fix["m_k_ref_kept"].astype(int), fix["m_k_ref_finite"].astype(int), np.abs(ref1[0][7] - spec_E[7]).max(), spread))

    # m_d<k>: dilation at, just above and far above half of a 21 x 21 image
    for k in DILATIONS:
        st, masks = colormap_stages(fix, exe, "m_d%d" % k, cscene.seam_case(40, 2, k), keep_masks=True)
        assert (masks == 255).any() and ((masks != 255).any() == (k < 64)), (k, (masks == 255).mean())
    # m_v<n>, m_c<n>: counts at the seams
    for nv in SEAM_VERTICES:
        st, _ = colormap_stages(fix, exe, "m_v%d" % nv, cscene.seam_case(nv, 2))
        p = st.proxy()
        assert nv == 1 or 0 < len(st.terms(0, p)) < len(st.lists[0])
    for nc in SEAM_CAMERAS:
        st, _ = colormap_stages(fix, exe, "m_c%d" % nc, cscene.seam_case(40, nc))
        assert all(len(x) > 0 for x in st.lists)


def main():
    fix = {"length": np.float64(LENGTH), "origin": np.array(ORIGIN)}
    tsdf_section(fix, GT.build())
    odometry_section(fix, GO.build())
    colormap_section(fix, GC.build())
    out = os.path.join(HERE, "rgbd_hostile.npz")
    packed_npz.save(out, fix)                                          # (a thousand small arrays: see tests/packed_npz.py)
    size, limit = os.path.getsize(out), os.path.getsize(os.path.join(HERE, "tsdf.npz"))
    print("rgbd_hostile.npz: %d bytes (tsdf.npz: %d)" % (size, limit))
    if size > limit:
        raise SystemExit("the fixture is larger than tsdf.npz")


if __name__ == "__main__":
    main()
