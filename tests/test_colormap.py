"""Color map optimization (visma_icp_color_map_*; colormap.hip).

The yardstick is the numpy specification tests/colormap_spec.py; tests/golden/colormap.npz (tests/golden/gen_colormap.py)
pins it to the compiled reference on the scene of tests/colormap_scene.py (83 x 61, six cameras, 3201 vertices).  Levels:
  exact     images, masks, visibility lists, the proxies before iteration 1 (sums of at most six floats in doubles)
  bounded   a camera's 29 sums: K 2^-53 sum|term| per sum, K its count (colormap_spec.sum_bound)
  measured  the extrinsics after 8 iterations: 100 x the fixture's pose_spread (the spread among the reference and the
            specification with sequential and with pairwise sums)
  colours   1e-15 absolute
The launch shape test 9 names: the iteration kernel runs 512 workgroups of 256 lanes per camera at most
(kColorMapMaxBlocks), so a camera with more than 131,072 visible vertices walks its list in strides."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import colormap_scene as scene
import colormap_spec as S
from oracle_engine import OracleEngine

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, STATE = 1, 5
STRIDE_SHAPE = 512 * 256


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "colormap.npz"))
    return {k: g[k] for k in g.files}


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def spec_option(**kw):
    o = S.default_option()
    o["maximum_allowable_depth"] = scene.MAX_DEPTH
    o.update(kw)
    return o


@pytest.fixture(scope="module")
def inputs(golden):
    """the scene as the generator saw it (digests checked): depths, colors, extrinsics, intrinsic, vertices"""
    depths, colors, E, K = scene.frames()
    V = scene.vertices()
    assert np.array_equal(sha(depths), golden["depths_sha"]) and np.array_equal(sha(colors), golden["colors_sha"])
    assert np.array_equal(sha(V), golden["vertices_sha"]) and np.array_equal(E, golden["extrinsics0"]) and np.array_equal(K, golden["intrinsic"])
    return depths, colors, E, K, V


@pytest.fixture(scope="module")
def spec(inputs):
    """the specification on the fixture case, computed once and left unchanged: the prepared state, the rows of iteration
    1, the states after 1 and 8 iterations, the residual history"""
    depths, colors, E, K, V = inputs
    st = S.State(V, depths, colors, E, K, spec_option())
    run = S.State(V, depths, colors, E, K, spec_option())
    out = dict(state=st, proxy0=st.proxy(), colors0=st.colours())
    res = [run.step()[:, 27].sum()]
    out["E1"] = run.E.copy()
    res += list(run.run(7))
    out["E8"], out["colors8"], out["residual"] = run.E.copy(), run.colours(), np.array(res)
    return out


def lists_of(golden):
    at = np.concatenate([[0], np.cumsum(golden["vis_n"])])
    return [golden["vis_list"][at[c]:at[c + 1]] for c in range(len(golden["vis_n"]))]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_specification_images_masks_visibility_proxy_equal_the_reference(golden, inputs, spec):
    depths, colors, E, K, V = inputs
    st = spec["state"]
    n, h, w = depths.shape
    for c in range(n):
        for t, im in enumerate((st.gray[c], st.dx[c], st.dy[c])):
            assert np.array_equal(S.O.image_digest(im), golden["img_sha"][c, t]), (c, t)
            assert np.array_equal(im[(0, h // 2, h - 1), :].view(np.uint32), golden["img_rows"][c, t].view(np.uint32))
        for k in (0, 1, 3):
            assert np.array_equal(S.depth_mask(depths[c], 0.1, k), golden["mask_k%d" % k][c]), (c, k)
        assert np.array_equal(st.lists[c], lists_of(golden)[c])
    assert np.array_equal(spec["proxy0"], golden["proxy0"])


def test_specification_poses_and_colours_equal_the_reference(golden, spec):
    tol = 100.0 * float(golden["pose_spread"])
    assert np.abs(spec["E1"] - golden["extr_1"]).max() <= tol
    assert np.abs(spec["E8"] - golden["extr_8"]).max() <= tol
    assert np.abs(spec["colors0"] - golden["colors_0"]).max() <= 1e-15
    assert np.abs(spec["colors8"] - golden["colors_8"]).max() <= 1e-15
    assert spec["residual"][7] < spec["residual"][0]
    assert np.allclose(spec["residual"], golden["spec_residual"], rtol=1e-9, atol=0)


def test_option_defaults_and_methods(lib):
    o = lib.color_map_option()
    assert (o.non_rigid_camera_coordinate, o.number_of_vertical_anchors, o.half_dilation_kernel_size_for_discontinuity_map) == (0, 16, 3)
    assert (o.non_rigid_anchor_point_weight, o.maximum_iteration, o.maximum_allowable_depth) == (0.316, 300.0, 2.5)
    assert (o.depth_threshold_for_visiblity_check, o.depth_threshold_for_discontinuity_check) == (0.03, 0.1)
    d = S.default_option()
    assert all(getattr(o, k) == d[k] for k in d)
    assert lib.color_map_option(maximum_iteration=8).maximum_iteration == 8.0
    for name in ("color_map", "color_map_optimization"):
        assert callable(getattr(lib.Context, name, None)), name
    for name in ("set_image", "set_vertices", "prepare", "image", "visible", "proxy", "sums", "step", "run", "extrinsics", "set_extrinsics",
                 "colors", "close"):
        assert callable(getattr(lib.ColorMap, name, None)), name


@pytest.fixture()
def hctx(lib, oracle):
    eng = OracleEngine(oracle)
    ctx = eng.context()
    ctx.engine = eng
    yield ctx
    ctx.close()


def test_create_checks_come_before_the_device(lib, hctx):
    """a context on the oracle engine has no device: a create that passes its checks ends at that engine's "not supported"
    (VISMA_ICP_ERR_STATE); every argument error is VISMA_ICP_ERR_INVALID, the non-rigid flag among them"""
    L, h = hctx.L, hctx._h
    m = C.c_void_p()
    k = np.array([70.0, 70.0, 41.0, 30.0]); pk = k.ctypes.data_as(C.POINTER(C.c_double))

    def create(w=83, hh=61, n=2, intr=pk, option=None, out=C.byref(m), ctx=h):
        return L.visma_icp_color_map_create(ctx, w, hh, n, intr, None if option is None else C.byref(option), out)

    assert create() == STATE
    assert create(ctx=None) == INVALID and create(out=None) == INVALID and create(intr=None) == INVALID
    assert create(n=0) == INVALID and create(n=-1) == INVALID
    assert create(w=20) == INVALID and create(hh=20) == INVALID and create(w=0) == INVALID and create(w=21, hh=21) == STATE
    bad = np.array([0.0, 70.0, 41.0, 30.0])
    assert create(intr=bad.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    assert create(option=lib.color_map_option(non_rigid_camera_coordinate=1)) == INVALID
    assert create(option=lib.color_map_option(half_dilation_kernel_size_for_discontinuity_map=-1)) == INVALID
    assert create(option=lib.color_map_option(maximum_allowable_depth=float("nan"))) == INVALID
    assert create(option=lib.color_map_option()) == STATE
    z = np.zeros(16)
    pz = z.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.visma_icp_color_map_optimization(h, 83, 61, 1, pk, np.zeros(83 * 61, np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                                            np.zeros(83 * 61 * 3, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), pz, pz, 1,
                                            C.byref(lib.color_map_option(non_rigid_camera_coordinate=1)), pz)
    assert rc == INVALID and not z.any()
    assert L.visma_icp_color_map_destroy(h, None) == INVALID and L.visma_icp_color_map_prepare(h, None, None) == INVALID


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def lib_option(lib, **kw):
    return lib.color_map_option(maximum_allowable_depth=scene.MAX_DEPTH, **kw)


def new_map(lib, ctx, depths, colors, E, K, V, **kw):
    n, h, w = depths.shape
    m = ctx.color_map(w, h, n, K, lib_option(lib, **kw))
    for i in range(n):
        m.set_image(i, depths[i], colors[i], E[i])
    m.set_vertices(V)
    return m


@pytest.fixture(scope="module")
def prepared(lib, ctx, inputs):
    depths, colors, E, K, V = inputs
    m = new_map(lib, ctx, depths, colors, E, K, V)
    counts = m.prepare()
    yield m, counts
    m.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def check_sums(rows, state, proxy):
    """rows (n x 29) against the specification's terms within the bound; the count equal"""
    for c in range(len(rows)):
        T = state.terms(c, proxy)
        want, bound = S.total(T), S.sum_bound(T)
        err = np.abs(rows[c] - want)
        print("camera %d: %d terms, worst error / bound %.3g" % (c, len(T), np.max(err / np.maximum(bound, 1e-300)) if len(T) else 0.0))
        assert rows[c][28] == len(T)
        assert np.all(err <= bound), (c, err, bound)


@pytest.mark.gpu
def test_staged_outputs_equal_the_reference(lib, golden, inputs, spec, prepared):
    """test 1: every staged output of the fixture case"""
    depths, colors, E, K, V = inputs
    m, counts = prepared
    n, h, w = depths.shape
    assert np.array_equal(counts, golden["vis_n"])
    for c in range(n):
        for t, which in enumerate(("gray", "dx", "dy")):
            im = m.image(c, which)
            assert np.array_equal(S.O.image_digest(im), golden["img_sha"][c, t]), (c, which)
            assert np.array_equal(bits(im[(0, h // 2, h - 1), :]), bits(golden["img_rows"][c, t]))
        assert np.array_equal(m.image(c, "mask"), golden["mask_k3"][c]), c
        assert np.array_equal(m.visible(c), lists_of(golden)[c]), c
    assert np.array_equal(bits(m.extrinsics()), bits(E))
    assert np.array_equal(bits(m.proxy()), bits(golden["proxy0"]))
    # the sums at the fixture's poses after iteration 1 (visibility stays that of the initial poses)
    m.set_extrinsics(golden["extr_1"])
    st = S.State(V, depths, colors, E, K, spec_option())
    st.E = golden["extr_1"].copy()
    p1 = st.proxy()
    assert np.array_equal(bits(m.proxy()), bits(p1))
    rows = m.sums()
    assert np.array_equal(bits(m.extrinsics()), bits(golden["extr_1"]))        # sums moves nothing
    check_sums(rows, st, p1)
    m.set_extrinsics(E)


@pytest.mark.gpu
def test_eight_iterations(lib, ctx, golden, inputs, spec):
    """tests 2, 5 and 6: the 8-iteration run against the reference; a repeated run is bit-identical; the residual history
    against the specification's within the sum bound of its rr terms"""
    depths, colors, E, K, V = inputs
    runs = []
    for _ in range(2):
        m = new_map(lib, ctx, depths, colors, E, K, V)
        m.prepare()
        res = m.run(8)
        runs.append((m.extrinsics(), m.colors(), res))
        m.close()
    E8, col8, res = runs[0]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(runs[0], runs[1]))
    tol = 100.0 * float(golden["pose_spread"])
    dist = np.abs(E8 - golden["extr_8"]).max()
    print("pose_spread %.3g, tolerance %.3g, reached %.3g; colours %.3g" % (float(golden["pose_spread"]), tol, dist, np.abs(col8 - golden["colors_8"]).max()))
    assert dist <= tol
    assert np.abs(col8 - golden["colors_8"]).max() <= 1e-15
    assert res[7] < res[0]
    # the bound of a residual: the sum bounds of the cameras' rr columns at the specification's poses of that iteration
    st = S.State(V, depths, colors, E, K, spec_option())
    for it in range(8):
        p = st.proxy()
        bound = sum(S.sum_bound(st.terms(c, p))[27] for c in range(len(E)))
        print("iteration %d: residual %.17g, specification %.17g, bound %.3g" % (it + 1, res[it], spec["residual"][it], bound))
        assert abs(res[it] - spec["residual"][it]) <= bound, it
        st.step()


@pytest.mark.gpu
def test_zero_iterations_and_one_call(lib, ctx, golden, inputs):
    """tests 3 and 4: zero iterations change no pose and still colour; the one-call entry point equals the staged path"""
    depths, colors, E, K, V = inputs
    E0, col0 = ctx.color_map_optimization(V, depths, colors, K, E, lib_option(lib, maximum_iteration=0))
    assert np.array_equal(bits(E0), bits(E))
    assert np.abs(col0 - golden["colors_0"]).max() <= 1e-15
    E2, col2 = ctx.color_map_optimization(V, depths, colors, K, E, lib_option(lib, maximum_iteration=2))
    m = new_map(lib, ctx, depths, colors, E, K, V)
    m.prepare()
    m.run(2)
    assert np.array_equal(bits(E2), bits(m.extrinsics())) and np.array_equal(bits(col2), bits(m.colors()))
    assert np.abs(E2 - golden["extr_2"]).max() <= 100.0 * float(golden["pose_spread"])
    m.close()


@pytest.mark.gpu
def test_a_camera_that_sees_nothing_keeps_its_pose(lib, ctx, inputs):
    """test 7: a seventh camera turned away reports count 0 and keeps its pose; the others do not notice it"""
    depths, colors, E, K, V = inputs
    d7, c7, E7 = scene.turned_away()
    m6 = new_map(lib, ctx, depths, colors, E, K, V)
    m6.prepare()
    m7 = new_map(lib, ctx, np.concatenate([depths, d7[None]]), np.concatenate([colors, c7[None]]), np.concatenate([E, E7[None]]), K, V)
    assert m7.prepare()[6] == 0
    for _ in range(2):
        rr6, n6 = m6.step()
        rr7, n7 = m7.step()
        assert n7[6] == 0 and rr7[6] == 0.0
        assert np.array_equal(bits(rr6), bits(rr7[:6])) and np.array_equal(n6, n7[:6])
    assert np.array_equal(bits(m7.extrinsics()[6]), bits(E7))
    assert np.array_equal(bits(m7.extrinsics()[:6]), bits(m6.extrinsics()))
    assert np.array_equal(bits(m7.colors()), bits(m6.colors()))
    m6.close(); m7.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 3])
def test_dilation_half_sizes(lib, ctx, golden, inputs, k):
    """test 8: the masks for half-sizes 0, 1 and 3"""
    depths, colors, E, K, V = inputs
    m = new_map(lib, ctx, depths[:2], colors[:2], E[:2], K, V[:300], half_dilation_kernel_size_for_discontinuity_map=k)
    m.prepare()
    for c in range(2):
        got = m.image(c, "mask")
        assert np.array_equal(got, S.depth_mask(depths[c], 0.1, k)) and np.array_equal(got, golden["mask_k%d" % k][c])
    m.close()


@pytest.mark.gpu
def test_a_list_longer_than_the_launch(lib, ctx, inputs):
    """test 9: three cameras, 600 000 vertices on the wall: a camera sees more than 512 x 256 of them, so the iteration
    kernel's grid-stride loop runs twice; one step's sums against the vectorised specification within the bound"""
    depths, colors, E, K, _ = inputs
    V = scene.vertices(n_wall=600000, n_floor=2000, n_sphere=2000, seed=9)
    pick = [0, 3, 4]
    st = S.State(V, depths[pick], colors[pick], E[pick], K, spec_option())
    m = new_map(lib, ctx, depths[pick], colors[pick], E[pick], K, V)
    counts = m.prepare()
    assert counts.max() > STRIDE_SHAPE
    assert all(np.array_equal(m.visible(c), st.lists[c]) for c in range(3))
    p = st.proxy()
    assert np.array_equal(bits(m.proxy()), bits(p))
    check_sums(m.sums(), st, p)
    m.close()


@pytest.mark.gpu
def test_seventy_cameras(lib, ctx, inputs):
    """test 10: 70 cameras cross the 32- and 64-camera words of the per-vertex bit matrix; 500 vertices"""
    _, _, _, K, V = inputs
    V = V[::6][:500].copy()
    poses = [scene.camera_to_world(i % 5) @ scene.rigid((0.0, 0.012 * (i // 5), 0.0), (0.01 * (i // 5), 0.0, 0.0)) for i in range(70)]
    frames = [scene.render_from(C_, i % 6) for i, C_ in enumerate(poses)]
    depths, colors = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    E = np.stack([scene.rigid(*scene._ERRORS[i % 6]) @ scene.invert_rigid(C_) for i, C_ in enumerate(poses)])
    st = S.State(V, depths, colors, E, K, spec_option())
    m = new_map(lib, ctx, depths, colors, E, K, V)
    counts = m.prepare()
    assert np.array_equal(counts, [len(x) for x in st.lists]) and (counts[64:] > 0).any() and (counts[32:64] > 0).any()
    assert all(np.array_equal(m.visible(c), st.lists[c]) for c in range(70))
    assert np.array_equal(bits(m.proxy()), bits(st.proxy()))
    assert np.abs(m.colors() - st.colours()).max() <= 1e-15
    m.close()


@pytest.mark.gpu
def test_argument_errors(lib, ctx, inputs):
    """test 11: INVALID for null pointers, a colour image that is not RGB8, an image index out of range and staged calls out
    of order; the object is usable afterwards"""
    depths, colors, E, K, V = inputs
    L, h = ctx.L, ctx._h
    n, hh, w = 2, depths.shape[1], depths.shape[2]
    m = ctx.color_map(w, hh, n, K, lib_option(lib))
    dp, fp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    d0, c0, e0 = depths[0].ctypes.data_as(fp), colors[0].ctypes.data_as(u8), np.ascontiguousarray(E[0]).ctypes.data_as(dp)
    buf = np.zeros(4 * len(V)); pb = buf.ctypes.data_as(dp)
    cnt = np.zeros(n, np.int64); pc = cnt.ctypes.data_as(C.POINTER(C.c_int64))
    si = L.visma_icp_color_map_set_image
    assert si(h, m._m, 0, None, c0, 3, e0) == INVALID and si(h, m._m, 0, d0, None, 3, e0) == INVALID and si(h, m._m, 0, d0, c0, 3, None) == INVALID
    assert si(h, m._m, 0, d0, c0, 1, e0) == INVALID and si(h, m._m, 0, d0, c0, 4, e0) == INVALID
    assert si(h, m._m, -1, d0, c0, 3, e0) == INVALID and si(h, m._m, n, d0, c0, 3, e0) == INVALID
    assert si(h, None, 0, d0, c0, 3, e0) == INVALID and si(None, m._m, 0, d0, c0, 3, e0) == INVALID
    assert L.visma_icp_color_map_set_vertices(h, m._m, None, 5) == INVALID and L.visma_icp_color_map_set_vertices(h, m._m, pb, 0) == INVALID
    # out of order: nothing is prepared, then an image is missing, then the vertices
    assert L.visma_icp_color_map_prepare(h, m._m, pc) == INVALID
    assert L.visma_icp_color_map_sums(h, m._m, pb) == INVALID and L.visma_icp_color_map_step(h, m._m, pb, pc) == INVALID
    assert L.visma_icp_color_map_run(h, m._m, 1, pb) == INVALID and L.visma_icp_color_map_get_proxy(h, m._m, pb, len(V)) == INVALID
    assert L.visma_icp_color_map_get_colors(h, m._m, pb, len(V)) == INVALID
    assert L.visma_icp_color_map_get_image(h, m._m, 0, 0, pb) == INVALID
    m.set_image(0, depths[0], colors[0], E[0])
    m.set_vertices(V)
    assert L.visma_icp_color_map_prepare(h, m._m, pc) == INVALID
    m.set_image(1, depths[1], colors[1], E[1])
    assert np.array_equal(m.prepare(), [233, 454])
    assert L.visma_icp_color_map_get_image(h, m._m, 2, 0, pb) == INVALID and L.visma_icp_color_map_get_image(h, m._m, 0, 4, pb) == INVALID
    assert L.visma_icp_color_map_get_image(h, m._m, 0, 0, None) == INVALID and L.visma_icp_color_map_sums(h, m._m, None) == INVALID
    assert L.visma_icp_color_map_get_proxy(h, m._m, pb, len(V) - 1) == INVALID
    m.set_image(1, depths[1], colors[1], E[1])                              # a new image asks for a new prepare
    assert L.visma_icp_color_map_step(h, m._m, pb, pc) == INVALID
    m.prepare()
    rr, count = m.step()
    assert count[0] > 6 and rr[0] > 0
    m.close()
    other = lib.Context(0)
    m2 = ctx.color_map(w, hh, 1, K, None)
    assert L.visma_icp_color_map_destroy(other._h, m2._m) == INVALID          # not a color map of that context
    other.close()
    m2.close()
