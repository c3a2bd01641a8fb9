"""The non-rigid color map optimization on the GPU (visma_icp_color_map_create_non_rigid and what follows it;
colormap_warp.hip) against the numpy specification tests/colormap_warp_spec.py, which tests/test_colormap_warp.py pins to the
compiled reference.  Levels:
  exact     anchor shape, initial flow, proxies, colours under the initial field; the counts; a camera that keeps
  bounded   a cell's 121 sums: K 2^-53 sum|term| per sum, K the cell's count (colormap_spec.sum_bound)
  measured  poses and flows after 1, 2 and 8 iterations: 100 x the fixture's spreads
  colours   after 8 iterations: 1e-15
  histories rr and rr_reg of iteration k: the sum bound alone.  The specification is evaluated at the LIBRARY's own state
            before that step (its extrinsics and flows put into a colormap_warp_spec.State), so nothing but the order of the
            additions differs: rr within the cells' K 2^-53 sum|term| plus cells x 2^-53 |rr| for the sum over the cells;
            rr_reg, a sum of 2 aw ah identical squares in two orders, within 2 aw ah 2^-53 rr_reg
The small shapes: 32 x 24 images of tests/colormap_scene.py's hostile kind (cameras without rotation, vertices on z = 1, the
margin leaves u in [10, 22), v in [10, 14)).  With 2 vertical anchors (step 24) every accepted visit is in cell 0; with 3
(step 12) they spread over four cells.  The sort's tile is 1024 visits."""
import numpy as np
import pytest

import colormap_scene as hostile
import colormap_spec as S
import colormap_warp_cases as cases
import colormap_warp_scene as scene
import colormap_warp_spec as WS

pytestmark = pytest.mark.gpu
ANCHORS = cases.ANCHORS
TILE = 1024


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def new_map(lib, ctx, depths, colors, E, K, V, option):
    n, h, w = depths.shape
    m = ctx.color_map_non_rigid(w, h, n, K, lib.color_map_option(**{k: v for k, v in option.items() if k != "non_rigid_camera_coordinate"}))
    for i in range(n):
        m.set_image(i, depths[i], colors[i], E[i])
    m.set_vertices(V)
    return m


def check_cell_sums(got, want, bound):
    """n x cells x 121 against the specification's within the bound; the counts equal"""
    assert got.shape == want.shape
    assert np.array_equal(got[:, :, 120], want[:, :, 120])
    err = np.abs(got - want)
    print("cells with visits: %d of %d; worst error / bound %.3g" % ((want[:, :, 120] > 0).sum(), want[:, :, 120].size,
                                                                       np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)


# ---------------------------------------------------------------------------
# the fixture cases
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=ANCHORS)
def fixture_run(request, lib, ctx):
    """the library on the fixture case: the initial state, the rows of iteration 1, the states after 1, 2 and 8, the histories"""
    a = request.param
    depths, colors, E, K, V = cases.inputs()
    m = new_map(lib, ctx, depths, colors, E, K, V, cases.spec_option(a))
    counts = m.prepare()
    o = dict(anchors=a, counts=counts, shape=m.anchor_shape(), flow0=m.flow(), proxy0=m.proxy(), colors0=m.colors(), rows0=m.cell_sums(),
             hist=[])
    assert np.array_equal(m.flow(), o["flow0"]) and np.array_equal(m.extrinsics(), E)          # cell_sums moved nothing
    o["before"] = []
    for k in range(1, 9):
        o["before"].append((m.extrinsics(), m.flow()))
        o["hist"].append(m.step_non_rigid())
        if k in (1, 2, 8):
            o["E%d" % k], o["F%d" % k] = m.extrinsics(), m.flow()
    o["colors8"] = m.colors()
    m.close()
    return o


def test_fixture_shape_flow_proxies_colours_bit_for_bit(fixture_run):
    a = fixture_run["anchors"]
    g, s, key = cases.golden(), cases.spec(a), "a%d_" % a
    assert fixture_run["shape"] == (int(g[key + "shape"][0]), int(g[key + "shape"][1]), float(g[key + "step"]))
    assert np.array_equal(bits(fixture_run["flow0"]), bits(np.tile(g[key + "flow0"], (len(fixture_run["counts"]), 1))))
    assert np.array_equal(bits(fixture_run["proxy0"]), bits(g[key + "proxy0"]))
    assert np.array_equal(bits(fixture_run["colors0"]), bits(s["colors0"]))
    assert np.abs(fixture_run["colors0"] - g[key + "colors_0"]).max() <= 1e-15
    assert np.array_equal(fixture_run["counts"], [len(x) for x in s["state"].lists])


def test_fixture_cell_sums_within_the_bound(fixture_run):
    s = cases.spec(fixture_run["anchors"])
    check_cell_sums(fixture_run["rows0"], s["rows"][0], s["bounds"][0])


def test_fixture_poses_flows_colours_and_histories(fixture_run):
    a = fixture_run["anchors"]
    g, s, key = cases.golden(), cases.spec(a), "a%d_" % a
    ptol, ftol = 100.0 * float(g[key + "pose_spread"]), 100.0 * float(g[key + "flow_spread"])
    for k in (1, 2, 8):
        dp, df = np.abs(fixture_run["E%d" % k] - g[key + "extr_%d" % k]).max(), np.abs(fixture_run["F%d" % k] - g[key + "flow_%d" % k]).max()
        print("anchors %d after %d: pose %.3g (tol %.3g), flow %.3g (tol %.3g)" % (a, k, dp, ptol, df, ftol))
        assert dp <= ptol and df <= ftol
    assert np.abs(fixture_run["colors8"] - g[key + "colors_8"]).max() <= 1e-15
    depths, colors, E, K, V = cases.inputs()
    st = WS.State(V, depths, colors, E, K, cases.spec_option(a))             # (visibility is that of the initial poses)
    nv, w = len(V), float(g[key + "weight"])
    for k in range(8):
        rr, reg, count = fixture_run["hist"][k]
        st.E, st.flows = fixture_run["before"][k][0].copy(), fixture_run["before"][k][1].copy()
        rows, bounds = st.cell_sums()
        n_cells = rows.shape[1]
        assert np.array_equal(count, rows[:, :, 120].sum(axis=1).astype(np.int64)), k
        for c in range(len(rr)):
            srr = rows[c][:, 119].sum()
            b_rr = bounds[c][:, 119].sum() + n_cells * S.U * abs(srr)
            r = (w * count[c] / nv) * (st.flows[c] - st.flow_init)
            sreg = float((r * r).sum()) if count[c] > 0 else 0.0
            b_reg = len(r) * S.U * sreg
            print("iteration %d camera %d: rr %.3g off (bound %.3g), rr_reg %.3g off (bound %.3g)" %
                  (k + 1, c, abs(rr[c] - srr), b_rr, abs(reg[c] - sreg), b_reg))
            assert abs(rr[c] - srr) <= b_rr and abs(reg[c] - sreg) <= b_reg


def test_one_call_entry_equals_the_staged_calls(lib, ctx, fixture_run):
    a = fixture_run["anchors"]
    depths, colors, E, K, V = cases.inputs()
    o = cases.spec_option(a, maximum_iteration=8.0)
    E8, colours, flows = ctx.color_map_optimization_non_rigid(V, depths, colors, K, E, lib.color_map_option(
        **{k: v for k, v in o.items() if k != "non_rigid_camera_coordinate"}))
    assert np.array_equal(bits(E8), bits(fixture_run["E8"])) and np.array_equal(bits(flows), bits(fixture_run["F8"]))
    assert np.array_equal(bits(colours), bits(fixture_run["colors8"]))


def test_run_reports_the_data_residual_and_handles_are_told_apart(lib, ctx):
    depths, colors, E, K, V = cases.inputs()
    o = cases.spec_option(5)
    m = new_map(lib, ctx, depths, colors, E, K, V, o)
    m.prepare()
    res = m.run(2)
    s = cases.spec(5)
    assert np.allclose(res, [s["hist"][k][0].sum() for k in range(2)], rtol=1e-9, atol=0)
    with pytest.raises(lib.IcpError) as e:
        m.sums()
    assert e.value.code == 1
    m.close()
    r = ctx.color_map(83, 61, len(E), K, lib.color_map_option(maximum_allowable_depth=o["maximum_allowable_depth"]))
    for call in (r.anchor_shape, r.step_non_rigid):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == 1
    z = np.zeros(4)
    for name in ("get_flow", "set_flow", "cell_sums"):                         # (the methods ask for the shape first)
        assert getattr(ctx.L, "visma_icp_color_map_" + name)(ctx._h, r._m, z.ctypes.data_as(lib._dp)) == 1
    r.close()


# ---------------------------------------------------------------------------
# the distorted scene
# ---------------------------------------------------------------------------
def test_the_fields_absorb_what_no_pose_explains(lib, ctx):
    depths, colors, E, K = scene.distorted_frames()
    V = scene.vertices()
    o = cases.spec_option(16)
    m = new_map(lib, ctx, depths, colors, E, K, V, o)
    m.prepare()
    non_rigid = m.run(9)
    m.close()
    r = ctx.color_map(scene.W, scene.H, len(E), K, lib.color_map_option(maximum_allowable_depth=o["maximum_allowable_depth"]))
    for i in range(len(E)):
        r.set_image(i, depths[i], colors[i], E[i])
    r.set_vertices(V)
    r.prepare()
    rigid = r.run(9)
    r.close()
    g = cases.golden()
    print("data residual of the state after 8 iterations: rigid %.6f, non-rigid %.6f (the reference: %.6f, %.6f)" %
          (rigid[8], non_rigid[8], float(g["dist_rigid_8"]), float(g["dist_non_rigid_8"])))
    assert non_rigid[8] < rigid[8]


# ---------------------------------------------------------------------------
# repeatability
# ---------------------------------------------------------------------------
def test_a_run_is_bit_identical_to_itself(lib, ctx):
    depths, colors, E, K, V = cases.inputs()
    out = []
    for _ in range(2):
        m = new_map(lib, ctx, depths, colors, E, K, V, cases.spec_option(16))
        m.prepare()
        rows = m.cell_sums()
        m.run(8)
        out.append((rows, m.flow(), m.extrinsics(), m.cell_sums()))
        m.close()
    for a, b in zip(*out):
        assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------
# small shapes, each against the specification
# ---------------------------------------------------------------------------
def plane_case(n_vertices, n_cameras, seed=1, inside=False):
    """32 x 24, cameras without rotation a fraction of a pixel apart, depth 1, vertices on z = 1 at random pixels of
    [8, 24) x [8, 16) (inside: of the margin's interior [10.5, 21.5) x [10.5, 13.5)) -> depths, colors, E, K, V"""
    rng = np.random.default_rng(seed)
    shift = [((c % 5 - 2) / 16.0, (c // 5 % 5 - 2) / 16.0) for c in range(n_cameras)]
    depths = np.ones((n_cameras, hostile.HH, hostile.HW), np.float32)
    colors = np.stack([hostile.pattern(du + hostile.pose_error(c)[0], dv + hostile.pose_error(c)[1]) for c, (du, dv) in enumerate(shift)])
    E = np.stack([hostile.shifted(du, dv) for du, dv in shift])
    lo, hi = ((10.5, 10.5), (21.5, 13.5)) if inside else ((8.0, 8.0), (24.0, 16.0))
    uv = rng.uniform(lo, hi, (n_vertices, 2))
    V = np.ascontiguousarray(np.stack([hostile.at_pixel(u, v) for u, v in uv]))
    return depths, colors, E, hostile.HK.copy(), V


def small_option(anchors, **kw):
    o = S.default_option()
    o.update(number_of_vertical_anchors=anchors, half_dilation_kernel_size_for_discontinuity_map=0, **kw)
    return o


def against_spec(lib, ctx, case, option, after_prepare=None):
    """proxies and colours bit for bit, cell sums within the bound, and one step: the counts, rr within the bound, the flows
    exactly flow + x[6:] of the library's own host solve on the library's rows, the poses of that x"""
    depths, colors, E, K, V = case
    st = WS.State(V, depths, colors, E, K, option)
    m = new_map(lib, ctx, depths, colors, E, K, V, option)
    counts = m.prepare()
    assert np.array_equal(counts, [len(x) for x in st.lists])
    assert m.anchor_shape() == (st.aw, st.ah, st.anchor_step)
    if after_prepare is not None:
        after_prepare(m, st)
    assert np.array_equal(bits(m.proxy()), bits(st.proxy()))
    assert np.array_equal(bits(m.colors()), bits(st.colours()))
    want, bound = st.cell_sums()
    rows = m.cell_sums()
    check_cell_sums(rows, want, bound)
    E0, F0 = m.extrinsics(), m.flow()
    rr, reg, count = m.step_non_rigid()
    assert np.array_equal(count, want[:, :, 120].sum(axis=1).astype(np.int64))
    assert np.all(np.abs(rr - want[:, :, 119].sum(axis=1)) <= bound[:, :, 119].sum(axis=1) + want.shape[1] * S.U * np.abs(rr))
    E1, F1 = m.extrinsics(), m.flow()
    kept = []
    for c in range(len(E)):
        x, reg_c, keep = lib.color_map_solve_non_rigid(st.aw, st.ah, rows[c], len(V), option["non_rigid_anchor_point_weight"], F0[c], st.flow_init)
        kept.append(keep)
        assert reg_c == reg[c]
        if keep:
            assert np.array_equal(bits(E1[c]), bits(E0[c])) and np.array_equal(bits(F1[c]), bits(F0[c])), c
        else:
            assert np.array_equal(bits(F1[c]), bits(F0[c] + x[6:])), c
            assert np.abs(E1[c] - WS.pose_update(x) @ E0[c]).max() <= 1e-14 * max(1.0, np.abs(E0[c]).max()), c
    m.close()
    return st, want, np.array(kept), count


def test_smallest_images_with_two_anchors(lib, ctx):
    depths, colors, E, K, V, extra = hostile.seam_case(n_vertices=40, n_cameras=2, half_dilation=0)
    st, want, kept, count = against_spec(lib, ctx, (depths, colors, E, K, V), small_option(2))
    assert (st.aw, st.ah) == (2, 2) and want.shape[1] == 1 and count.sum() > 0


@pytest.mark.parametrize("n_vertices", [1, 255, 256, 257, TILE + 1])
def test_vertex_counts_around_the_tiles(lib, ctx, n_vertices):
    st, want, kept, count = against_spec(lib, ctx, plane_case(n_vertices, 2, seed=n_vertices), small_option(3))
    assert (st.aw, st.ah) == (4, 3)
    if n_vertices >= 255:
        assert (want[:, :, 120] > 0).sum(axis=1).min() >= 4 and count.min() < n_vertices       # four cells, and the margin rejects


@pytest.mark.parametrize("n_cameras", [1, 33])
def test_camera_counts(lib, ctx, n_cameras):
    st, want, kept, count = against_spec(lib, ctx, plane_case(300, n_cameras, seed=7), small_option(3))
    assert len(count) == n_cameras and count.min() > 6


@pytest.mark.parametrize("n_vertices", [64, 65, 2 * TILE + 5])
def test_every_visit_in_one_cell(lib, ctx, n_vertices):
    """2 anchors: step 24, and the margin's interior lies in cell 0"""
    st, want, kept, count = against_spec(lib, ctx, plane_case(n_vertices, 2, seed=n_vertices, inside=True), small_option(2))
    assert want.shape[1] == 2 and np.all(want[:, 0, 120] == n_vertices) and np.all(want[:, 1, 120] == 0)


def test_cameras_with_no_and_with_few_visits_keep_bit_for_bit(lib, ctx):
    depths, colors, E, K, V, extra = hostile.keep_pose_case()
    depths = np.concatenate([depths, np.zeros_like(depths[:1])])               # a last camera that sees nothing
    colors, E = np.concatenate([colors, colors[:1]]), np.concatenate([E, E[:1]])
    st, want, kept, count = against_spec(lib, ctx, (depths, colors, E, K, V), small_option(3, **extra))
    few = slice(hostile.KEEP_NORMAL, hostile.KEEP_NORMAL + 5)
    assert list(count[few]) == [1, 2, 3, 4, 5] and kept[few].all()
    assert count[-1] == 0 and kept[-1]
    assert kept[hostile.KEEP_CONSTANT]                                         # constant images: the pose's block is zero
    assert not kept[:hostile.KEEP_NORMAL].any()


def test_a_field_pushed_out_of_the_margin(lib, ctx):
    def push(m, st):
        st.flows = st.flows + 100.0
        m.set_flow(st.flows)
        assert np.array_equal(m.flow(), st.flows)

    st, want, kept, count = against_spec(lib, ctx, plane_case(300, 2, seed=3), small_option(3), push)
    assert count.sum() == 0 and kept.all() and not st.proxy().any()


def test_poses_moved_after_prepare(lib, ctx):
    """camera 0: a vertex at its centre (every other vertex then has z == 0); camera 1: 14 pixels to the left with the field
    pushed 14 pixels right: u < 0 inside cell 0 is kept with p < 0; camera 2: 30 pixels right, u >= w; camera 3: 40 pixels
    left, u <= -step; camera 4 stays"""
    case = plane_case(400, 5, seed=11)
    info = []

    def move(m, st):
        E = st.E.copy()
        E[0] = np.eye(4); E[0][:3, 3] = -st.V[st.lists[0][0]]
        E[1][0, 3] -= 14.0 / 16.0
        E[2][0, 3] += 30.0 / 16.0
        E[3][0, 3] -= 40.0 / 16.0
        st.E = E
        st.flows[1, 0::2] += 14.0
        m.set_extrinsics(E)
        m.set_flow(st.flows)
        st.info = info

    st, want, kept, count = against_spec(lib, ctx, case, small_option(3), move)
    by_camera = info[:5]                                                       # (the first cell_sums of the specification)
    print(by_camera, count)
    assert count[0] == 0 and by_camera[0]["skipped"] == len(st.lists[0])
    assert by_camera[1]["negative_p"] > 0 and count[1] > 0
    assert by_camera[2]["skipped"] > 0 and by_camera[3]["skipped"] > 0
    assert count[4] > 6 and not kept[4]
