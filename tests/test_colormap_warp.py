"""The non-rigid color map optimization on the CPU: the numpy specification (tests/colormap_warp_spec.py) against the compiled
reference's fixture (tests/golden/colormap_warp.npz, tests/golden/gen_colormap_warp.py), the host-only banded solve
(visma_icp_color_map_solve_non_rigid) against numpy, the keep rules, and the argument checks of the new entry points.

Levels:
  exact     anchor shape, initial flow, the proxies under the initial field
  measured  poses and flows after 1, 2 and 8 iterations: 100 x the fixture's spreads (the largest distance among the compiled
            reference, the specification with sequential sums, with pairwise sums, and with the banded solve)
  colours   1e-15
  solve     |x - numpy's| <= 1e3 * 2^-53 * cond(JJ) * |x|_inf: the textbook backward-error bound of a stable solve, cond by numpy"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import colormap_warp_cases as cases
import colormap_warp_spec as WS
from oracle_engine import OracleEngine

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_colormap_solve  # noqa: E402

INVALID, STATE = 1, 5
ANCHORS = cases.ANCHORS
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def golden():
    return cases.golden()


@pytest.fixture(scope="module")
def inputs():
    return cases.inputs()


@pytest.fixture(scope="module")
def spec():
    return {a: cases.spec(a) for a in ANCHORS}


# ---- the specification against the fixture ------------------------------------------------------------------------------
@pytest.mark.parametrize("anchors", ANCHORS)
def test_specification_shape_flow_and_proxies_equal_the_reference(golden, spec, anchors):
    st, key = spec[anchors]["state"], "a%d_" % anchors
    assert (st.aw, st.ah) == tuple(golden[key + "shape"]) and st.anchor_step == float(golden[key + "step"])
    assert np.array_equal(st.flow_init, golden[key + "flow0"])
    assert np.array_equal(spec[anchors]["proxy0"], golden[key + "proxy0"])
    assert (st.aw, st.ah) == {5: (7, 5), 16: (22, 16)}[anchors]


@pytest.mark.parametrize("anchors", ANCHORS)
def test_specification_poses_flows_and_colours_equal_the_reference(golden, spec, anchors):
    s, key = spec[anchors], "a%d_" % anchors
    ptol, ftol = 100.0 * float(golden[key + "pose_spread"]), 100.0 * float(golden[key + "flow_spread"])
    for k in (1, 2, 8):
        dp, df = np.abs(s["E%d" % k] - golden[key + "extr_%d" % k]).max(), np.abs(s["F%d" % k] - golden[key + "flow_%d" % k]).max()
        print("anchors %d after %d: pose %.3g (tol %.3g), flow %.3g (tol %.3g)" % (anchors, k, dp, ptol, df, ftol))
        assert dp <= ptol and df <= ftol
    assert np.abs(s["colors0"] - golden[key + "colors_0"]).max() <= 1e-15
    assert np.abs(s["colors8"] - golden[key + "colors_8"]).max() <= 1e-15
    rr = np.array([h[0].sum() for h in s["hist"]]); reg = np.array([h[1].sum() for h in s["hist"]])
    assert np.allclose(rr, golden[key + "rr"], rtol=1e-9, atol=0) and np.allclose(reg, golden[key + "rr_reg"], rtol=1e-7, atol=1e-18)
    assert np.abs(golden[key + "flow_8"] - golden[key + "flow0"]).max() > 0.1                  # the fields did move


def test_the_fixture_says_the_fields_absorb_the_distortion(golden):
    assert float(golden["dist_non_rigid_8"]) < float(golden["dist_rigid_8"])


# ---- the host-only solve ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchors", ANCHORS)
def test_banded_solve_against_numpy(lib, golden, spec, inputs, anchors):
    """every camera of the fixture case at iteration 1, and at flows moved off their anchors (the regulariser's right side)"""
    st = spec[anchors]["state"]
    rows = spec[anchors]["rows"][0]
    nv = len(inputs[4])
    w = float(golden["a%d_weight" % anchors])
    rng = np.random.default_rng(3)
    seen = 0
    for c in range(len(rows)):
        for flow in (st.flow_init, st.flow_init + rng.normal(0, 0.5, len(st.flow_init))):
            JJ, Jb, _, reg, count = WS.assemble(st.aw, st.ah, rows[c], nv, w, flow, st.flow_init)
            x, reg_lib, kept = lib.color_map_solve_non_rigid(st.aw, st.ah, rows[c], nv, w, flow, st.flow_init)
            assert not kept and count >= 6
            want = np.linalg.solve(JJ, -Jb)
            cond = np.linalg.cond(JJ)
            bound = 1e3 * 2.0 ** -53 * cond * np.abs(want).max()
            err = np.abs(x - want).max()
            print("anchors %d camera %d: cond %.3g, error %.3g, bound %.3g" % (anchors, c, cond, err, bound))
            assert err <= bound
            assert abs(reg_lib - reg) <= 1e-12 * max(reg, 1e-300)
            seen += 1
    assert seen == 2 * len(rows)


def one_cell_rows(aw, ah, cell, n, seed=0):
    """cell rows with n synthetic visits in one cell"""
    rng = np.random.default_rng(seed)
    R = np.concatenate([rng.normal(size=(n, 15)), np.ones((n, 1))], 1)
    rows = np.zeros(((aw - 1) * (ah - 1), WS.ROW))
    rows[cell] = np.stack([R[:, x] * R[:, y] for x, y in WS.PAIRS], 1).sum(axis=0)
    return rows


def test_keep_rules(lib):
    aw, ah = 4, 3
    f0 = WS.initial_flow(aw, ah, 10.0)
    zero = np.zeros(6 + 2 * aw * ah)
    # weight 0 and anchors no visit touches: their pivots are 0
    x, reg, kept = lib.color_map_solve_non_rigid(aw, ah, one_cell_rows(aw, ah, 0, 40), 100, 0.0, f0 + 1.0, f0)
    assert kept and np.array_equal(x, zero) and reg == 0.0
    # ... the same rows with a weight: solved
    x, reg, kept = lib.color_map_solve_non_rigid(aw, ah, one_cell_rows(aw, ah, 0, 40), 100, 0.5, f0 + 1.0, f0)
    assert not kept and np.all(np.isfinite(x)) and x.any()
    assert reg == pytest.approx(((0.5 * 40 / 100) ** 2) * len(f0), rel=1e-12)
    # fewer than 6 visits, and none
    for n in (1, 5):
        x, reg, kept = lib.color_map_solve_non_rigid(aw, ah, one_cell_rows(aw, ah, 1, n), 100, 0.5, f0, f0)
        assert kept and np.array_equal(x, zero)
    x, reg, kept = lib.color_map_solve_non_rigid(aw, ah, np.zeros(((aw - 1) * (ah - 1), WS.ROW)), 100, 0.5, f0 + 1.0, f0)
    assert kept and np.array_equal(x, zero) and reg == 0.0
    x, reg, kept = lib.color_map_solve_non_rigid(aw, ah, one_cell_rows(aw, ah, 1, 6), 100, 0.5, f0, f0)
    assert not kept
    # a NaN row: in a sum, and in the count
    for at in (3, 110, 120):
        rows = one_cell_rows(aw, ah, 2, 40)
        rows[2, at] = np.nan
        x, reg, kept = lib.color_map_solve_non_rigid(aw, ah, rows, 100, 0.5, f0, f0)
        assert kept and np.array_equal(x, zero), at
    # the specification keeps where the library keeps
    assert WS.solve_dense(aw, ah, one_cell_rows(aw, ah, 0, 40), 100, 0.0, f0 + 1.0, f0)[2]
    assert WS.solve_dense(aw, ah, one_cell_rows(aw, ah, 1, 5), 100, 0.5, f0, f0)[2]


def test_assembly_and_solve_under_the_sanitizers():
    """tests/cpp/colormap_solve_driver.cpp: the host-only assembly and solve on 2 x 2 and 128 x 64 anchors, empty rows, the
    keep cases, a count of INT_MAX, 1 / 16 / 64 threads, compiled with -fsanitize=address,undefined"""
    exe = build_colormap_solve.build()[0]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "all passed" in p.stdout and "FAILED" not in p.stdout and "runtime error" not in p.stderr, (p.stdout, p.stderr)
    assert p.stdout.count(": ok") == 15


def test_solve_argument_checks(lib):
    L = lib.load()
    aw, ah = 4, 3
    f0 = WS.initial_flow(aw, ah, 10.0)
    rows, x = one_cell_rows(aw, ah, 0, 10), np.zeros(6 + 2 * aw * ah)
    p = lambda a: a.ctypes.data_as(_dp)

    def call(aw=aw, ah=ah, rows=p(rows), nv=100, w=0.5, f=p(f0), g=p(f0), xx=p(x)):
        return L.visma_icp_color_map_solve_non_rigid(aw, ah, rows, nv, w, f, g, xx, None, None)

    assert call() == 0
    assert call(aw=1) == INVALID and call(ah=1) == INVALID and call(aw=128, ah=65) == INVALID
    assert call(rows=None) == INVALID and call(f=None) == INVALID and call(g=None) == INVALID and call(xx=None) == INVALID
    assert call(nv=0) == INVALID and call(w=float("nan")) == INVALID and call(w=-1.0) == INVALID and call(w=float("inf")) == INVALID


# ---- the new entry points' checks come before the device ------------------------------------------------------------------
@pytest.fixture()
def hctx(lib, oracle):
    eng = OracleEngine(oracle)
    ctx = eng.context()
    ctx.engine = eng
    yield ctx
    ctx.close()


def test_create_non_rigid_checks_come_before_the_device(lib, hctx):
    """on the oracle engine a create that passes its checks ends at "not supported" (VISMA_ICP_ERR_STATE)"""
    L, h = hctx.L, hctx._h
    m = C.c_void_p()
    k = np.array([70.0, 70.0, 41.0, 30.0]); pk = k.ctypes.data_as(_dp)

    def create(w=83, hh=61, n=2, intr=pk, option=None, out=C.byref(m), ctx=h):
        return L.visma_icp_color_map_create_non_rigid(ctx, w, hh, n, intr, None if option is None else C.byref(option), out)

    assert create() == STATE
    assert create(option=lib.color_map_option(non_rigid_camera_coordinate=1)) == STATE        # the flag is not read
    assert create(option=lib.color_map_option(non_rigid_camera_coordinate=0, number_of_vertical_anchors=2)) == STATE
    assert create(option=lib.color_map_option(number_of_vertical_anchors=64)) == STATE
    assert create(ctx=None) == INVALID and create(out=None) == INVALID and create(intr=None) == INVALID
    assert create(n=0) == INVALID and create(w=20) == INVALID and create(hh=20) == INVALID
    assert create(option=lib.color_map_option(number_of_vertical_anchors=1)) == INVALID
    assert create(option=lib.color_map_option(number_of_vertical_anchors=65)) == INVALID
    assert create(option=lib.color_map_option(number_of_vertical_anchors=0)) == INVALID
    # 64 vertical anchors on an image 4 times as wide as high: 64 * 254 anchors
    assert create(w=400, hh=100, option=lib.color_map_option(number_of_vertical_anchors=64)) == INVALID
    assert create(w=200, hh=100, option=lib.color_map_option(number_of_vertical_anchors=64)) == STATE     # 64 * 127 = 8128
    assert create(option=lib.color_map_option(non_rigid_anchor_point_weight=float("nan"))) == INVALID
    assert create(option=lib.color_map_option(non_rigid_anchor_point_weight=-0.5)) == INVALID
    assert create(option=lib.color_map_option(non_rigid_anchor_point_weight=float("inf"))) == INVALID
    assert create(option=lib.color_map_option(non_rigid_anchor_point_weight=0.0)) == STATE
    assert create(option=lib.color_map_option(half_dilation_kernel_size_for_discontinuity_map=-1)) == INVALID
    # the old entry points still refuse the flag, and say where to go
    assert L.visma_icp_color_map_create(h, 83, 61, 2, pk, C.byref(lib.color_map_option(non_rigid_camera_coordinate=1)), C.byref(m)) == INVALID
    assert b"visma_icp_color_map_create_non_rigid" in L.visma_icp_last_error(h)
    z = np.zeros(16)
    pz = z.ctypes.data_as(_dp)
    rc = L.visma_icp_color_map_optimization_non_rigid(h, 83, 61, 1, pk, np.zeros(83 * 61, np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                                                      np.zeros(83 * 61 * 3, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), pz, pz, 1,
                                                      C.byref(lib.color_map_option(number_of_vertical_anchors=1)), pz, None)
    assert rc == INVALID and not z.any()
    for name in ("get_flow", "set_flow", "cell_sums"):
        assert getattr(L, "visma_icp_color_map_" + name)(h, None, pz) == INVALID
    assert L.visma_icp_color_map_get_anchor_shape(h, None, None, None, None) == INVALID
    assert L.visma_icp_color_map_step_non_rigid(h, None, pz, pz, None) == INVALID


def test_python_surface(lib):
    for name in ("color_map_non_rigid", "color_map_optimization_non_rigid"):
        assert callable(getattr(lib.Context, name, None)), name
    for name in ("anchor_shape", "flow", "set_flow", "cell_sums", "step_non_rigid"):
        assert callable(getattr(lib.ColorMap, name, None)), name
    assert callable(lib.color_map_solve_non_rigid) and lib.COLOR_MAP_CELL_SUMS == 121
