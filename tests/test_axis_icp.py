"""Registrations with the rotation constrained to one axis (visma_icp_set_rotation_axis): the whole loop -- host loop,
device loop, persistent launches, the ring search, batches, yaw sweeps, the corpus -- against a Python loop of the
reference's nearest neighbours (or the library's own passes) and numpy's 4-DoF solves."""
import numpy as np
import pytest

from visma_amd import _lib, synth
from test_axis_solve import rot, restated

Y = np.array([0.0, 1.0, 0.0])
GENERAL = np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])


def yaw_pair(axis, ns=5000, nt=20000):
    """target = S-surf, source = T_gt^-1 target-surface sample, T_gt = rotation by 0.3 about `axis` + a translation"""
    tgt = synth.surface_points(nt, 1234)
    src = synth.surface_points(ns, 5678)
    T_gt = np.eye(4)
    T_gt[:3, :3] = rot(axis, 0.3)
    T_gt[:3, 3] = [0.02, -0.01, 0.015]
    Ti = np.linalg.inv(T_gt)
    src = src @ Ti[:3, :3].T + Ti[:3, 3]
    return src.astype(np.float32).astype(np.float64), tgt.astype(np.float32).astype(np.float64), T_gt


def tilt_deg(T, axis=Y):
    """angle between R^T a and a"""
    v = np.asarray(T)[:3, :3].T @ axis
    return float(np.degrees(np.arccos(np.clip(v @ axis, -1.0, 1.0))))


def upright_err(T, axis=Y):
    return float(np.abs(np.asarray(T)[:3, :3].T @ axis - axis).max())


def python_loop(src, tgt, r, axis, nn, iters=20):
    """O3D's loop (Registration.cpp:166-184) without a stop test: nn(T) -> correspondence index, numpy 4-DoF solve"""
    T = np.eye(4)
    idx = nn(T)
    for _ in range(iters):
        m = idx >= 0
        p = src[m] @ T[:3, :3].T + T[:3, 3]
        upd, _ = restated(p, tgt[idx[m]], axis)
        T = upd @ T
        idx = nn(T)
    return T, int((idx >= 0).sum())


def ctx_with(src, tgt, axis=Y, device_loop=None, persistent=True, ring=None):
    c = _lib.Context(0)
    if ring is not None:
        c.set_ring_search(ring)
    c.set_device_loop(device_loop)
    c.set_persistent(persistent)
    c.set_clouds_f64(src, tgt)
    c.set_rotation_axis(axis)
    return c


def _check_against(res, T_py, k_py):
    assert res.num_correspondences == k_py
    assert np.abs(res.transformation_ - T_py).max() < 1e-9, np.abs(res.transformation_ - T_py).max()


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [Y, GENERAL], ids=["y", "general"])
def test_loop_equals_python_loop_over_the_reference_kd_tree(lib, ref, axis):
    src, tgt, _ = yaw_pair(axis)
    r = synth.default_radius(len(tgt))
    T_py, k_py = python_loop(src, tgt, r, axis, lambda T: ref.evaluate_registration(src, tgt, r, T).idx)
    c = ctx_with(src, tgt, axis)
    res = c.run(None, r, 20, 0.0, 0.0)
    assert res.iterations == 20
    _check_against(res, T_py, k_py)
    assert upright_err(res.transformation_, axis) < 1e-12
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [Y, GENERAL], ids=["y", "general"])
def test_loop_equals_python_loop_over_the_oracle_grid(lib, oracle, axis):
    src, tgt, _ = yaw_pair(axis)
    r = synth.default_radius(len(tgt))

    def nn(T):
        return oracle.nn_pass(src @ T[:3, :3].T + T[:3, 3], tgt, r, grid=True)[1]
    T_py, k_py = python_loop(src, tgt, r, axis, nn)
    c = ctx_with(src, tgt, axis)
    res = c.run(None, r, 20, 0.0, 0.0)
    _check_against(res, T_py, k_py)
    c.close()


@pytest.mark.gpu
def test_loop_flavours_agree(lib):
    """host loop, device loop, persistent launch on / off, ring search forced on / off: the same registration"""
    src, tgt, _, _ = synth.make_pair(16384, 65536, motion="fixed")
    out = {}
    for name, kw in [("host", dict(device_loop=False)), ("host, no persistent", dict(device_loop=False, persistent=False)),
                     ("device", dict(device_loop=True)), ("host, ring", dict(device_loop=False, ring=1)),
                     ("host, no ring", dict(device_loop=False, ring=0)), ("device, ring", dict(device_loop=True, ring=1))]:
        c = ctx_with(src, tgt, Y, **kw)
        c.set_nn_mode(lib.NN_GRID)
        out[name] = c.run(None, 0.15, 30)
        if kw.get("ring") == 1:
            assert c.search_kernel_used() == "ring", name
        c.close()
    a = out["host"]
    assert upright_err(a.transformation_) < 1e-12
    for name, b in out.items():
        assert b.num_correspondences == a.num_correspondences, name
        assert b.iterations == a.iterations, name
        assert np.abs(b.transformation_ - a.transformation_).max() < 1e-11, (name, np.abs(b.transformation_ - a.transformation_).max())


def c3():
    import bench
    return bench.c3_problems()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_c3_batch_is_upright_and_equals_single_runs(lib):
    objs, probs = c3()
    batch = [p[:4] for p in probs]
    c = _lib.Context(0)
    free = c.run_batch(batch, 30)                                  # unconstrained: make_pair's 1 degree tilt shows
    assert max(tilt_deg(r.transformation_) for r in free) > 0.5
    c.set_rotation_axis(Y)
    got = c.run_batch(batch, 30)
    assert len(got) == 288
    assert max(upright_err(r.transformation_) for r in got) < 1e-12
    info = c.sweep_info()
    assert info["aborts"] == 0, info
    w = [_lib.Context(0) for _ in range(2)]
    for x in w:
        x.set_rotation_axis(Y)
    multi = _lib.run_batch_multi(w, batch, 30)
    for i in range(288):
        assert multi[i].num_correspondences == got[i].num_correspondences, i
        assert np.array_equal(multi[i].transformation_, got[i].transformation_), i
    one = _lib.Context(0)
    one.set_rotation_axis(Y)
    for oi in (0, 5, 11):
        src, tgt = objs[oi]
        one.set_clouds_f64(src, tgt)
        for k in range(24):
            i = oi * 24 + k
            r1 = one.run(probs[i][2], 0.02, 30)
            assert r1.num_correspondences == got[i].num_correspondences, i
            assert r1.iterations == got[i].iterations, i
            assert synth.rel_frobenius(got[i].transformation_, r1.transformation_) < 1e-9, i
    for x in [c, one] + w:
        x.close()


@pytest.mark.gpu
def test_yaw_sweeps_are_upright_and_best_equals_a_single_run(lib):
    src, tgt, _, _ = synth.make_pair(4000, 12000)
    r = synth.default_radius(len(tgt))
    c = ctx_with(src, tgt)
    best, bl, per = c.run_yaw_sweep(24, r, 30)
    assert all(upright_err(p.transformation_) < 1e-12 for p in per)
    info = c.sweep_info()
    assert info["aborts"] == 0, info
    one = ctx_with(src, tgt, device_loop=False)
    init = synth.make_T(synth.rot_y(2 * np.pi * bl / 24), [0, 0, 0])
    r1 = one.run(init, r, 30)
    assert r1.num_correspondences == best.num_correspondences
    assert synth.rel_frobenius(best.transformation_, r1.transformation_) < 1e-9
    # point-to-plane
    tgt, nrm = _ellipsoid(12000, 7, noise=2e-4)
    src, _ = _ellipsoid(4000, 8)
    for x in (c, one):
        x.set_clouds_f64(src, tgt)
        x.set_target_normals_f64(nrm)
    best, bl, per = c.run_yaw_sweep_point_to_plane(24, 0.03, 30)
    assert all(upright_err(p.transformation_) < 1e-12 for p in per)
    init = synth.make_T(synth.rot_y(2 * np.pi * bl / 24), [0, 0, 0])
    r1 = one.run_point_to_plane(init, 0.03, 30)
    assert r1.num_correspondences == best.num_correspondences
    assert synth.rel_frobenius(best.transformation_, r1.transformation_) < 1e-9
    c.close()
    one.close()


def _ellipsoid(n, seed, axes=(0.5, 0.3, 0.2), centre=(0.3, -0.2, 1.0), noise=0.0):
    """points on an ellipsoid with three different axes and their exact unit normals (as tests/test_c3_batch.py)"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = np.asarray(axes)
    p = u * a
    nrm = p / a ** 2
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = p + rng.normal(size=p.shape) * noise + np.asarray(centre)
    return p, nrm


def plane_step(p, q, n, axis):
    J4 = np.c_[np.cross(p, n) @ axis, n]
    r = ((p - q) * n).sum(1)
    y = np.linalg.solve(J4.T @ J4, -(J4.T @ r))
    T = np.eye(4)
    T[:3, :3] = rot(axis, y[0])
    T[:3, 3] = y[1:]
    return T


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [Y, GENERAL], ids=["y", "general"])
def test_point_to_plane_equals_python_loop(lib, axis):
    tgt, nrm = _ellipsoid(9000, 40, noise=2e-4)
    src, _ = _ellipsoid(3000, 50)
    c0 = tgt.mean(0)
    src = (src - c0) @ rot(axis, 0.05).T + c0 + np.array([0.004, -0.003, 0.002])
    r, iters = 0.03, 10
    c = ctx_with(src, tgt, axis)
    c.set_target_normals_f64(nrm)
    T = np.eye(4)
    for _ in range(iters):
        c.nn_pass(T, r)
        si, ti, _ = c.get_correspondences()
        p = src[si] @ T[:3, :3].T + T[:3, 3]
        T = plane_step(p, tgt[ti], nrm[ti], axis) @ T
    c.nn_pass(T, r)
    k = len(c.get_correspondences()[0])
    res = c.run_point_to_plane(None, r, iters, 0.0, 0.0)
    assert res.num_correspondences == k
    assert np.abs(res.transformation_ - T).max() < 1e-10, np.abs(res.transformation_ - T).max()
    assert upright_err(res.transformation_, axis) < 1e-12
    b = _lib.Context(0)
    b.set_rotation_axis(axis)
    got = b.run_batch_point_to_plane([(src, tgt, nrm, None, r), (src, tgt, nrm, None, r)], iters, 0.0, 0.0)
    for g in got:
        assert g.num_correspondences == k
        assert np.abs(g.transformation_ - T).max() < 1e-10, np.abs(g.transformation_ - T).max()
    c.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_corpus_two_contexts_equal_one_and_axes_must_agree(lib):
    objs, _ = c3()
    scene = objs[0][1]
    items = [(objs[i][0][:3000], scene) for i in range(4)]
    corpus = _lib.Corpus(items, level=24, max_dist=0.02, max_iter=20)
    one = _lib.Context(0)
    one.set_rotation_axis(Y)
    a = corpus.run([one])
    two = [_lib.Context(0) for _ in range(2)]
    for x in two:
        x.set_rotation_axis(Y)
    b = _lib.Corpus(items, level=24, max_dist=0.02, max_iter=20).run(two)
    for (ra, la, _, ia), (rb, lb, _, ib) in zip(a, b):
        assert la == lb and ia == ib
        assert ra.num_correspondences == rb.num_correspondences
        assert np.array_equal(ra.transformation_, rb.transformation_)
        assert upright_err(ra.transformation_) < 1e-12
    two[1].set_rotation_axis(GENERAL)
    with pytest.raises(lib.IcpError):
        _lib.Corpus(items, level=24, max_dist=0.02, max_iter=20).run(two)
    with pytest.raises(lib.IcpError):
        _lib.run_batch_multi(two, [(items[0][0], scene, None, 0.02)] * 2, 10)
    for x in [one] + two:
        x.close()


@pytest.mark.gpu
def test_edges(lib):
    src, tgt, _, r = synth.make_pair(3000, 9000)
    fresh = _lib.Context(0)
    fresh.set_clouds_f64(src, tgt)
    ref_res = fresh.run(None, r, 30)
    # set and cleared before any registration: the context is a fresh one
    b = _lib.Context(0)
    b.set_clouds_f64(src, tgt)
    b.set_rotation_axis(Y)
    b.set_rotation_axis(None)
    same = b.run(None, r, 30)
    assert np.array_equal(same.transformation_, ref_res.transformation_)
    assert same.num_correspondences == ref_res.num_correspondences and same.iterations == ref_res.iterations
    b.close()
    c = _lib.Context(0)
    c.set_clouds_f64(src, tgt)
    assert c.rotation_axis() is None
    c.set_rotation_axis([0, 2.0, 0])
    assert np.array_equal(c.rotation_axis(), Y)
    with pytest.raises(lib.IcpError):
        c.run(None, r, 30, with_scaling=True)
    for solver in (lib.SOLVER_GN_EULER, lib.SOLVER_GN_EXPMAP):
        with pytest.raises(lib.IcpError):
            c.run(None, r, 30, solver=solver)
        with pytest.raises(lib.IcpError):
            c.run_batch([(src, tgt, None, r)] * 2, 10, solver=solver)
    for bad in ([0, 0, 0], [np.nan, 1, 0], [1e-15, 0, 0]):
        with pytest.raises(lib.IcpError):
            c.set_rotation_axis(bad)
    assert np.array_equal(c.rotation_axis(), Y)                   # (a refused axis leaves the one in use)
    c.run(None, r, 30)
    c.set_rotation_axis(None)
    assert c.rotation_axis() is None
    again = c.run(None, r, 30)
    # (behind a registration of its own the search starts warm: the same result to rounding)
    assert np.abs(again.transformation_ - ref_res.transformation_).max() < 1e-9
    assert again.num_correspondences == ref_res.num_correspondences and again.iterations == ref_res.iterations
    # sharded ranks take no axis (the header's rule), in either order
    c.set_rotation_axis(Y)
    with pytest.raises(lib.IcpError):
        c.set_target_shard(0, 2 * len(tgt), np.zeros(3))
    with pytest.raises(lib.IcpError):
        c.set_allreduce(lambda st: None, 0, 2)
    s = _lib.Context(0)
    s.set_target_shard(0, 2 * len(tgt), np.zeros(3))
    with pytest.raises(lib.IcpError):
        s.set_rotation_axis(Y)
    for x in (fresh, c, s):
        x.close()
