"""BASELINE config 3 at its real shape: all objects of one scene in flight -- 12 objects x 24 yaw
starts = 288 ICPs in ONE visma_icp_run_batch (bench.py --workload c3 times this set).  EVERY one of the 288 results,
from every path that computes them (one batch, the batch dealt to 2 and 3 worker contexts, one registration at a time
with the host loop and with the device loop), is held to the COMPILED REFERENCE's own output
(tests/golden/c3_ref.npz, written by tests/golden/gen_batch_ref.py from oracle/_ref: Open3D's RegistrationICP with its
default criteria, one call per problem): K equal, fitness bit-equal, rmse and transformation within 1e-9."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_batch_ref  # noqa: E402
import gen_c4  # noqa: E402
from bench import c3_problems  # noqa: E402
from visma_amd import _lib, synth  # noqa: E402

G3 = np.load(os.path.join(HERE, "golden", "c3_ref.npz"))


@pytest.fixture(scope="module")
def c3():
    return c3_problems()


def _name(probs, i):
    src, tgt, _, r, oi = probs[i]
    return "object %d start %d (%d -> %d points, r = %g)" % (oi, i % 24, len(src), len(tgt), r)


def _against_fixture(what, results, probs):
    """Every one of the 288 results against the compiled reference's; prints (and returns) the worst distances seen."""
    assert len(results) == len(probs) == len(G3["k"]) == 288
    wt = wr = 0.0
    for i, g in enumerate(results):
        at = "%s: %s" % (what, _name(probs, i))
        assert g.num_correspondences == int(G3["k"][i]), at
        assert g.fitness_ == float(G3["fitness"][i]), at                      # both are K / NS in f64
        er = abs(g.inlier_rmse_ - float(G3["rmse"][i])) / float(G3["rmse"][i])
        et = synth.rel_frobenius(g.transformation_, G3["T"][i])                # (K >= 3 everywhere: the CPU test below)
        wt, wr = max(wt, et), max(wr, er)
        assert er < 1e-9, (at, er)
        assert et < 1e-9, (at, et)
    print("C3 %s vs compiled reference, 288 of 288: worst rel. Frobenius %.3e, worst rel. rmse difference %.3e" % (what, wt, wr))
    return wt, wr


# ---- the fixture itself (no GPU): it cannot rot unseen ------------------------------------------------------------
def test_c3_fixture_is_consistent_and_its_inputs_regenerate(c3):
    """shapes, fitness == K / NS exactly, no problem with K < 3, no registration on which the two CPU implementations
    disagreed, and the clouds this machine generates are the ones the reference saw"""
    objs, probs = c3
    assert G3["T"].shape == (288, 4, 4) and G3["T"].dtype == np.float64
    for key in ("k", "fitness", "rmse", "idx_sum", "idx_wsum"):
        assert G3[key].shape == (288,), key
    assert int(G3["level"]) == 24 and int(G3["max_iter"]) == 30 and float(G3["radius"]) == 0.02
    assert len(G3["cpu_disagree"]) == 0, G3["cpu_disagree"]
    assert int(G3["k"].min()) >= 3
    assert np.array_equal(G3["T"][:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (288, 1)))
    for oi, (src, tgt) in enumerate(objs):
        assert (len(src), len(tgt)) == (int(G3["ns"][oi]), int(G3["nt"][oi])), oi
        assert gen_c4.input_checksum(src) == int(G3["src_checksum"][oi]), oi
        assert gen_c4.input_checksum(tgt) == int(G3["tgt_checksum"][oi]), oi
        sl = slice(24 * oi, 24 * oi + 24)
        assert np.array_equal(G3["fitness"][sl], G3["k"][sl] / float(len(src))), oi
    for i, p in enumerate(probs):
        assert p[3] == float(G3["radius"]) and np.array_equal(p[2], gen_batch_ref.start(i % 24)), i


def test_c3_restatement_equals_the_fixture_on_the_two_smallest_objects(c3, oracle):
    """the independent CPU restatement on 48 of the 288: K equal, transformation and rmse within 1e-9"""
    objs, probs = c3
    wt = 0.0
    for oi in np.argsort([len(s) for s, _ in objs])[:2]:
        for k in range(24):
            i = int(oi) * 24 + k
            src, tgt, init, r, _ = probs[i]
            w = oracle.registration_icp(src, tgt, r, init=init, max_iter=30, grid=True)
            assert w.k == int(G3["k"][i]), _name(probs, i)
            assert w.fitness == float(G3["fitness"][i]), _name(probs, i)
            assert abs(w.rmse - float(G3["rmse"][i])) < 1e-9 * float(G3["rmse"][i]), _name(probs, i)
            e = synth.rel_frobenius(w.T, G3["T"][i])
            wt = max(wt, e)
            assert e < 1e-9, (_name(probs, i), e)
            assert gen_c4.checksum(w.idx) == (int(G3["idx_sum"][i]), int(G3["idx_wsum"][i]), w.k), _name(probs, i)
    print("C3 restatement vs compiled reference, 48 registrations: worst rel. Frobenius %.3e" % wt)


def test_c3_reference_repeats_the_fixture(c3, ref):
    """Where the compiled reference is built: the smallest object's 24 registrations, regenerated.  K, fitness and the
    final correspondence set repeat exactly.  The transformation and the rmse do NOT repeat bit for bit: the
    reference merges its per-thread correspondence lists and sums inside an OpenMP critical section, in the order
    the threads arrive (Registration.cpp:54-82), so the order of its sums changes from run to run.  Held to 1e-12;
    seen on 8 cores, three runs: at most 2.9e-15 in the transformation, 8.0e-15 in the rmse."""
    objs, probs = c3
    oi = int(np.argmin([len(s) for s, _ in objs]))
    wt = wr = 0.0
    for k in range(24):
        i = oi * 24 + k
        src, tgt, init, r, _ = probs[i]
        w = ref.registration_icp(src, tgt, r, init=init, max_iter=30)
        assert (w.k, w.fitness) == (int(G3["k"][i]), float(G3["fitness"][i])), _name(probs, i)
        assert gen_c4.checksum(w.idx) == (int(G3["idx_sum"][i]), int(G3["idx_wsum"][i]), w.k), _name(probs, i)
        et = synth.rel_frobenius(w.T, G3["T"][i])
        er = abs(w.rmse - float(G3["rmse"][i])) / float(G3["rmse"][i])
        wt, wr = max(wt, et), max(wr, er)
        assert et < 1e-12 and er < 1e-12, (_name(probs, i), et, er)
    print("C3 compiled reference, run again, 24 registrations: worst rel. Frobenius %.3e, worst rel. rmse difference %.3e" % (wt, wr))


# ---- the GPU paths ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_288_problems_in_flight(lib, oracle, c3):
    """One visma_icp_run_batch over the 288 problems: all 288 against the compiled reference, all 288 against
    one-at-a-time host-loop runs of the library (each of those against the reference too, its final correspondence
    set included: the batch API returns no pairs), and a sample against the CPU restatement.
    Measured on the MI355X, all 288 (worst relative Frobenius / worst relative rmse difference to the compiled
    reference): one batch 7.1e-15 / 1.6e-14, one at a time on the host loop 7.1e-15 / 1.6e-14."""
    objs, probs = c3
    assert len(probs) == 288
    ctx = _lib.Context(0)
    got = ctx.run_batch([p[:4] for p in probs], max_iter=30)
    assert ctx.search_mode_used() == "exact"
    _against_fixture("one batch", got, probs)
    # every problem against a one-at-a-time host-loop run of the library
    _one_at_a_time(got, objs, probs, False)
    # a sample against the oracle (the CPU restatement of Open3D's RegistrationICP)
    rng = np.random.default_rng(0)
    for i in rng.choice(288, 6, replace=False):
        src, tgt, init, r, _ = probs[int(i)]
        w = oracle.registration_icp(src, tgt, r, init=init, max_iter=30, grid=True)
        assert got[i].num_correspondences == w.k, i
        if w.k >= 3:
            assert synth.rel_frobenius(got[i].transformation_, w.T) < 1e-9, i
    ctx.close()


def _one_at_a_time(got, objs, probs, device_loop):
    """all 12 objects x 24 starts through visma_icp_run, one registration per call: equal to the batch's result `got`
    (K, iterations, 1e-11) and to the compiled reference's (its final correspondence set by two checksums)"""
    one = _lib.Context(0)
    one.set_device_loop(device_loop)
    single = []
    for oi in range(12):
        src, tgt = objs[oi]
        one.set_clouds_f64(src, tgt)
        for k in range(24):
            i = oi * 24 + k
            w = one.run(probs[i][2], 0.02, 30)
            assert got[i].num_correspondences == w.num_correspondences, (oi, k)
            assert got[i].iterations == w.iterations, (oi, k)
            assert synth.rel_frobenius(got[i].transformation_, w.transformation_) < 1e-11, (oi, k)
            s1, s2, kk = gen_c4.checksum(one.correspondence_index())
            assert (s1, s2, kk) == (int(G3["idx_sum"][i]), int(G3["idx_wsum"][i]), int(G3["k"][i])), _name(probs, i)
            single.append(w)
    assert one.search_mode_used() == "exact"
    one.close()
    _against_fixture("one at a time, %s loop" % ("device" if device_loop else "host"), single, probs)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_288_problems_one_at_a_time_on_the_device_loop(lib, c3):
    """The same 288 through the device-resident loop of visma_icp_run, against the batch and the compiled reference.
    Measured on the MI355X: 7.1e-15 / 1.6e-14 (worst relative Frobenius / rmse difference over the 288)."""
    objs, probs = c3
    ctx = _lib.Context(0)
    got = ctx.run_batch([p[:4] for p in probs], max_iter=30)
    ctx.close()
    _one_at_a_time(got, objs, probs, True)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("workers", [2, 3])
def test_288_problems_over_worker_contexts(lib, c3, workers):
    """visma_icp_run_batch_multi as bench.py --workload c3 calls it (objects dealt to the worker contexts, shares side
    by side): all 288 against the compiled reference, and bit-equal to the one-context batch.
    Measured on the MI355X, 2 and 3 contexts alike: 7.1e-15 / 1.6e-14 (worst relative Frobenius / rmse difference)."""
    objs, probs = c3
    ctxs = [_lib.Context(0) for _ in range(workers)]
    batch = ctxs[0].make_batch([p[:4] for p in probs])
    want = ctxs[0].run_batch(batch, max_iter=30)
    want = [(w.transformation_.copy(), w.num_correspondences, w.iterations, w.fitness_, w.inlier_rmse_) for w in want]
    got = _lib.run_batch_multi(ctxs, batch, max_iter=30)
    _against_fixture("batch over %d worker contexts" % workers, got, probs)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a.num_correspondences, a.iterations, a.fitness_, a.inlier_rmse_) == b[1:], _name(probs, i)
        assert np.array_equal(a.transformation_, b[0]), _name(probs, i)
    for c in ctxs:
        c.close()


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("ring", [-1, 0, 1])
def test_288_problems_under_each_ring_search_setting(lib, c3, ring):
    """set_ring_search(-1 / 0 / 1) before the batch, all 288 against the compiled reference each time.
    A batch does NOT honour the setting: run_loop_batch plans one radius-sized grid per problem (grid_plan) and never
    the ring grid, so all three runs cover the same kernel family (the lane-serial first pass and nn_wave_kernel_one
    after it) and ring_search() reports no ring grid.  The single registrations below (the same context, the largest
    object, its 24 starts, each against the reference with its correspondence set) do consult the setting, but at
    r = 0.02 their radius-sized grid holds 1.15 points per occupied cell, below what the ring search asks for, so
    set_ring_search(1) keeps the radius-sized grid too: NO run of config 3 reaches grid_ring.hip, and this parity does
    not cover it (the large-radius fixture c4_literal_ref.npz does).  The log prints what ring_search() reported.
    Measured on the MI355X, every setting: batch 7.1e-15 / 1.6e-14 over the 288, single runs 6.1e-15 (worst relative
    Frobenius / rmse difference)."""
    objs, probs = c3
    ctx = _lib.Context(0)
    ctx.set_ring_search(ring)
    got = ctx.run_batch([p[:4] for p in probs], max_iter=30)
    print("C3 batch under set_ring_search(%d): ring_search() = %s, search kernel %s" % (ring, ctx.ring_search(), ctx.search_kernel_used()))
    assert ctx.ring_search()["rings"] == 0
    _against_fixture("one batch, set_ring_search(%d)" % ring, got, probs)
    oi = int(np.argmax([len(s) for s, _ in objs]))
    src, tgt = objs[oi]
    ctx.set_clouds_f64(src, tgt)
    wt = 0.0
    for k in range(24):
        i = oi * 24 + k
        w = ctx.run(probs[i][2], 0.02, 30)
        assert w.num_correspondences == int(G3["k"][i]), _name(probs, i)
        assert w.fitness_ == float(G3["fitness"][i]), _name(probs, i)
        assert abs(w.inlier_rmse_ - float(G3["rmse"][i])) < 1e-9 * float(G3["rmse"][i]), _name(probs, i)
        e = synth.rel_frobenius(w.transformation_, G3["T"][i])
        wt = max(wt, e)
        assert e < 1e-9, (_name(probs, i), e)
        assert gen_c4.checksum(ctx.correspondence_index()) == (int(G3["idx_sum"][i]), int(G3["idx_wsum"][i]), int(G3["k"][i])), _name(probs, i)
    rs = ctx.ring_search()
    print("C3 single runs of object %d under set_ring_search(%d): ring_search() = %s, search kernel %s, worst rel. Frobenius %.3e"
          % (oi, ring, rs, ctx.search_kernel_used(), wt))
    if ring == 0:
        assert rs["rings"] == 0
    ctx.close()


def _ellipsoid(n, seed, axes=(0.5, 0.3, 0.2), centre=(0.3, -0.2, 1.0), noise=0.0):
    """points on an ellipsoid with three different axes (all six degrees of freedom are constrained)
    and their exact unit normals"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = np.asarray(axes)
    p = u * a
    nrm = p / a ** 2
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = p + rng.normal(size=p.shape) * noise + np.asarray(centre)
    return p, nrm


def _pp_problems():
    probs = []
    for k, (ns, nt, r) in enumerate([(3000, 9000, 0.03), (5000, 20000, 0.02), (1500, 4000, 0.045)]):
        tgt, nrm = _ellipsoid(nt, 40 + k, noise=2e-4)
        src, _ = _ellipsoid(ns, 50 + k)
        a = 0.02
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        c = tgt.mean(0)
        src = (src - c) @ R.T + c + np.array([0.004, -0.003, 0.002])
        for y in range(3):                                       # the same clouds from three starts: shared uploads
            b = 0.01 * y
            init = np.eye(4)
            Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
            init[:3, :3] = Ry
            init[:3, 3] = c - Ry @ c
            probs.append((src, tgt, nrm, init, r))
    return probs


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("precision", ["exact", "f32"])
def test_batch_point_to_plane_equals_single_runs_and_oracle(lib, oracle, precision):
    """visma_icp_run_batch_point_to_plane: problems with their own clouds and normals, shared targets
    included, against one-at-a-time runs of the library and the oracle's point-to-plane ICP."""
    from oracle.oracle import EST_POINT_TO_PLANE
    probs = _pp_problems()
    ctx = _lib.Context(0)
    ctx.set_search_precision(precision)
    got = ctx.run_batch_point_to_plane(probs, max_iter=15)
    assert ctx.search_mode_used() == precision
    one = _lib.Context(0)
    one.set_search_precision(precision)
    one.set_device_loop(False)
    for i, (src, tgt, nrm, init, r) in enumerate(probs):
        one.set_clouds_f64(src, tgt)
        one.set_target_normals_f64(nrm)
        w = one.run_point_to_plane(init, r, 15)
        assert w.fitness_ > 0.9, (i, w)                            # the registrations do converge
        assert got[i].num_correspondences == w.num_correspondences, i
        assert got[i].iterations == w.iterations, i
        assert synth.rel_frobenius(got[i].transformation_, w.transformation_) < (1e-10 if precision == "exact" else 1e-6), i
        if precision == "exact" and i % 3 == 0:
            o = oracle.registration_icp(src, tgt, r, init=init, max_iter=15, estimator=EST_POINT_TO_PLANE,
                                        tgt_normals=nrm, grid=True)
            assert got[i].num_correspondences == o.k, i
            assert synth.rel_frobenius(got[i].transformation_, o.T) < 1e-9, i


@pytest.mark.gpu
def test_batch_point_to_plane_without_normals_returns_the_initial_transform(lib):
    tgt, nrm = _ellipsoid(6000, 3)
    src, _ = _ellipsoid(2000, 4)
    r = 0.04
    init = np.eye(4); init[0, 3] = 1e-3
    ctx = _lib.Context(0)
    got = ctx.run_batch_point_to_plane([(src, tgt, nrm, init, r), (src, tgt.copy(), None, init, r)], max_iter=5)
    assert got[0].num_correspondences > 0 and not np.allclose(got[0].transformation_, init)
    assert np.array_equal(got[1].transformation_, init)          # Registration.cpp:152-157


def test_abi_exports_the_multi_context_batch(lib):
    assert hasattr(lib.load(), "visma_icp_run_batch_multi")


@pytest.mark.gpu
def test_batch_over_worker_contexts_equals_one_context(lib):
    """visma_icp_run_batch_multi: the problems dealt (targets kept together) to 1, 2 and 3 contexts on the same GPU,
    shares side by side -- every problem's result is the single-context batch's, bit for bit."""
    from visma_amd import _lib, synth
    rng = np.random.default_rng(5)
    probs = []
    for k, (ns, nt) in enumerate(((3000, 9000), (7000, 5000), (1500, 12000), (5000, 5000), (900, 700))):
        src, tgt, T_gt, _ = synth.make_pair(ns, nt, seed_t=30 + k, seed_s=60 + k, motion="fixed")
        for yaw in (0.0, 0.2, -0.3):
            probs.append((src, tgt, synth.make_T(synth.rot_y(yaw), rng.normal(size=3) * 0.01), 0.05 + 0.01 * k))
    ctxs = [_lib.Context(0) for _ in range(3)]
    want = ctxs[0].run_batch(probs, max_iter=15)
    for W in (1, 2, 3):
        got = _lib.run_batch_multi(ctxs[:W], probs, max_iter=15)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.num_correspondences == b.num_correspondences and a.iterations == b.iterations
            assert np.array_equal(a.transformation_, b.transformation_)
    for c in ctxs:
        c.close()


@pytest.mark.gpu
def test_batch_over_worker_contexts_edge_cases(lib):
    """more contexts than target groups, an empty batch, a failing share (message comes back)"""
    src, tgt, _, _ = synth.make_pair(2000, 4000, seed_t=3, seed_s=4, motion="fixed")
    ctxs = [_lib.Context(0) for _ in range(3)]
    probs = [(src, tgt, synth.make_T(synth.rot_y(0.1 * k), [0, 0, 0]), 0.05) for k in range(4)]   # ONE target group
    want = ctxs[0].run_batch(probs, max_iter=8)
    got = _lib.run_batch_multi(ctxs, probs, max_iter=8)              # only one context gets work
    for a, b in zip(got, want):
        assert np.array_equal(a.transformation_, b.transformation_) and a.num_correspondences == b.num_correspondences
    assert _lib.run_batch_multi(ctxs, [], max_iter=8) == []
    L = _lib.load()
    import ctypes as C
    h = (C.c_void_p * 2)(ctxs[0]._h, None)
    err = C.create_string_buffer(256)
    arr, n, _keep, out = ctxs[0].make_batch(probs)
    assert L.visma_icp_run_batch_multi(h, 2, arr, n, 8, 1e-6, 1e-6, 0, out, err, 256) != 0 and b"NULL context" in err.value
    assert L.visma_icp_run_batch_multi(h, 1, arr, n, 8, 1e-6, 1e-6, 99, out, err, 256) != 0 and len(err.value) > 0   # unknown solver
    for c in ctxs:
        c.close()
