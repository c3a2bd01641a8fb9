"""The whole-wave re-scan of the certificate kernel (visma_amd/csrc/grid_coop.hip, the end of a searcher's f64 stage): a
query the chunk bookkeeping cannot decide -- a third chunk inside the rounding band, more than four flagged candidates --
has every listed candidate ranked in f64 by its whole wave, one such query at a time.  On ordinary clouds that is one query
in thousands; the clouds here make it the common path: the target is a lattice (with points given twice), the queries sit
at the centres of its squares and cubes, so every one of them has 4 or 8 nearest neighbours at EXACTLY the same distance,
in fp32 and in f64.  Many lanes of one wave take the path at once, two waves of a workgroup, every workgroup, some
workgroups and not others (what a version that defers the re-scan behind the wave's other queries would have to get right:
uniform branches, the hand-over of a slow query -- DESIGN 4.1e, round 7).  Compared bit for bit with the lane-serial kernel
(indices, d2, the 38 statistics, the state-dependent next passes), once per pass (nn_coop_kernel_one / _many) and inside a
host loop (nn_coop_kernel_persist); the ties must resolve to the lowest original index, as the reference's ranking does,
and they must really be there."""
import os

import numpy as np
import pytest

from visma_amd import _lib, synth

pytestmark = pytest.mark.gpu

H = 0.25                      # lattice spacing: every coordinate and every squared distance below is exact in fp32
RADIUS = 0.3                  # > sqrt(3) / 2 * H = 0.2165 (cube centre to corner)
SERIAL = {"VISMA_ICP_COOP": "0", "VISMA_ICP_GRID_LANES": "801"}


def ctx_env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def lattice(n, dup_every=0):
    """n^3 lattice points (original order shuffled), every dup_every-th of them given a second time at the end"""
    rng = np.random.default_rng(n)
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float64) * H
    p = p[rng.permutation(len(p))]
    if dup_every:
        p = np.concatenate([p, p[::dup_every]])
    return p


def centres(n, count, seed, squares=True):
    """`count` centres of lattice cubes (8-way ties) and, every other one, of lattice squares (4-way ties)"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, n - 1, (count, 3)).astype(np.float64)
    q = (c + 0.5) * H
    if squares:
        q[1::2, 2] = c[1::2, 2] * H
    return q


def generic(n, count, seed, x_lo=0):
    """points of general position inside the lattice (cells x_lo and up along x): one nearest neighbour, or one given twice"""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, n - 1, (count, 3))
    cell[:, 0] = rng.integers(x_lo, n - 1, count)
    return rng.uniform(0.3, 0.45, (count, 3)) * H + cell * H


def expected_at_identity(src, tgt):
    """brute force in the reference's arithmetic (flann L2: dx*dx, += dy*dy, += dz*dz; the lowest original index on an
    exact tie) -> (index per query, squared distance, how many target points share that distance)"""
    idx = np.empty(len(src), np.int64)
    d2 = np.empty(len(src))
    ties = np.empty(len(src), np.int64)
    for a in range(0, len(src), 256):
        s = src[a:a + 256]
        dx = tgt[None, :, 0] - s[:, None, 0]
        dy = tgt[None, :, 1] - s[:, None, 1]
        dz = tgt[None, :, 2] - s[:, None, 2]
        d = dx * dx
        d += dy * dy
        d += dz * dz
        m = d.min(axis=1)
        idx[a:a + 256] = d.argmin(axis=1)                  # (the first minimum: the lowest index)
        d2[a:a + 256] = m
        ties[a:a + 256] = (d == m[:, None]).sum(axis=1)
    return idx, d2, ties


def d2_per_query(x):
    si, _, d2 = x.get_correspondences()
    out = np.full(x.ns, np.nan, np.float32)
    out[si] = d2
    return out


def small_T(rng, m):
    return synth.make_T(synth.rot_y(rng.uniform(-1, 1) * m * RADIUS * 0.5) @ synth.rot_x(rng.uniform(-1, 1) * m * RADIUS * 0.3),
                        rng.standard_normal(3) * RADIUS * m * 0.5)


def three_contexts(src, tgt, normals=None):
    ref = ctx_env(SERIAL)
    nocert = ctx_env({"VISMA_ICP_CERT": "0"})
    c = _lib.Context(0)
    for x in (ref, nocert, c):
        x.set_nn_mode(_lib.NN_GRID)
        x.set_ring_search(0)
        x.set_clouds_f64(src, tgt)
        if normals is not None:
            x.set_target_normals_f64(normals)
    return ref, nocert, c


def passes_equal(name, ctxs, motions, seed):
    """the per-pass API: every context runs the same sequence of poses; everything bit for bit against the first"""
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    first = None
    for p, m in enumerate(motions):
        if m is None:
            T = np.eye(4)                                     # exactly: the ties are exact again
        elif m > 0:
            T = small_T(rng, m) @ T
        outs = []
        for x in ctxs:
            x.nn_pass(T, RADIUS)
            st = x.reduce()
            outs.append((x.correspondence_index(), x.get_correspondences()[2].view(np.uint32), st.view(np.uint64)))
        if first is None:
            first = outs[0]
        for w, o in enumerate(outs[1:]):
            assert np.array_equal(o[0], outs[0][0]), (name, w, p)
            assert np.array_equal(o[1], outs[0][1]), (name, w, p)
            if p > 0:                                         # (the cold pass may use more lanes per query)
                assert np.array_equal(o[2], outs[0][2]), (name, w, p)
    return first


# name, lattice side, queries, share of them that are tie centres, where the generic ones go, duplicates
CASES = [
    ("many lanes of one wave", 12, 64, 1.0, 0),
    ("two waves of one workgroup", 12, 128, 1.0, 3),
    ("every workgroup", 14, 1000, 1.0, 3),
    ("some workgroups without a slow query", 14, 1024, 0.25, 3),
    ("one slow query in all", 12, 700, 0.0, 0),
]
MOTIONS = [None, None, 0.02, 0.0, None, 0.3, 0.01, None]


@pytest.mark.parametrize("name,n,count,tie_share,dup", CASES, ids=[c[0] for c in CASES])
def test_ties_take_the_rescan_and_equal_the_lane_serial_kernel(lib, name, n, count, tie_share, dup):
    tgt = lattice(n, dup)
    k = int(round(count * tie_share))
    # (the tie centres come last and lie in one corner of the lattice when they share the source with generic points:
    #  in the order of the array and in the order of space alike, some workgroups hold none of them)
    ties_q = centres(n if tie_share == 1.0 else 4, k, seed=count) if k else np.empty((0, 3))
    gen_q = generic(n, count - k, seed=count + 1, x_lo=0 if tie_share == 0.0 else 4)
    src = np.concatenate([gen_q, ties_q])
    if tie_share == 0.0:
        src[len(src) // 2] = (np.array([3, 4, 5]) + 0.5) * H  # one 8-way tie among 699 generic queries
    want_idx, want_d2, ties = expected_at_identity(src, tgt)
    slow_share = float(np.mean(ties >= 3))
    if tie_share > 0.0:
        assert not np.any(ties[:count - k] >= 3)              # (the generic queries: decided by the chunk bookkeeping)
    else:
        assert int(np.sum(ties >= 3)) == 1
    print("%s: %d queries, %.1f%% of them with 3 or more nearest neighbours at the same distance" % (name, len(src), 100 * slow_share))
    assert slow_share > 0.0
    if tie_share == 1.0:
        assert ties.min() >= 4
    ctxs = three_contexts(src, tgt)
    first = passes_equal(name, ctxs, MOTIONS, seed=n + count)
    # the poses that are exactly the identity: the lowest original index among the tied points, the exact distance
    assert np.array_equal(first[0], want_idx.astype(np.int32))
    for x in ctxs:
        x.nn_pass(np.eye(4), RADIUS)
        x.reduce()
        assert np.array_equal(x.correspondence_index(), want_idx.astype(np.int32)), name
        assert np.array_equal(d2_per_query(x), want_d2.astype(np.float32)), name
    for x in ctxs:
        x.close()


def host_loops_equal(name, src, tgt, normals=None):
    """whole host loops: one launch of the certificate kernel per pass, the persistent launch, the persistent launch with
    every query queued in every pass.  (The lane-serial kernel is compared pass by pass, passes_equal: a host loop's cold
    pass may sum its statistics over more lanes per query than the lane-serial one.)"""
    ref = ctx_env({"VISMA_ICP_CERT": "0"})
    per_pass, persist = _lib.Context(0), _lib.Context(0)
    ref.set_persistent(True)
    per_pass.set_persistent(False)
    persist.set_persistent(True)
    for x in (ref, per_pass, persist):
        x.set_nn_mode(_lib.NN_GRID)
        x.set_ring_search(0)
        x.set_clouds_f64(src, tgt)
        if normals is not None:
            x.set_target_normals_f64(normals)
    persist.set_profiling(1)
    persist.get_timing(reset=True)
    rng = np.random.default_rng(len(src))
    T0 = small_T(rng, 0.05)
    if normals is None:
        Ts = [np.eye(4), np.eye(4), np.eye(4)]
        for steps in (1, 6, 3):                               # (from the identity: the first passes see the exact ties)
            outs = []
            for w, x in enumerate((ref, per_pass, persist)):
                Ts[w], res = x.iterate(Ts[w], RADIUS, steps)
                outs.append((Ts[w].copy(), res, [v.view(np.uint32) for v in x.get_correspondences()]))
            for o in outs[1:]:
                assert np.array_equal(o[0], outs[0][0]), (name, steps)
                assert o[1].num_correspondences == outs[0][1].num_correspondences and o[1].inlier_rmse_ == outs[0][1].inlier_rmse_
                for u, v in zip(o[2], outs[0][2]):
                    assert np.array_equal(u, v), (name, steps)
    else:
        for init in (None, T0):
            outs = [x.run_point_to_plane(init, RADIUS, 8, 0.0, 0.0) for x in (ref, per_pass, persist)]
            idxs = [x.correspondence_index() for x in (ref, per_pass, persist)]
            for o, i in zip(outs[1:], idxs[1:]):
                assert np.array_equal(np.asarray(o.transformation_), np.asarray(outs[0].transformation_)), name
                assert o.num_correspondences == outs[0].num_correspondences and o.inlier_rmse_ == outs[0].inlier_rmse_
                assert np.array_equal(i, idxs[0]), name
    tm = persist.get_timing(reset=True)
    for x in (ref, per_pass, persist):
        x.close()
    return tm


def test_host_loops_over_ties_point_to_point_and_point_to_plane(lib):
    n = 14
    tgt = lattice(n, 3)
    src = np.concatenate([generic(n, 300, seed=5), centres(n, 700, seed=6)])
    _, _, ties = expected_at_identity(src, tgt)
    assert float(np.mean(ties >= 3)) > 0.5
    tm = host_loops_equal("point-to-point", src, tgt)
    assert tm["persist_launches"] >= 2 and tm["persist_aborts"] == 0, tm
    # normals of a lattice: anything of unit length will do for the comparison -- the same on every context
    rng = np.random.default_rng(9)
    nrm = rng.standard_normal((len(tgt), 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    tm = host_loops_equal("point-to-plane", src, tgt, nrm)
    assert tm["persist_launches"] >= 1 and tm["persist_aborts"] == 0, tm


def test_several_queries_per_lane_over_ties(lib):
    """a source too big for one query per lane (nn_coop_kernel_many) at a small grid: every query a 4- or 8-way tie"""
    n = 12
    tgt = lattice(n, 0)
    base = centres(n, 1331, seed=2)
    src = np.tile(base, (210, 1))                             # 279,510 queries
    _, _, ties = expected_at_identity(base, tgt)
    assert ties.min() >= 4
    ctxs = three_contexts(src, tgt)
    passes_equal("several queries per lane", ctxs, [None, None, 0.02, None], seed=3)
    want_idx, _, _ = expected_at_identity(base, tgt)
    assert np.array_equal(ctxs[2].correspondence_index(), np.tile(want_idx.astype(np.int32), 210))
    for x in ctxs:
        x.close()


def test_one_small_case_against_the_oracle(lib, oracle):
    n = 12
    tgt = lattice(n, 4)
    src = np.concatenate([generic(n, 100, seed=11), centres(n, 200, seed=12)])
    want_idx, _, ties = expected_at_identity(src, tgt)
    assert float(np.mean(ties >= 3)) > 0.5
    k, o_idx, o_d2, _ = oracle.nn_pass(src, tgt, RADIUS)
    assert np.array_equal(o_idx, want_idx.astype(np.int32)) and k == len(src)
    c = _lib.Context(0)
    c.set_nn_mode(_lib.NN_GRID)
    c.set_ring_search(0)
    c.set_clouds_f64(src, tgt)
    for _ in range(3):                                        # (cold pass, then two warm ones at the same pose)
        c.nn_pass(np.eye(4), RADIUS)
        c.reduce()
        assert np.array_equal(c.correspondence_index(), o_idx)
        assert np.array_equal(d2_per_query(c), o_d2.astype(np.float32))
    c.close()
