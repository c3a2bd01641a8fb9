"""The chunk loop of the certificate kernel (visma_amd/csrc/grid_coop.hip, phase B2) runs only the slots of a trip that hold
a chunk: the count of live slots is a wave-uniform scalar made from the window's chunk total, the trip's base and the
wave's first position.  What that arithmetic can get wrong depends on the chunk total of a WORKGROUP alone, so the clouds
here are swept until a workgroup lists exactly the totals at its edges -- none at all, fewer than 8 (one octet of wave 0),
31 / 32 / 33 (the last wave's last octet, the first position of slot 1), 223 / 224 / 225 (the end of a trip), more than
1,408 (a second list window) -- and the kernel's own word says so: the persistent launch's timeline records, per pass and
workgroup, the queued queries and the chunks listed (VISMA_ICP_PERSIST_TIMELINE; the chunk total modulo 256), and the
profiling counters give the candidates listed.  Every case is compared bit for bit with the lane-serial kernel: indices,
d2, the 38 statistics, the state-dependent next pass -- once per pass (nn_coop_kernel_one) and inside a host loop
(nn_coop_kernel_persist), with the certificate on and with VISMA_ICP_CERT=0 (every query queued in every pass)."""
import os

import numpy as np
import pytest

from visma_amd import _lib, synth

pytestmark = pytest.mark.gpu

SIDE = 30                         # 27,000 target points
H = 1.0 / SIDE
R_SMALL = 1.5 * H                 # 20^3 = 8,000 radius-sized cells, ~3.4 points in each: one chunk per cell
R_BIG = 3.75 * H                  # 8^3 = 512 cells, ~53 points in each: 7 chunks per cell
SERIAL = {"VISMA_ICP_COOP": "0", "VISMA_ICP_GRID_LANES": "801"}
EDGES = (31, 32, 33, 223, 224, 225)


def ctx_env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    c.set_nn_mode(_lib.NN_GRID)
    c.set_ring_search(0)
    return c


@pytest.fixture(scope="module")
def target():
    rng = np.random.default_rng(30)
    i, j, k = np.meshgrid(np.arange(SIDE), np.arange(SIDE), np.arange(SIDE), indexing="ij")
    p = (np.stack([i.ravel(), j.ravel(), k.ravel()], 1) + 0.5 + rng.uniform(-0.2, 0.2, (SIDE ** 3, 3))) * H
    return p[rng.permutation(len(p))]


def source_of(target, variant, n):
    """n target points themselves (every query's previous winner is at distance zero: the cells listed around it are its
    own cell, and its neighbours' where it lies within 4 % of a radius of a face), from the middle of the cloud"""
    rng = np.random.default_rng(100 + variant)
    inner = np.flatnonzero(np.all((target > 0.2) & (target < 0.8), axis=1))
    return target[rng.permutation(inner)[:n]].copy()


def timeline_records(path):
    """-> [(work[pass][workgroup])] per persistent launch: queued queries | (chunks listed mod 256) << 12"""
    raw = np.fromfile(path, dtype=np.uint64)
    out, pos = [], 0
    while pos + 3 <= len(raw):
        passes, blocks, ran = (int(x) for x in raw[pos:pos + 3])
        n = 2 * passes * blocks
        rec = raw[pos + 3:pos + 3 + n].reshape(passes, blocks, 2)
        out.append((rec[:min(passes, ran), :, 1] >> np.uint64(44)).astype(np.int64))
        pos += 3 + n
    return out


def chunks_of(work):
    """queued queries and chunk total of ONE workgroup's word; the total is recorded modulo 256 and is at least the number
    of queued queries (every query here lists its own cell) and, at the small radius, below twice that + 256"""
    nq, mm = int(work) & 0xFFF, int(work) >> 12
    m = mm
    while m < nq:
        m += 256
    return nq, m


class Loops:
    """the host loops that must agree: one launch of the certificate kernel per pass, the persistent launch, the persistent
    launch with every query queued (and its timeline recorded).  (The lane-serial kernel is compared pass by pass,
    passes_equal: a host loop's cold pass may sum its statistics over more lanes per query than the lane-serial one.)"""

    def __init__(self, tmp_path):
        self.path = str(tmp_path / "timeline.bin")
        self.per_pass = ctx_env({})
        self.persist = ctx_env({})
        self.queued = ctx_env({"VISMA_ICP_CERT": "0", "VISMA_ICP_PERSIST_TIMELINE": self.path})
        self.per_pass.set_persistent(False)
        self.persist.set_persistent(True)
        self.queued.set_persistent(True)
        self.all = (self.per_pass, self.persist, self.queued)

    def close(self):
        for c in self.all:
            c.close()

    def last_work(self):
        return timeline_records(self.path)[-1]

    def scout(self, src, tgt, r):
        """the chunk total of the one workgroup of `src` in a warm pass at the identity"""
        self.queued.set_clouds_f64(src, tgt)
        self.queued.iterate(np.eye(4), r, 3)               # (the cold pass, then a launch of two warm ones)
        return chunks_of(self.last_work()[0, 0])

    def compare(self, name, src, tgt, r, steps=(3, 2)):
        for c in self.all:
            c.set_clouds_f64(src, tgt)
        Ts = [np.eye(4) for _ in self.all]
        works = []
        for s in steps:
            outs = []
            for w, c in enumerate(self.all):
                Ts[w], res = c.iterate(Ts[w], r, s)
                outs.append((Ts[w].copy(), res, [v.view(np.uint32) for v in c.get_correspondences()]))
            works.append(self.last_work())
            for w, o in enumerate(outs[1:]):
                assert np.array_equal(o[0], outs[0][0]), (name, s, w)
                assert o[1].num_correspondences == outs[0][1].num_correspondences, (name, s, w)
                assert o[1].fitness_ == outs[0][1].fitness_ and o[1].inlier_rmse_ == outs[0][1].inlier_rmse_, (name, s, w)
                for u, v in zip(o[2], outs[0][2]):
                    assert np.array_equal(u, v), (name, s, w)
        return works


def passes_equal(name, src, tgt, r, seed):
    """the per-pass API (nn_coop_kernel_one): lane-serial, every query queued, certificate on -- the same poses, everything
    bit for bit; -> the candidates listed by the second pass (warm, at the identity) with every query queued"""
    ctxs = (ctx_env(SERIAL), ctx_env({"VISMA_ICP_CERT": "0"}), ctx_env({}))
    for c in ctxs:
        c.set_clouds_f64(src, tgt)
    ctxs[1].set_profiling(1)
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    listed = None
    for p, m in enumerate((None, None, 0.05, 0.0, 0.4, 0.01, None)):
        if m is None:
            T = np.eye(4)
        elif m > 0:
            T = synth.make_T(synth.rot_y(rng.uniform(-1, 1) * m * r * 0.5) @ synth.rot_x(rng.uniform(-1, 1) * m * r * 0.3),
                             rng.standard_normal(3) * r * m * 0.5) @ T
        outs = []
        for c in ctxs:
            c.nn_pass(T, r)
            st = c.reduce()
            outs.append((c.correspondence_index(), c.get_correspondences()[2].view(np.uint32), st.view(np.uint64)))
        tm = ctxs[1].get_timing(reset=True)
        if p == 1:
            listed = tm["grid_candidates"]
        for w, o in enumerate(outs[1:]):
            assert np.array_equal(o[0], outs[0][0]), (name, w, p)
            assert np.array_equal(o[1], outs[0][1]), (name, w, p)
            if p > 0:                                         # (the cold pass may use more lanes per query)
                assert np.array_equal(o[2], outs[0][2]), (name, w, p)
    for c in ctxs:
        c.close()
    return listed


def test_one_workgroup_at_every_edge_of_the_slot_arithmetic(lib, target, tmp_path):
    loops = Loops(tmp_path)
    # ---- the sweep: sources of 1, 2, 3 ... points of one workgroup, until its chunk total has passed every edge
    found = {}                                               # chunk total -> (variant, n)
    small = None                                             # a total below 8 (one octet of wave 0) with >= 3 queries
    for variant in range(4):
        missing = [e for e in EDGES if e not in found]
        if not missing and small:
            break
        for n in range(3, 257):
            nq, m = loops.scout(source_of(target, variant, n), target, R_SMALL)
            assert nq == n, (variant, n, nq)                  # (VISMA_ICP_CERT=0: every query is queued)
            if m < 8 and small is None:
                small = (variant, n, m)
            if m in EDGES and m not in found:
                found[m] = (variant, n)
            if missing and m > max(missing) + 8:
                break
    print("chunk totals reached: below 8:", small, "| edges:", found)
    assert small is not None
    assert sorted(found) == list(EDGES), found               # every edge was reached exactly, by the kernel's own count
    # ---- every edge: the host loops and the per-pass API, bit for bit; the compared passes list what the sweep saw
    cases = [("below 8", small[0], small[1], small[2])] + [("edge %d" % e, found[e][0], found[e][1], e) for e in EDGES]
    for name, variant, n, want in cases:
        src = source_of(target, variant, n)
        works = loops.compare(name, src, target, R_SMALL)
        for work in works:                                   # (the first pass of each of the two launches)
            print(name, "queued queries, chunks listed:", chunks_of(work[0, 0]))
            assert chunks_of(work[0, 0]) == (n, want), (name, chunks_of(work[0, 0]))
        listed = passes_equal(name, src, target, R_SMALL, seed=n)
        assert want * 8 >= listed > 0, (name, listed)
    loops.close()


def test_no_query_queued_and_a_second_list_window(lib, target, tmp_path):
    path = str(tmp_path / "tl.bin")
    # ---- none: with the certificate on, a source that stands still queues nothing after its first warm passes (the
    # branch of the round without barriers)
    c = ctx_env({"VISMA_ICP_PERSIST_TIMELINE": path})
    c.set_persistent(True)
    c.set_profiling(1)
    src = source_of(target, 7, 200)
    c.set_clouds_f64(src, target)
    c.get_timing(reset=True)
    T, _ = c.iterate(np.eye(4), R_SMALL, 6)
    tm = c.get_timing(reset=True)
    work = timeline_records(path)[-1]
    queued = [chunks_of(w)[0] for w in work[:, 0]]
    print("queued queries per pass, certificate on:", queued, "| passes of the launch:", tm["persist_passes"])
    # (the source IS a part of the target: the cold pass leaves every query a winner at distance zero and a bound; the
    #  five passes of the launch certify all 200)
    assert tm["persist_launches"] == 1 and tm["persist_passes"] == 5 and tm["persist_aborts"] == 0, tm
    assert len(queued) >= 4 and all(q == 0 for q in queued[:4]), queued
    assert all(int(w) >> 12 == 0 for w in work[:4, 0])
    c.close()
    loops = Loops(tmp_path)
    loops.compare("standstill", src, target, R_SMALL, steps=(6,))
    # ---- above 1,408: 256 queries of one workgroup at a radius whose cells hold ~53 points (7 chunks each)
    src = source_of(target, 8, 256)
    works = loops.compare("second window", src, target, R_BIG)
    assert chunks_of(works[0][0, 0])[0] == 256
    listed = passes_equal("second window", src, target, R_BIG, seed=8)
    print("second window: %d candidates listed by one workgroup: at least %d chunks" % (listed, -(-int(listed) // 8)))
    assert listed > 8 * 1408                                 # (a chunk holds at most 8 candidates)
    loops.close()


@pytest.mark.parametrize("n,r", [(1, R_SMALL), (2, R_SMALL), (63, R_SMALL), (300, R_SMALL), (300, R_BIG), (1000, R_SMALL), (1024, R_SMALL),
                                 (1000, R_BIG)])
def test_one_to_four_workgroups(lib, target, tmp_path, n, r):
    """1 to 1,024 queries: counts that are no multiple of 64, a last workgroup with inactive lanes (300 = 256 + 44; 1,000 =
    3 x 256 + 232), a last wave with one query"""
    src = source_of(target, 20 + n % 7, n)
    listed = passes_equal("n=%d" % n, src, target, r, seed=n)
    assert listed >= n                                       # (every query queued: each lists at least its winner's cell)
    if n >= 3:                                               # (a rigid motion needs three pairs)
        loops = Loops(tmp_path)
        works = loops.compare("n=%d" % n, src, target, r)
        blocks = works[0].shape[1]
        assert blocks == -(-n // 256), (n, blocks)
        queued = sorted(chunks_of(w)[0] for w in works[0][0])
        assert sum(queued) == n and queued[-1] == min(n, 256), (n, queued)
        loops.close()
