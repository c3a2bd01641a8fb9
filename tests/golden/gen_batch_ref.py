#!/usr/bin/env python3
"""Generate tests/golden/c3_ref.npz and tests/golden/c5_ref.npz: EVERY registration of the batched workloads
(BASELINE config 3: 12 objects x 24 yaw starts = 288; config 5: 192 items x 24 yaw starts = 4,608) run through the
COMPILED REFERENCE (oracle/_ref: Open3D's own RegistrationICP, Registration.cpp:141-186, with its KDTreeFlann), one
call per registration with the reference's default ICPConvergenceCriteria (30 iterations, relative fitness / rmse
1e-6) -- what feh::RegisterModelToScene passes (src/annotation.cpp:29-64).  `pytest -m gpu tests/test_c3_batch.py
tests/test_c5_corpus.py` holds every batched path of the library to these values.

The problems come from where the tests and the benchmark take them (bench.c3_problems(), bench.c5_corpus()); the
fixtures store the recipe's checksums (the clouds come back from visma_amd.synth, a counter-based Philox stream that is
identical on every machine), not the points.

c3_ref.npz, per problem (288): `T` (4 x 4 f64), `k`, `fitness`, `rmse`, `idx_sum` / `idx_wsum` (gen_c4.checksum of the
    reference's final correspondence index); per object (12): `ns`, `nt`, `src_checksum`, `tgt_checksum`.
c5_ref.npz, per item x start (192 x 24): `T` ([:3, :] of the transformation: the last row is constant), `k` (int32),
    `fitness`, `rmse`; per item: `best_level` (annotation.cpp:59: the FIRST start with strictly the most
    correspondences), `margin` = k[best] - max(k[others]) (0: a tie in K, decided by order); per scene (12) and per
    candidate (16): `scene_n` / `cad_n`, `scene_checksum` / `cad_checksum`.
    `yawed_*`: the same arrays for the 24 items of yawed_corpus() (below) -- items whose answer is NOT start 0 -- with
    `yawed_item` (index into the corpus), `yawed_angle` and `yawed_cad_checksum` (the turned candidates).
Both: `cpu_disagree`, the names of the registrations on which the compiled reference and the independent CPU
restatement (oracle.Oracle.registration_icp(grid=True): another search structure, another summation order) differ in K
or by more than 1e-9 in T.  Expected empty; the reference's value is the yardstick either way.  Every stored number is
the reference's f64, unrounded.

    python tests/golden/gen_batch_ref.py [--c3] [--c5] [--out DIR]
                                        (--out: write there instead of tests/golden, to compare two runs)
Runs only where oracle/_ref exists (c3: about 3 minutes on 8 cores, c5: about 15, restatement included); the .npz travel.

A second run repeats every integer array (K, the correspondence checksums, best_level, margin) and the fitness bit for
bit, NOT the transformations and the rmse: the reference merges its threads' correspondence lists and sums in the
order the threads arrive (Registration.cpp:54-82, an OpenMP critical section), so the order of its sums differs from
run to run.  Two runs on 8 cores differed by at most 3.8e-15 (relative Frobenius of T) and 9.1e-15 (relative rmse)
over the 288 + 4,608 + 576 registrations: six orders inside the 1e-9 the GPU is held to."""
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from gen_c4 import checksum, input_checksum  # noqa: E402
from visma_amd import synth  # noqa: E402

LEVEL, MAX_ITER = 24, 30
C3_RADIUS, C5_RADIUS = 0.02, 0.05
SIZE_BOUND = 717187                        # tests/golden/live_checks.npz, the largest fixture before these


def first_strictly_most(k):
    """annotation.cpp:59-61: `if (k > best.k)` over the starts in order, from a default result with K = 0."""
    best, level = 0, -1
    for i, v in enumerate(k):
        if v > best:
            best, level = int(v), i
    return level


def margin_of(k, level):
    others = [int(v) for i, v in enumerate(k) if i != level]
    return int(k[level]) - max(others)


def start(level_index, level=LEVEL):
    """The initial transformation of one yaw start (annotation.cpp:35-43): AngleAxis(2 pi i / level, UnitY)."""
    return synth.make_T(synth.rot_y(2 * np.pi * level_index / level), [0, 0, 0])


def yawed_corpus(scenes, cads, items):
    """24 items of the corpus (item 9 j mod 192, j = 0..23: scenes and candidates vary) whose candidate is turned about
    Y by -(2 pi j / 24 + 0.03) before it is handed over, so that start j is the one that lands: the corpus itself has
    its candidates within 0.05 rad of the scene's yaw, where every item's best start is 0.
    -> list of (item index, angle, turned candidate (float32-rounded f64, like every cloud here), scene)"""
    out = []
    for j in range(LEVEL):
        i = (9 * j) % len(items)
        s, c = items[i]
        a = -(2 * math.pi * j / LEVEL + 0.03)
        cad = (cads[c] @ synth.rot_y(a).T).astype(np.float32).astype(np.float64)
        out.append((i, a, cad, scenes[s]))
    return out


class Table:
    """reference against restatement over one set of registrations"""

    def __init__(self, name):
        self.name, self.n, self.kd, self.fd, self.k3, self.wt, self.wr = name, 0, 0, 0, 0, 0.0, 0.0
        self.disagree = []

    def add(self, what, r, o):
        self.n += 1
        bad = r.k != o.k
        self.kd += bad
        self.fd += np.float64(r.fitness).view(np.uint64) != np.float64(o.fitness).view(np.uint64)
        self.k3 += r.k < 3
        if r.k >= 3:
            e = synth.rel_frobenius(o.T, r.T)
            self.wt = max(self.wt, e)
            bad = bad or not e <= 1e-9
        if r.rmse > 0:
            self.wr = max(self.wr, abs(o.rmse - r.rmse) / r.rmse)
        if bad:
            self.disagree.append(what)

    def show(self):
        print("| set | registrations | K differs | fitness differs (bits) | K < 3 | worst rel. Frobenius of T | worst rel. rmse difference |")
        print("|---|---|---|---|---|---|---|")
        print("| %s | %d | %d | %d | %d | %.1e | %.1e |" % (self.name, self.n, self.kd, self.fd, self.k3, self.wt, self.wr))
        for d in self.disagree:
            print("  the CPU implementations disagree on", d)


def both(ref, orc, src, tgt, r, init):
    w = ref.registration_icp(src, tgt, r, init=init, max_iter=MAX_ITER)
    o = orc.registration_icp(src, tgt, r, init=init, max_iter=MAX_ITER, grid=True)
    return w, o


def gen_c3(ref, orc):
    from bench import c3_problems
    objs, probs = c3_problems()
    assert len(objs) == 12 and len(probs) == 12 * LEVEL
    n = len(probs)
    T = np.empty((n, 4, 4)); k = np.empty(n, np.int64); fit = np.empty(n); rmse = np.empty(n)
    s1 = np.empty(n, np.int64); s2 = np.empty(n, np.int64)
    tab = Table("C3, all")
    for i, (src, tgt, init, r, oi) in enumerate(probs):
        assert r == C3_RADIUS and oi == i // LEVEL and np.array_equal(init, start(i % LEVEL))
        w, o = both(ref, orc, src, tgt, r, init)
        tab.add("object %d start %d (%d -> %d)" % (oi, i % LEVEL, len(src), len(tgt)), w, o)
        a, b, kk = checksum(w.idx)
        assert kk == w.k
        T[i], k[i], fit[i], rmse[i], s1[i], s2[i] = w.T, w.k, w.fitness, w.rmse, a, b
    tab.show()
    return dict(T=T, k=k, fitness=fit, rmse=rmse, idx_sum=s1, idx_wsum=s2,
                ns=np.array([len(s) for s, _ in objs], np.int64), nt=np.array([len(t) for _, t in objs], np.int64),
                src_checksum=np.array([input_checksum(s) for s, _ in objs], np.uint64),
                tgt_checksum=np.array([input_checksum(t) for _, t in objs], np.uint64),
                radius=C3_RADIUS, level=LEVEL, max_iter=MAX_ITER, cpu_disagree=np.array(tab.disagree, dtype="U64"))


def sweep_set(ref, orc, name, pairs, names):
    """every start of every (candidate, scene) pair -> the per-start arrays, best_level, margin"""
    n = len(pairs)
    T = np.empty((n, LEVEL, 3, 4)); k = np.empty((n, LEVEL), np.int32)
    fit = np.empty((n, LEVEL)); rmse = np.empty((n, LEVEL))
    best = np.empty(n, np.int32); margin = np.empty(n, np.int32)
    tab = Table(name)
    t0 = time.time()
    for i, (cad, scene) in enumerate(pairs):
        for j in range(LEVEL):
            w, o = both(ref, orc, cad, scene, C5_RADIUS, start(j))
            tab.add("%s start %d (%d -> %d)" % (names[i], j, len(cad), len(scene)), w, o)
            assert np.array_equal(w.T[3], [0, 0, 0, 1])
            T[i, j], k[i, j], fit[i, j], rmse[i, j] = w.T[:3], w.k, w.fitness, w.rmse
        best[i] = first_strictly_most(k[i])
        margin[i] = margin_of(k[i], best[i])
        if (i + 1) % 16 == 0:
            print("  %s: %d / %d items (%.0f s)" % (name, i + 1, n, time.time() - t0), flush=True)
    tab.show()
    return dict(T=T, k=k, fitness=fit, rmse=rmse, best_level=best, margin=margin), tab.disagree


def gen_c5(ref, orc):
    from bench import c5_corpus
    scenes, cads, items = c5_corpus()
    assert len(items) == 192
    # the short set first: its claim (the answer is not start 0) is checked before the long run
    yawed = yawed_corpus(scenes, cads, items)
    y, ydis = sweep_set(ref, orc, "C5 yawed, all", [(cad, scene) for _, _, cad, scene in yawed],
                        ["yawed item %d (corpus item %d)" % (j, yi[0]) for j, yi in enumerate(yawed)])
    print("yawed best_level:", y["best_level"].tolist(), "margins:", y["margin"].tolist())
    assert len(set(y["best_level"].tolist())) >= 12, "the yawed items do not spread over the starts"
    assert int((y["best_level"] != 0).sum()) >= 20, "too many yawed items still answer start 0"
    a, dis = sweep_set(ref, orc, "C5, all", [(cads[c], scenes[s]) for s, c in items],
                       ["item %d (scene %d, candidate %d)" % (i, s, c) for i, (s, c) in enumerate(items)])
    print("best_level 0 for %d of %d items, ties in K: %d (yawed: %d)" % (
        int((a["best_level"] == 0).sum()), len(items), int((a["margin"] == 0).sum()), int((y["margin"] == 0).sum())))
    out = dict(a)
    out.update({"yawed_" + key: v for key, v in y.items()})
    out.update(yawed_item=np.array([yi[0] for yi in yawed], np.int32), yawed_angle=np.array([yi[1] for yi in yawed]),
               yawed_cad_checksum=np.array([input_checksum(yi[2]) for yi in yawed], np.uint64),
               scene_n=np.array([len(s) for s in scenes], np.int64), cad_n=np.array([len(c) for c in cads], np.int64),
               scene_checksum=np.array([input_checksum(s) for s in scenes], np.uint64),
               cad_checksum=np.array([input_checksum(c) for c in cads], np.uint64),
               radius=C5_RADIUS, level=LEVEL, max_iter=MAX_ITER, cpu_disagree=np.array(dis + ydis, dtype="U64"))
    return out


def main():
    from oracle.oracle import Oracle, Ref
    ref, orc = Ref(), Oracle()
    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    for flag, name, gen in (("--c3", "c3_ref.npz", gen_c3), ("--c5", "c5_ref.npz", gen_c5)):
        if flag not in sys.argv:
            continue
        t0 = time.time()
        out = gen(ref, orc)
        path = os.path.join(out_dir, name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("wrote %s (%d bytes) in %.0f s" % (path, size, time.time() - t0), flush=True)
        assert size < SIZE_BOUND, "larger than the largest fixture committed before"


if __name__ == "__main__":
    main()
