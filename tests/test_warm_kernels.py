"""BOTH warm search kernels on a SINGLE registration, each against the lane-serial exact search, bit for bit:
correspondence indices, distance bits and all 38 statistics of three passes (identity, then two small random motions, so
that the warm state is read).  The launcher hands single registrations to the certificate kernel (grid_coop.hip) and
batches and sweeps to the wave kernel (grid_wave.hip); VISMA_ICP_COOP_KERNEL = cert | wave forces either, and is read
once per process -- so every case runs in a child of its own (tools/warm_kernel_probe.py), one at a time, under a time
limit.  The cases reach what the wave kernel otherwise meets only through batches: its dense-list windows, its whole-wave
re-scan (six copies of every target point), its several-queries-per-lane instantiation and its PLANE instantiations
(tools/warm_kernel_probe.py says how a single pass is made a point-to-plane pass)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from visma_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "warm_kernel_probe.py")


def rand_T(rng, ang, tr):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(0, ang)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = rng.normal(size=3) * tr
    return T


def passes(rng, T_gt, r):
    return np.stack([np.eye(4), T_gt @ rand_T(rng, r * 0.8, r * 0.5), T_gt @ rand_T(rng, r * 0.8, r * 0.5)])


def plain(rng):
    src, tgt, T_gt, r = synth.make_pair(2000, 8000, motion="radius")
    return src, tgt, T_gt, r


def seven_targets(rng):
    src, tgt, T_gt, _ = synth.make_pair(300, 7, motion="radius")
    return src, tgt, T_gt, 0.5


def exact_ties(rng, copies=4):
    """1500 target points, each given four times, in shuffled order: the flagged candidates of a query are copies of one
    another.  Four copies fit the four slots of the f64 ranking: the whole-wave re-scan runs only where they straddle three
    chunks or another point lies in the band."""
    src, tgt, T_gt, r = synth.make_pair(1500, 1500, motion="radius")
    tgt = np.concatenate([tgt] * copies)[rng.permutation(copies * len(tgt))]
    return src, tgt, T_gt, r


def exact_ties_six(rng):
    """... each given SIX times: the copies of the nearest point share its cell and its fp32 distance, so every query with
    a partner has six flagged candidates in two kept chunks (more than the four slots) or a third chunk at the minimum:
    every one of them goes through the whole-wave re-scan, by construction."""
    return exact_ties(rng, 6)


DENSE_R = 0.05


def dense_lists(rng):
    """200 cluster centres, 80 target points each within 2 % of the cell edge of their centre; 1024 sources near the
    centres: more than 8 chunks per query, which overflows one list window of either kernel (512 chunk descriptors per
    64 queries in the wave kernel, 4 x 352 per 256 queries in the certificate kernel)."""
    centres = rng.uniform(0.0, 0.3, size=(200, 3))
    tgt = (centres[:, None, :] + rng.normal(size=(200, 80, 3)) * (0.02 * DENSE_R)).reshape(-1, 3)
    src = centres[np.arange(1024) % 200] + rng.normal(size=(1024, 3)) * (0.05 * DENSE_R)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return f32(src), f32(tgt), np.eye(4), DENSE_R


# name, clouds, point-to-plane, environment of the child on top of the kernel switch
CASES = [
    ("plain", plain, 0, {}),
    ("plain point-to-plane", plain, 1, {}),
    ("seven targets", seven_targets, 0, {}),
    ("exact ties", exact_ties, 0, {}),
    ("exact ties, six copies", exact_ties_six, 0, {}),
    ("dense lists", dense_lists, 0, {}),
    # 2000 queries on 2 workgroups = 512 lanes (kernels.h: search_blocks caps the workgroups of lanes code 9901 like every
    # other): four queries per lane, the _many kernels
    ("several queries per lane", plain, 0, {"VISMA_ICP_GRID_BLOCKS": "2"}),
    ("several queries per lane point-to-plane", plain, 1, {"VISMA_ICP_GRID_BLOCKS": "2"}),
]


def run_probe(tmp_path, arrays, env, timeout=120):
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, **arrays)
    e = dict(os.environ)
    for k in ("VISMA_ICP_COOP", "VISMA_ICP_GRID_LANES", "VISMA_ICP_GRID_BLOCKS", "VISMA_ICP_COOP_KERNEL"):
        e.pop(k, None)
    e.update(env)
    # (every child under a time limit of its own)
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, PROBE, fin, fout], capture_output=True, text=True,
                       timeout=timeout + 30, cwd=ROOT, env=e)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return dict(np.load(fout))


@pytest.mark.parametrize("kernel", ["wave", "cert"])
@pytest.mark.parametrize("name,clouds,plane,env", CASES, ids=[c[0] for c in CASES])
def test_each_warm_kernel_equals_the_lane_serial_search_on_one_registration(lib, tmp_path, kernel, name, clouds, plane, env):
    rng = np.random.default_rng(20 + len(name))
    src, tgt, T_gt, r = clouds(rng)
    Ts = passes(rng, T_gt, r)
    got = run_probe(tmp_path, {"src": src, "tgt": tgt, "Ts": Ts, "r": np.array(r), "plane": np.array(plane)},
                    dict(env, VISMA_ICP_COOP_KERNEL=kernel))
    for p in range(len(Ts)):
        ref, warm = "ref_%d_" % p, "warm_%d_" % p
        assert str(got[ref + "kern"]) == "serial" and str(got[warm + "kern"]) == "warm", (name, kernel, p)
        i0 = got[ref + "idx"]
        print("%s / %s pass %d: %d pairs, %.1f candidates per query" % (name, kernel, p, int((i0 >= 0).sum()),
                                                                       float(got[warm + "cand"]) / len(src)))
        assert np.array_equal(got[warm + "idx"], i0), (name, kernel, p)
        assert np.array_equal(got[warm + "d2"].view(np.uint32), got[ref + "d2"].view(np.uint32)), (name, kernel, p)
        assert np.array_equal(got[warm + "st"].view(np.uint64), got[ref + "st"].view(np.uint64)), (name, kernel, p)
        if name.startswith("exact ties"):
            # the lowest original index among the copies of the winner
            hit = i0 >= 0
            assert hit.any()
            _, first = np.unique(tgt, axis=0, return_index=True)        # (sorted unique rows; first occurrence of each)
            lowest = {tgt[j].tobytes(): j for j in first}
            assert all(lowest[tgt[j].tobytes()] == j for j in i0[hit]), (name, kernel, p)
        if name == "dense lists":
            # (so that a change to the clouds or to the grid cannot quietly empty the case: more than 8 chunks per query)
            assert float(got[warm + "cand"]) / len(src) > 80.0, (name, kernel, p)
    # ---- which kernel ran: the last pass again, nothing moved.  The wave kernel leaves LB = 0 and certifies nothing: it
    # searches every query again (at least the winner is listed).  The certificate kernel certifies every query whose
    # winner was decided without a near-tie -- in the clouds of distinct random points, nearly all.
    pairs = int((got["ref_%d_idx" % (len(Ts) - 1)] >= 0).sum())
    cert, cand = float(got["warm_repeat_cert"]), float(got["warm_repeat_cand"])
    print("%s / %s the last pass again: %d certified, %d candidates listed, %d pairs" % (name, kernel, cert, cand, pairs))
    if kernel == "wave":
        assert cert == 0 and cand >= pairs, (name, kernel)
    elif name not in ("seven targets", "exact ties", "exact ties, six copies"):
        assert cert > len(src) // 2, (name, kernel)
    if plane:
        # the statistics above have the point-to-plane layout (J^T J, J^T r; the nine q p^T sums of the closed form
        # absent): they came from a PLANE fold
        st = got["warm_1_st"]
        assert np.all(st[29:] == 0.0) and np.all(st[2:29] != 0.0), (name, kernel)
        # and the host loop of the point-to-plane estimator, three iterations, one launch per pass: statistics that are
        # bit-identical pass by pass give the same solves, so every bit of the result is the lane-serial context's
        assert str(got["ref_run_kern"]) == "serial" and str(got["warm_run_kern"]) == "warm", (name, kernel)
        assert np.array_equal(got["warm_run"].view(np.uint64), got["ref_run"].view(np.uint64)), (name, kernel)
        assert np.array_equal(got["warm_run_idx"], got["ref_run_idx"]), (name, kernel)
        assert np.array_equal(got["warm_run_d2"].view(np.uint32), got["ref_run_d2"].view(np.uint32)), (name, kernel)
