"""The GPU body of tests/test_warm_kernels.py: one registration's passes through the lane-serial exact search and through
ONE of the two warm search kernels (grid_wave.hip, grid_coop.hip), in one process.  Which of the two serves a single
registration is read from VISMA_ICP_COOP_KERNEL once per process, so the test starts one child per kernel and case and
sets the switch (and VISMA_ICP_GRID_BLOCKS, where a case wants several queries per lane) in the child's environment.
It judges nothing: every assertion lives in the test.

usage: warm_kernel_probe.py in.npz out.npz
in.npz:  src, tgt (f64, n x 3), Ts (passes x 4 x 4), r, plane (0 | 1: point-to-plane over normals estimated here, knn 12)
out.npz: per pass p and context tag in (ref, warm): {tag}_{p}_idx, _d2, _st, _kern; warm_{p}_cand = candidates the warm
         kernel listed in that pass (profiling counters).  Then the last pass once more on the warm context, same
         transform: warm_repeat_cand, warm_repeat_cert = candidates listed, queries certified without a search -- which
         tells the two kernels apart (the wave kernel leaves LB = 0 and certifies nothing).  plane = 1: then the host loop
         of visma_icp_run_point_to_plane, three iterations, on both: {tag}_run (transform, K, fitness, rmse, iterations),
         {tag}_run_idx, _run_d2, _run_kern.

A point-to-plane pass here is visma_icp_reduce_robust with the kernel L2 and plane = 1: with all weights 1 the driver
hands it straight to the engine's reduce(plane = true) (driver.cpp, visma_icp_reduce_robust), which launches the search
with point_to_plane = 1 -- the PLANE instantiation of the kernel under test, whose fused fold gives the statistics."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from visma_amd import _lib  # noqa: E402

SERIAL = {"VISMA_ICP_COOP": "0", "VISMA_ICP_GRID_LANES": "801"}      # lane-serial, one lane per query
WARM = {"VISMA_ICP_GRID_LANES": "9901"}                              # the warm kernel from the first pass (radius pruning)


def make_ctx(env):
    for k in ("VISMA_ICP_COOP", "VISMA_ICP_GRID_LANES"):
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        c = _lib.Context(0)
    finally:
        for k in env:
            os.environ.pop(k, None)
    c.set_nn_mode(_lib.NN_GRID)
    c.set_ring_search(0)                                     # (dense cells would otherwise go to the ring search)
    c.set_persistent(False)
    return c


def one_pass(c, T, r, plane):
    c.nn_pass(T, r)
    return c.reduce_robust("l2", plane=True)[0] if plane else c.reduce()           # (weights 1: the engine's own reduce)


def main():
    fin, fout = sys.argv[1:3]
    cin = np.load(fin)
    src, tgt, Ts, r, plane = cin["src"], cin["tgt"], cin["Ts"], float(cin["r"]), bool(int(cin["plane"]))
    ctxs = (("ref", make_ctx(SERIAL)), ("warm", make_ctx(WARM)))
    nrm = ctxs[0][1].estimate_normals(tgt, knn=12) if plane else None
    for _tag, c in ctxs:
        c.set_clouds_f64(src, tgt)
        if plane:
            c.set_target_normals_f64(nrm)
    ctxs[1][1].set_profiling(True)
    ctxs[1][1].get_timing(reset=True)
    out = {}
    for p, T in enumerate(Ts):
        for tag, c in ctxs:
            st = one_pass(c, T, r, plane)
            key = "%s_%d_" % (tag, p)
            out[key + "idx"], out[key + "d2"], out[key + "st"] = c.correspondence_index(), c.get_correspondences()[2], st
            out[key + "kern"] = np.array(c.search_kernel_used())
        out["warm_%d_cand" % p] = np.array(ctxs[1][1].get_timing(reset=True)["grid_candidates"])
    # the last pass again: nothing moved, so the certificate kernel certifies and the wave kernel searches
    one_pass(ctxs[1][1], Ts[-1], r, plane)
    t = ctxs[1][1].get_timing(reset=True)
    out["warm_repeat_cand"], out["warm_repeat_cert"] = np.array(t["grid_candidates"]), np.array(t["grid_certified"])
    if plane:
        for tag, c in ctxs:
            c.set_device_loop(False)                         # (the host loop, one launch per pass: persistent off above)
            c.forget_winners()
            res = c.run_point_to_plane(None, r, 3, 0.0, 0.0)
            out[tag + "_run"] = np.concatenate([np.asarray(res.transformation_, np.float64).ravel(),
                                                [res.num_correspondences, res.fitness_, res.inlier_rmse_, res.iterations]])
            out[tag + "_run_idx"], out[tag + "_run_d2"] = c.correspondence_index(), c.get_correspondences()[2]
            out[tag + "_run_kern"] = np.array(c.search_kernel_used())
    for _tag, c in ctxs:
        c.close()
    np.savez(fout, **out)
    print("warm_kernel_probe %s: %d passes, %d arrays" % (os.environ.get("VISMA_ICP_COOP_KERNEL", "-"), len(Ts), len(out)))


if __name__ == "__main__":
    main()
