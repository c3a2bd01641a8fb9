#!/usr/bin/env python
"""Times of the NON-RIGID color map optimization on one MI355X, for profiles/colormap_warp_probe.txt: the workload of
tools/colormap_probe.py (50 cameras of 640 x 480, 1,000,000 vertices, Open3D's default option: 16 vertical anchors, a field of
21 x 16 anchors and 678 unknowns per camera).
  * prepare: images, masks, visibility (one-time), and the sort's buffers;
  * cell_sums: keys, sort (histogram, scan, scatter) and reduce over every camera and the read-back of the 50 x 300 rows of
    121, the proxies being valid: five launches and one wait;
  * keys, sort, reduce: the kernels' own times, from a second run of the same child under `rocprofv3 --kernel-trace --stats`
    (a run of its own, fewer calls: its wall clock is not used), the average per launch with min .. max;
  * read_back: cell_sums' median less the five kernels' averages: the copy of the rows (their bytes are printed), the
    launches and the wait;
  * proxy: the poses' and the fields' upload and the warped proxy kernel;
  * proxy+cell_sums: the device side of one iteration in one call;
  * step: one whole iteration = that + the 50 banded solves on up to 16 host threads and the updates;
    host_solve_ms_per_iteration is the step's median less the median of proxy+cell_sums;
  * solve_one_camera: visma_icp_color_map_solve_non_rigid on one camera's rows, one thread;
  * run300: a whole 300-iteration run from the perturbed poses and the initial fields (as many of --run-reps calls as fit
    into two minutes, at least 3: the number is printed).
The times are the wall clock of the Python call (each ends with the device idle); the spread (min .. max) is printed beside
every median and belongs to it.  tests/golden/gen_colormap_warp.py --time times the compiled reference on the same input.
The measurement runs in a child process under its own time limit; one warm-up call, then the median and the spread of
--reps calls (default 20)."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from colormap_probe import H, N_CAMERAS, N_VERTICES, W, timed, workload  # noqa: E402,F401


def child(reps, n_cameras, n_vertices, run_reps):
    from visma_amd import _lib
    depths, colors, E, K, V = workload(n_cameras, W, H, n_vertices)
    ctx = _lib.Context(0)
    m = ctx.color_map_non_rigid(W, H, n_cameras, K, _lib.color_map_option())
    for i in range(n_cameras):
        m.set_image(i, depths[i], colors[i], E[i])
    m.set_vertices(V)
    aw, ah, step = m.anchor_shape()
    out = {"case": "%d cameras of %d x %d, %d vertices, %d x %d anchors" % (n_cameras, W, H, len(V), aw, ah), "reps": reps}
    t, counts = timed(m.prepare, 3)
    out["prepare"] = dict(t, visible_pairs=int(counts.sum()), most_per_camera=int(counts.max()))
    F0 = m.flow()
    m.cell_sums()
    t, rows = timed(m.cell_sums, reps)
    out["cell_sums"] = dict(t, accepted=int(rows[:, :, 120].sum()), cells_with_visits=int((rows[:, :, 120] > 0).sum()), read_back_bytes=int(rows.nbytes))

    def reset():
        m.set_extrinsics(E)
        m.set_flow(F0)

    def proxy():
        reset()
        return m.proxy()
    tp, _ = timed(proxy, reps)
    out["proxy"] = tp

    def proxy_and_sums():
        reset()
        return m.cell_sums()
    tps, _ = timed(proxy_and_sums, reps)
    out["proxy+cell_sums"] = tps

    def step():
        reset()
        return m.step_non_rigid()
    ts, _ = timed(step, reps)
    out["step"] = dict(ts, host_solve_ms_per_iteration=ts["median_ms"] - tps["median_ms"])
    t1, _ = timed(lambda: _lib.color_map_solve_non_rigid(aw, ah, rows[0], len(V), 0.316, F0[0], F0[0]), reps)
    out["solve_one_camera"] = t1

    def run300():
        reset()
        return m.run(300)
    t0 = time.perf_counter()
    run300()
    run_reps = max(3, min(run_reps, int(120.0 / max(time.perf_counter() - t0, 1e-3))))
    tr, res = timed(run300, run_reps)
    out["run300"] = dict(tr, reps=run_reps, residual_first=float(res[0]), residual_last=float(res[-1]))
    tc, _ = timed(m.colors, reps)
    out["colors"] = tc
    m.close()
    ctx.close()
    print("RESULT " + json.dumps(out))


KERNELS = (("keys", ("cm_warp_keys_kernel",)), ("sort", ("cm_warp_hist_kernel", "cm_warp_scan_kernel", "cm_warp_scatter_kernel")),
           ("reduce", ("cm_warp_reduce_kernel",)))


def kernel_split(a):
    """the child again under a kernel trace -> {stage: (average, min, max) in ms per launch, summed over the stage's kernels}, or a
    string that says why there is none"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return "no rocprofv3 here"
    d = tempfile.mkdtemp(prefix="warp_trace_")
    try:
        p = subprocess.run(["timeout", "-k", "10", "400", exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                            os.path.abspath(__file__), "--child", "--reps", "3", "--run-reps", "3", "--cameras", str(a.cameras), "--vertices",
                            str(a.vertices)], capture_output=True, text=True)
        if p.returncode != 0:
            return "the traced run ended with %d" % p.returncode
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return "the trace wrote no kernel statistics"
        rows = list(csv.DictReader(open(files[0])))
        out = {}
        for stage, names in KERNELS:
            tot = [0.0, 0.0, 0.0]
            for n in names:
                hit = [r for r in rows if n in r.get("Name", "")]
                if not hit:
                    return "no %s in the trace" % n
                for k, col in enumerate(("AverageNs", "MinNs", "MaxNs")):
                    tot[k] += float(hit[0][col]) * 1e-6
            out[stage] = tuple(tot)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run-reps", type=int, default=20)
    ap.add_argument("--cameras", type=int, default=N_CAMERAS)
    ap.add_argument("--vertices", type=int, default=N_VERTICES)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colormap_warp_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.cameras, a.vertices, a.run_reps)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                        "--run-reps", str(a.run_reps), "--cameras", str(a.cameras), "--vertices", str(a.vertices)], capture_output=True, text=True)
    if p.returncode != 0:
        print("exit %d\n%s" % (p.returncode, p.stderr[-2000:]))
        return 1
    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    res = json.loads(lines[-1])
    text = ["# tools/colormap_warp_probe.py: %s, median of %d calls after one warm-up (min .. max), wall clock of the Python call" % (res["case"], res["reps"])]
    for k, v in res.items():
        if isinstance(v, dict):
            extra = ", ".join("%s %s" % (a_, ("%.4g" % b) if isinstance(b, float) else b) for a_, b in v.items() if a_ not in ("median_ms", "min_ms", "max_ms"))
            text.append("%-16s %10.3f ms (%.3f .. %.3f)%s" % (k, v["median_ms"], v["min_ms"], v["max_ms"], "  " + extra if extra else ""))
    split = kernel_split(a)
    if isinstance(split, str):
        text.append("keys / sort / reduce / read_back: not measured (%s)" % split)
    else:
        for stage, (avg, lo, hi) in split.items():
            text.append("%-16s %10.3f ms (%.3f .. %.3f)  kernel time per launch, a traced run of its own" % (stage, avg, lo, hi))
        text.append("%-16s %10.3f ms  cell_sums' median less the kernels' averages: the rows' copy, five launches, one wait" %
                    ("read_back", res["cell_sums"]["median_ms"] - sum(v[0] for v in split.values())))
    text.append(lines[-1])
    print("\n".join(text))
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
