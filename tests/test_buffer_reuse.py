"""The engine's buffers (visma_amd/csrc/dev_buf.h: DevPool, DevBuf) across calls of different sizes.

CPU: tests/cpp/dev_buf_driver.cpp -- the pool's rules, reserve / reset, moves, teardown and above all the failure path (an
allocation that fails leaves its buffer empty, so the next call allocates again) against a malloc-backed allocator, under
ASan and UBSan.  The failure path is tested only there.

GPU: one context runs a small registration, a yaw sweep, a batch, a larger registration and the first one again; every
result is bit for bit what the same call gives on a context that has done nothing before it.  The shapes are small on
purpose: what can go wrong is a buffer that is too small, stale or unset after a grow / shrink / grow sequence, and that
shows at any size."""
import os
import subprocess
import sys

import numpy as np
import pytest

from visma_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_dev_buf  # noqa: E402


def test_buffers_and_pool_under_the_sanitizers():
    """tests/cpp/dev_buf_driver.cpp, compiled with -fsanitize=address,undefined: every case passes, nothing leaks (the leak
    check at exit fails the run), nothing is freed twice"""
    exe = build_dev_buf.build()[0]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "all passed" in p.stdout and "FAILED" not in p.stdout and "runtime error" not in p.stderr, (p.stdout, p.stderr)
    assert "ERROR: " not in p.stderr, p.stderr                          # (AddressSanitizer / LeakSanitizer reports)
    assert p.stdout.count(": ok") == 15


def _bits(r):
    return (r.transformation_.view(np.uint64).tolist(), r.iterations, r.nn_passes, r.num_correspondences,
            np.float64(r.fitness_).view(np.uint64), np.float64(r.inlier_rmse_).view(np.uint64))


def _pairs(ctx):
    """source indices, target indices and d2 (as bits) of the context's last pass"""
    si, ti, d2 = ctx.get_correspondences()
    return si.tolist(), ti.tolist(), d2.view(np.uint32).tolist()


@pytest.mark.gpu
def test_one_context_reused_across_sizes_equals_fresh_contexts(lib):
    small = synth.make_pair(300, 1000, seed_t=11, seed_s=12)
    large = synth.make_pair(2000, 8000, seed_t=13, seed_s=14)
    batch = []
    for i in range(3):
        s, t, _, r = synth.make_pair(200, 800, seed_t=20 + i, seed_s=30 + i)
        batch.append((s, t, None, r))

    def single(pair):
        def call(ctx):
            ctx.set_clouds_f64(pair[0], pair[1])
            r = ctx.run(None, pair[3], 12, 0.0, 0.0)
            return [_bits(r)], _pairs(ctx)
        return call

    def sweep(ctx):
        ctx.set_clouds_f64(small[0], small[1])
        best, level, per = ctx.run_yaw_sweep(4, small[3], 12, 0.0, 0.0)
        return [level, _bits(best)] + [_bits(p) for p in per], _pairs(ctx)

    def batched(ctx):
        # (a batch's problems bring their own clouds: the context has no correspondence set of its own to read afterwards)
        return [_bits(r) for r in ctx.run_batch(batch, max_iter=12, rel_fitness=0, rel_rmse=0)], None

    calls = [("300 -> 1000", single(small)), ("yaw sweep of 4", sweep), ("batch of 3", batched),
             ("2000 -> 8000", single(large)), ("300 -> 1000 again", single(small))]
    reused = lib.Context(0)
    try:
        for name, call in calls:
            got = call(reused)
            fresh = lib.Context(0)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert got[0] == want[0], name                  # transformations, iteration and pass counts, K, fitness, rmse
            assert got[1] == want[1], name                  # correspondence indices and d2
            assert got[1] is None or len(got[1][0]) > 0, name
    finally:
        reused.close()
