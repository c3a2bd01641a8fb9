"""The C++/Eigen shim's estimators constrained to one rotation axis (cicp::TransformationEstimationPointToPointYaw /
PointToPlaneYaw, include/visma_icp_open3d.hpp) and RegisterModelToScene(..., upright = true), through
tests/cpp/axis_driver.cpp compiled in both Eigen storage orders (tests/cpp/build_axis.py)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from visma_amd import synth
from test_axis_solve import AXES, pl_stats, pp_stats, restated, rot

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_axis  # noqa: E402
import build_shim  # noqa: E402

Y = np.array([0.0, 1.0, 0.0])


@pytest.fixture(scope="module")
def bins(lib):
    if build_shim.eigen_dir() is not None:
        build_axis.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_axis.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("axis driver not prebuilt and no Eigen headers here")
    return paths


def run(binary, mode, tmp_path, src, tgt, radius=0.0, iters=0, level=0, init=None, up=Y, tn=None):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    init = np.eye(4) if init is None else np.asarray(init, np.float64)
    with open(inp, "wb") as f:
        f.write(struct.pack("<qqdii", len(src), len(tgt), float(radius), int(iters), int(level)))
        f.write(init.astype("<f8").tobytes())
        f.write(np.asarray(up, "<f8").tobytes())
        f.write(np.ascontiguousarray(src, "<f8").tobytes())
        f.write(np.ascontiguousarray(tgt, "<f8").tobytes())
        if tn is not None:
            f.write(np.ascontiguousarray(tn, "<f8").tobytes())
    p = subprocess.run([binary, mode, inp, outp], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (mode, p.returncode, p.stderr)
    o = np.fromfile(outp, "<f8")
    return dict(T=o[:16].reshape(4, 4), fitness=o[16], rmse=o[17], k=int(o[18]), extra=o[19])


def test_compute_transformation_equals_the_c_abi_and_numpy(lib, bins, tmp_path):
    rng = np.random.default_rng(21)
    for b in bins:
        for k, a in enumerate(AXES[:3] + [np.array([0.3, 1.0, -0.2])]):
            n = 700
            p = rng.standard_normal((n, 3))
            q = p @ rot(a, 0.4 + 0.3 * k).T + rng.standard_normal(3) * 0.1 + rng.standard_normal((n, 3)) * 1e-3
            got = run(b, "solve", tmp_path, p, q, up=a)
            assert np.abs(got["T"] - lib.solve_from_stats_axis(pp_stats(p, q), a)).max() < 1e-12
            assert np.abs(got["T"] - restated(p, q, a)[0]).max() < 1e-12
            assert abs(got["rmse"] - np.sqrt(((p - q) ** 2).sum(1).mean())) < 1e-12
            nr = rng.standard_normal((n, 3))
            nr /= np.linalg.norm(nr, axis=1, keepdims=True)
            got = run(b, "solve_plane", tmp_path, p, q, up=a, tn=nr)
            assert np.abs(got["T"] - lib.solve_from_stats_axis(pl_stats(p, q, nr), a, plane=True)).max() < 1e-12
            an = a / np.linalg.norm(a)
            J4 = np.c_[np.cross(p, nr) @ an, nr]
            y = np.linalg.solve(J4.T @ J4, -(J4.T @ ((p - q) * nr).sum(1)))
            assert np.abs(got["T"][:3, :3] - rot(an, y[0])).max() < 1e-12
            assert np.abs(got["T"][:3, 3] - y[1:]).max() < 1e-12


@pytest.mark.gpu
def test_registration_icp_with_the_yaw_estimators(lib, bins, tmp_path):
    src, tgt, _, r = synth.make_pair(5000, 20000)
    init = synth.make_T(synth.rot_y(0.1), [0.01, 0.0, 0.0])
    ctx = lib.Context(0)
    ctx.set_clouds_f64(src, tgt)
    ctx.set_rotation_axis(Y)
    want = ctx.run(init, r, 20, 0.0, 0.0)
    ctx.close()
    for b in bins:
        got = run(b, "icp_yaw", tmp_path, src, tgt, r, 20, init=init)
        assert got["k"] == want.num_correspondences
        assert np.abs(got["T"] - want.transformation_).max() < 1e-12
        plug = run(b, "plugin", tmp_path, src, tgt, r, 20, init=init)          # the generic plugin loop
        assert plug["k"] == want.num_correspondences
        assert np.abs(plug["T"] - want.transformation_).max() < 1e-9
        around = run(b, "stock_around", tmp_path, src, tgt, r, 20, init=init)   # the axis was cleared behind the call
        assert around["extra"] == 0.0
        assert np.abs(around["T"][:3, :3].T @ Y - Y).max() > 1e-6              # (the stock estimator tilts)


@pytest.mark.gpu
def test_register_model_to_scene_upright(lib, bins, tmp_path):
    src, tgt, _, r = synth.make_pair(3000, 9000)
    for b in bins:
        up = run(b, "upright", tmp_path, src, tgt, r, level=8)
        assert np.abs(up["T"][:3, :3].T @ Y - Y).max() < 1e-12
        free = run(b, "free", tmp_path, src, tgt, r, level=8)
        assert np.abs(free["T"][:3, :3].T @ Y - Y).max() > 1e-6
