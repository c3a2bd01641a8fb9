"""The stand-alone Open3D header set of color map optimization (include/Core/ColorMap/ColorMapOptimization.h,
Core/Camera/PinholeCameraTrajectory.h, Core/Geometry/TriangleMesh.h): tests/cpp/colormap_driver.cpp compiles against it in
both Eigen storage orders, and cicp::ColorMapOptimization on a TriangleMesh and on a PointCloud gives the extrinsics and
colours of tests/golden/colormap.npz after 8 iterations at the tolerances of tests/test_colormap.py; the non-rigid option
throws std::invalid_argument and touches nothing."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import colormap_scene as scene
from test_colormap import bits

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_colormap  # noqa: E402


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_colormap.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_colormap.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("colormap driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_colormap.build()
    assert outs and all(os.path.exists(p) for p in outs)


@pytest.mark.gpu
def test_shim_gives_the_reference(lib, driver_bins, tmp_path):
    g = np.load(os.path.join(HERE, "golden", "colormap.npz"))
    depths, colors, E, K = scene.frames()
    V = scene.vertices()
    n, h, w = depths.shape
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii4dii2d", w, h, *[float(v) for v in K], n, len(V), 8.0, scene.MAX_DEPTH))
        for i in range(n):
            f.write(np.ascontiguousarray(E[i], "<f8").tobytes()); f.write(np.ascontiguousarray(depths[i], "<f4").tobytes())
            f.write(np.ascontiguousarray(colors[i], np.uint8).tobytes())
        f.write(np.ascontiguousarray(V, "<f8").tobytes())
    tol = 100.0 * float(g["pose_spread"])
    results = []
    for b in driver_bins:
        p = subprocess.run([b, inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        out = np.frombuffer(open(outp, "rb").read(), "<f8")
        assert len(out) == 2 * (16 * n + 3 * len(V)) + 1
        at = 0
        for _ in ("a mesh on the caller's context", "a cloud on the thread's context"):
            Eo = out[at:at + 16 * n].reshape(n, 4, 4); at += 16 * n
            col = out[at:at + 3 * len(V)].reshape(len(V), 3); at += 3 * len(V)
            assert np.abs(Eo - g["extr_8"]).max() <= tol
            assert np.abs(col - g["colors_8"]).max() <= 1e-15
            results.append((Eo, col))
        assert out[at] == 1.0                                         # the non-rigid option threw and touched nothing
    for Eo, col in results[1:]:                                       # one computation, whichever carrier and storage order
        assert np.array_equal(bits(Eo), bits(results[0][0])) and np.array_equal(bits(col), bits(results[0][1]))
