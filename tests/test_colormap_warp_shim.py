"""The stand-alone Open3D header set of the non-rigid color map optimization: tests/cpp/colormap_warp_driver.cpp compiles
against it in both Eigen storage orders; cicp::ColorMapOptimizationNonRigid on a TriangleMesh and on a PointCloud -- with the
option's flag set and not set -- equals the staged calls of visma_icp.h bit for bit and the fixture's extrinsics and colours
after 8 iterations at the tolerances of tests/test_colormap_warp_gpu.py; ColorMapOptimization with the flag set still throws
std::invalid_argument, names the new function and touches nothing."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import colormap_warp_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_colormap_warp  # noqa: E402

ANCHORS = 5


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_colormap_warp.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_colormap_warp.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("colormap warp driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_colormap_warp.build()
    assert outs and all(os.path.exists(p) for p in outs)


@pytest.mark.gpu
def test_shim_equals_the_staged_calls_and_the_reference(lib, driver_bins, tmp_path):
    g = cases.golden()
    depths, colors, E, K, V = cases.inputs()
    n, h, w = depths.shape
    key = "a%d_" % ANCHORS
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii4dii2d", w, h, *[float(v) for v in K], n, len(V), 8.0, cases.scene.scene.MAX_DEPTH))
        f.write(struct.pack("<id", ANCHORS, float(g[key + "weight"])))
        for i in range(n):
            f.write(np.ascontiguousarray(E[i], "<f8").tobytes()); f.write(np.ascontiguousarray(depths[i], "<f4").tobytes())
            f.write(np.ascontiguousarray(colors[i], np.uint8).tobytes())
        f.write(np.ascontiguousarray(V, "<f8").tobytes())
    tol = 100.0 * float(g[key + "pose_spread"])
    results = []
    for b in driver_bins:
        p = subprocess.run([b, inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        out = np.frombuffer(open(outp, "rb").read(), "<f8")
        assert len(out) == 3 * (16 * n + 3 * len(V)) + 1
        at = 0
        for _ in ("a mesh on the caller's context", "a cloud on the thread's context, the flag set", "the staged calls"):
            Eo = out[at:at + 16 * n].reshape(n, 4, 4); at += 16 * n
            col = out[at:at + 3 * len(V)].reshape(len(V), 3); at += 3 * len(V)
            assert np.abs(Eo - g[key + "extr_8"]).max() <= tol
            assert np.abs(col - g[key + "colors_8"]).max() <= 1e-15
            results.append((Eo, col))
        assert out[at] == 1.0                                         # the old function threw, named the new one, touched nothing
    for Eo, col in results[1:]:                                       # one computation, whichever carrier, flag and storage order
        assert np.array_equal(Eo.view(np.uint64), results[0][0].view(np.uint64)) and np.array_equal(col.view(np.uint64), results[0][1].view(np.uint64))
