"""The stand-alone Open3D header set of RGB-D odometry (include/Core/Geometry/Image.h, RGBDImage.h,
Camera/PinholeCameraIntrinsic.h, Odometry/*.h): tests/cpp/odometry_driver.cpp compiles against it in both Eigen storage
orders, and cicp::ComputeRGBDOdometry returns what the C ABI returns, bit for bit."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_odometry  # noqa: E402


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_odometry.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_odometry.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("odometry driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_odometry.build()
    assert outs and all(os.path.exists(p) for p in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1])
def test_shim_equals_the_c_abi_bit_for_bit(lib, driver_bins, tmp_path, method):
    g = np.load(os.path.join(HERE, "golden", "odometry.npz"))
    fr = [g["a_" + k] for k in ("src_gray", "src_depth", "tgt_gray", "tgt_depth")]
    k, init, o = g["a_intrinsic"], g["a_init"], g["a_option"]
    its = [int(i) for i in (g["a_iterations"] if method == 1 else g["a_color_iterations"])]
    h, w = fr[0].shape
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<iiii%di" % len(its), w, h, method, len(its), *its))
        f.write(struct.pack("<3d", *[float(v) for v in o]))
        f.write(np.ascontiguousarray(k, "<f8").tobytes()); f.write(np.ascontiguousarray(init, "<f8").tobytes())
        for a in fr:
            f.write(np.ascontiguousarray(a, "<f4").tobytes())
    ctx = lib.Context(0)
    try:
        want = ctx.rgbd_odometry(*fr, k, init, method, lib.odometry_option(its, float(o[0]), float(o[1]), float(o[2])))
    finally:
        ctx.close()
    assert want.success
    for b in driver_bins:
        p = subprocess.run([b, inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        v = np.frombuffer(open(outp, "rb").read(), "<f8").reshape(3, 53)
        for call in v[:2]:                                            # a context of its own, the thread's context
            assert call[0] == 1.0
            assert call[1:17].tobytes() == want.T.tobytes() and call[17:].tobytes() == want.information.tobytes()
        assert v[2][0] == 0.0 and np.array_equal(v[2][1:17].reshape(4, 4), np.eye(4)) and np.all(v[2][17:] == 0.0)    # a size mismatch
