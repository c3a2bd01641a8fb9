"""open3d::TSDFVolume::ExtractTriangleMesh of the stand-alone header set (include/Core/Integration/): tests/cpp/tsdf_mesh_driver.cpp
compiles against it in both Eigen storage orders; on u21 (each colour type) and on a scalable case the shim's meshes equal,
to the bit and the index, what the C ABI gives for the same frames (tests/test_tsdf_mesh.py pins that to the
specification), and cicp::ColorMapOptimization takes the mesh."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import tsdf_mesh_cases as cases
import tsdf_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_tsdf_mesh  # noqa: E402


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_tsdf_mesh.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_tsdf_mesh.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("tsdf mesh driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_tsdf_mesh.build()
    assert outs and all(os.path.exists(p) for p in outs)


class Cursor:
    def __init__(self, v):
        self.v, self.at = v, 0

    def take(self, n):
        out = self.v[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out

    def mesh(self):
        nv, nc, nt = [int(v) for v in self.take(3)]
        return (self.take(3 * nv).reshape(nv, 3).copy(), self.take(3 * nc).reshape(nc, 3).copy() if nc else None,
                self.take(3 * nt).astype(np.int32).reshape(nt, 3))


def same_mesh(a, b):
    for x, y in zip(a, b):
        if (x is None) != (y is None):
            return False
        if x is not None and x.tobytes() != y.tobytes():
            return False
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("t", [S.COLOR_NONE, S.COLOR_RGB8, S.COLOR_GRAY32])
def test_shim_meshes_equal_the_c_abi(lib, driver_bins, tmp_path, t):
    uniform = dict(cases.load("u21"), color_type=t)
    scalable = cases.load({S.COLOR_RGB8: "s0", S.COLOR_GRAY32: "s1", S.COLOR_NONE: "s2"}[t])
    frames = uniform["frames"]
    h, w = frames[0][0].shape
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii4di", w, h, *[float(v) for v in uniform["intrinsic"]], len(frames)))
        f.write(struct.pack("<ii5d", uniform["R"], t, uniform["length"], uniform["sdf_trunc"], *uniform["origin"]))
        for depth, rgb, gray, E in frames:
            f.write(np.ascontiguousarray(E, "<f8").tobytes()); f.write(np.ascontiguousarray(depth, "<f4").tobytes())
            f.write(np.ascontiguousarray(rgb, np.uint8).tobytes()); f.write(np.ascontiguousarray(gray, "<f4").tobytes())
        f.write(struct.pack("<iiii2d", scalable["R"], scalable["stride"], scalable["color_type"], len(scalable["frames"]),
                            scalable["voxel_length"], scalable["sdf_trunc"]))
    ctx = lib.Context(0)
    want = []
    for case in (uniform, scalable):
        vol = cases.lib_volume(ctx, case)
        want.append(vol.extract_triangle_mesh())
        assert len(want[-1][2]) > 0
        vol.close()
    ctx.close()
    for b in driver_bins:
        p = subprocess.run([b, inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        c = Cursor(np.frombuffer(open(outp, "rb").read(), "<f8"))
        assert same_mesh(c.mesh(), want[0]), b
        assert c.take(1)[0] == 1.0, p.stderr                          # ColorMapOptimization took the mesh
        assert same_mesh(c.mesh(), want[1]), b
        assert c.at == len(c.v)
