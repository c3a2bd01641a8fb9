"""The stand-alone Open3D header set of TSDF integration (include/Core/Integration/TSDFVolume.h, UniformTSDFVolume.h and
the point-cloud factories next to Core/Geometry/RGBDImage.h): tests/cpp/tsdf_driver.cpp compiles against it in both Eigen
storage orders, and the shim's classes on case U21 of tests/golden/tsdf.npz give what tests/test_tsdf.py reads from the C
ABI: the reference's volumes, extractions and point clouds; and open3d::ScalableTSDFVolume on case s0 (RGB8 volumes) or s1
(Gray32) or s2 (no colour) gives the fixture's unit sets, units and extractions."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import tsdf_spec as S
from test_tsdf import N_FRAMES, check_extraction, check_scalable_extraction, check_units, check_volume, frames_of, s_config, same_bits

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_tsdf  # noqa: E402


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_tsdf.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_tsdf.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("tsdf driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_tsdf.build()
    assert outs and all(os.path.exists(p) for p in outs)


class Cursor:
    def __init__(self, v):
        self.v, self.at = v, 0

    def take(self, n):
        out = self.v[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out

    def cloud(self):
        n, nn, nc = [int(v) for v in self.take(3)]
        return (self.take(3 * n).reshape(n, 3).copy(), self.take(3 * nn).reshape(nn, 3).copy(), self.take(3 * nc).reshape(nc, 3).copy())


@pytest.mark.gpu
@pytest.mark.parametrize("t", [S.COLOR_NONE, S.COLOR_RGB8, S.COLOR_GRAY32])
def test_shim_gives_the_reference_on_u21(lib, driver_bins, tmp_path, t):
    g = np.load(os.path.join(HERE, "golden", "tsdf.npz"))
    g = {k: g[k] for k in g.files}
    R = 21
    frames = frames_of(g)
    h, w = frames[0][0].shape
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii4di", w, h, *[float(v) for v in g["intrinsic"]], N_FRAMES))
        f.write(struct.pack("<ii5d", R, t, float(g["length"]), float(g["u21_sdf_trunc"]), *[float(v) for v in g["origin"]]))
        for depth, rgb, gray, E in frames:
            f.write(np.ascontiguousarray(E, "<f8").tobytes()); f.write(np.ascontiguousarray(depth, "<f4").tobytes())
            f.write(np.ascontiguousarray(rgb, np.uint8).tobytes()); f.write(np.ascontiguousarray(gray, "<f4").tobytes())
        name = {S.COLOR_RGB8: "s0", S.COLOR_GRAY32: "s1", S.COLOR_NONE: "s2"}[t]
        sR, stride, vl, strunc, st, nf = s_config(g, name)
        f.write(struct.pack("<iiiii2d", sR, stride, st, nf, 16, vl, strunc))
    n = R ** 3
    for b in driver_bins:
        p = subprocess.run([b, inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        c = Cursor(np.frombuffer(open(outp, "rb").read(), "<f8"))
        for stage in (0, 1):                                          # what test 1 reads: the volume after the first and the last frame
            tsdf, weight = c.take(n).astype(np.float32), c.take(n).astype(np.float32)
            color = c.take(3 * n).astype(np.float32).reshape(n, 3) if t else None
            check_volume(g, R, stage, t, tsdf, weight, color)

        def clouds():
            pts, nrm, col = c.cloud()
            vp, vn, vc = c.cloud()
            assert len(vn) == 0 and len(col) == (len(pts) if t else 0)
            return (pts, nrm, col if t else None), (vp, vc)

        first = clouds()                                              # a context of the caller's
        check_extraction(g, R, t, *first)
        again = clouds()                                              # the thread's context, after Reset()
        check_extraction(g, R, t, *again)
        assert all(same_bits(x, y) for x, y in zip(first[0][:2] + first[1], again[0][:2] + again[1]))
        pts, nrm, col = c.cloud()
        assert same_bits(pts, g["p_s4_id_points"]) and len(nrm) == 0 and len(col) == 0
        pts, nrm, col = c.cloud()
        assert same_bits(pts, g["p_s1_id_points"]) and len(nrm) == 0
        want = g["p_rgb_id_colors"] if t == S.COLOR_RGB8 else g["p_gray_id_colors"].astype(np.float64)
        assert same_bits(col, want)
        assert c.take(1)[0] == 1.0                                    # the frame that does not fit threw
        keys = None
        for i in range(nf):                                           # what test 3 reads: the unit set after each frame
            m = int(c.take(1)[0])
            keys = c.take(3 * m).astype(np.int32).reshape(m, 3)
            assert np.array_equal(keys, g["%s_units_f%d" % (name, i)]), (name, i)
        n3 = sR ** 3
        units = {}
        for key in map(tuple, keys.tolist()):
            units[key] = (c.take(n3).astype(np.float32), c.take(n3).astype(np.float32),
                          c.take(3 * n3).astype(np.float32).reshape(n3, 3) if st else None)
        check_units(g, name, keys, lambda q: units[q])
        pts, nrm, col = c.cloud()
        vp, vn, vc = c.cloud()
        check_scalable_extraction(g, name, (pts, nrm, col if st else None), (vp, vc))
        assert c.at == len(c.v)
