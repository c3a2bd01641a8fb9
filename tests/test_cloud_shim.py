"""open3d::PointCloud of the stand-alone header set (include/Core/Geometry/PointCloud.h): tests/cpp/cloud_driver.cpp calls
GetMinBound / GetMaxBound, NormalizeNormals, PaintUniformColor, Transform, SelectDownSample, UniformDownSample, CropPointCloud,
the two OrientNormals*, ComputePointCloudMeanAndCovariance and ComputePointCloudMahalanobisDistance with the reference's names
and signatures, compiled in both Eigen storage orders; on a few cases of tests/cloud_cases.py its clouds and results equal the
specification's bit for bit (tests/test_cloud_spec.py pins that to the compiled reference), once through the free functions
(an upload and a download each) and once on one cicp::DevicePointCloud.  Also: cicp::ExtractPointCloud takes the volume's
cloud on the device, and a chain on it equals the host chain."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_cases as cases
import cloud_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_cloud  # noqa: E402

# the programs the header set's names express (operator+= of the host class is older than this driver and stays as it is)
SHIM_OPS = ("transform", "norm", "paint", "bounds", "select", "uniform", "crop", "orient_dir", "orient_cam", "meancov", "mahal")
ITEMS = [("tile257", 0), ("tile257", 4), ("sums16384", 1), ("planar", 1), ("empty", 2), ("bounds_nan_first", 0), ("bounds_zero_neg_first", 0),
         ("select", 0), ("uniform", 2), ("transform", 0), ("transform", 3), ("normals", 0), ("normals", 5), ("normals", 7), ("normals", 10)]
assert all(op[0] in SHIM_OPS for name, p in ITEMS for op in cases.load()[name][1][p])


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_cloud.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_cloud.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("cloud driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_cloud.build()
    assert outs and all(os.path.exists(p) for p in outs)


class Cursor:
    def __init__(self, v):
        self.v, self.at = v, 0

    def take(self, n):
        out = self.v[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out

    def rows(self):
        n = int(self.take(1)[0])
        return self.take(3 * n).reshape(n, 3).copy()

    def cloud(self):
        p, nrm, col = self.rows(), self.rows(), self.rows()
        has = [bool(x) for x in self.take(2)]
        return dict(points=p, normals=nrm if has[0] else None, colors=col if has[1] else None), self.take(int(self.take(1)[0])).copy()


def same(got, want, label, within=None):
    """within: {attribute: bound per entry} for rows that are not claimed to the bit"""
    (cloud, results), (want_cloud, want_results) = got, want
    for k in S.ATTRS:
        assert (cloud[k] is None) == (want_cloud[k] is None), (label, k)
        if want_cloud[k] is not None:
            assert cloud[k].shape == want_cloud[k].shape, (label, k, cloud[k].shape, want_cloud[k].shape)
            if within and k in within:
                assert (np.abs(cloud[k] - want_cloud[k]) <= within[k]).all(), (label, k)
            else:
                assert np.array_equal(cases.bits(cloud[k]), cases.bits(want_cloud[k])), (label, k)
    want_results = cases.flat_results(want_results)
    assert results.shape == want_results.shape and np.array_equal(cases.bits(results), cases.bits(want_results)), (label, results[:12], want_results[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("name,p", ITEMS)
def test_shim_clouds_equal_the_specification(lib, driver_bins, tmp_path, name, p):
    c, programs = cases.load()[name]
    want = cases.spec(name, p, cases.CHUNK)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(cases.encode(c, programs[p]))
    # PointCloud::Transform of the header set is a host member older than this driver and stays as it is: Eigen's block product
    # there (R p + t) adds its three products and the translation in an order of its own.  Two orders of one sum of four
    # rounded terms differ by at most 2 gamma(3) sum |terms| (gamma(3) < 4 * 2^-53); the normals have three terms.  The
    # DevicePointCloud's rows are the specification's to the bit.
    within = None
    if programs[p][0][0] == "transform":
        assert len(programs[p]) == 1
        T = np.abs(np.asarray(programs[p][0][1], np.float64).reshape(4, 4))
        within = {"points": 8.0 * 2.0 ** -53 * (np.abs(c["points"]) @ T[:3, :3].T + T[:3, 3]),
                  "normals": 8.0 * 2.0 ** -53 * (np.abs(c["normals"]) @ T[:3, :3].T)}
    for b in driver_bins:
        r = subprocess.run([b, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (b, r.returncode, r.stdout, r.stderr)
        cur = Cursor(np.frombuffer(open(outp, "rb").read(), "<f8"))
        same(cur.cloud(), want, (name, p, b, "the reference's names"), within)
        same(cur.cloud(), want, (name, p, b, "one DevicePointCloud"))
        assert cur.take(1)[0] == 1.0, r.stderr               # cicp::ExtractPointCloud(volume): the rows of ExtractPointCloud()
        assert cur.take(1)[0] == 1.0, r.stderr               # ... and crop, VoxelDownSample, EstimateNormals on it: the host chain's rows
        assert cur.at == len(cur.v)
