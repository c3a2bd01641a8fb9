"""open3d::TriangleMesh of the stand-alone header set (include/Core/Geometry/TriangleMesh.h): tests/cpp/trimesh_driver.cpp
calls ComputeTriangleNormals, ComputeVertexNormals, NormalizeNormals, Purge, Transform, SelectDownSample and CropTriangleMesh
with the reference's names and signatures, compiled in both Eigen storage orders; on a few cases of tests/trimesh_cases.py its
meshes equal the specification's bit for bit (tests/test_trimesh_spec.py pins that to the compiled reference).  Also: the
host members (GetMinBound / GetMaxBound, PaintUniformColor, operator+) and the volume's mesh handed over on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import trimesh_cases as cases
import trimesh_spec as T

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_trimesh  # noqa: E402

# the programs the class can express (the four steps of Purge are protected members in the reference)
SHIM_OPS = ("ctn", "cvn", "norm", "purge", "select", "crop", "transform")
ITEMS = [("keys", 4), ("fan", 2), ("fan", 3), ("normalize", 0), ("normalize", 3), ("tile257", 0), ("tile257", 3), ("tile257", 4),
         ("tile257", 5), ("loose", 0), ("crop", 0), ("select", 0), ("transform", 1), ("transform", 3)]
assert all(op[0] in SHIM_OPS for name, p in ITEMS for op in cases.load()[name][1][p])


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_trimesh.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_trimesh.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("trimesh driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_trimesh.build()
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

    def mesh(self):
        v, vn, vc = self.rows(), self.rows(), self.rows()
        t = self.rows().astype(np.int32)
        tn = self.rows()
        has = [bool(x) for x in self.take(3)]
        return dict(vertices=v, vertex_normals=vn if has[0] else None, vertex_colors=vc if has[1] else None, triangles=t,
                    triangle_normals=tn if has[2] else None)


def same(got, want, label):
    for k in T.ATTRS:
        assert (got[k] is None) == (want[k] is None), (label, k)
        if want[k] is not None:
            assert got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
            assert np.array_equal(cases.bits(got[k]), cases.bits(want[k])), (label, k)


def joined(a, b):
    """a + b as TriangleMesh.cpp:97-139 joins two meshes"""
    both = lambda k: None if a[k] is None or b[k] is None else np.concatenate([a[k], b[k]])
    return T.mesh(np.concatenate([a["vertices"], b["vertices"]]), np.concatenate([a["triangles"], b["triangles"] + len(a["vertices"])]),
                  both("vertex_normals"), both("vertex_colors"), both("triangle_normals"))


@pytest.mark.gpu
@pytest.mark.parametrize("name,p", ITEMS)
def test_shim_meshes_equal_the_specification(lib, driver_bins, tmp_path, name, p):
    m, programs = cases.load()[name]
    want, _ = cases.spec(name, p)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(cases.encode(m, programs[p]))
    painted = T.copy(m)
    painted["vertex_colors"] = np.tile([0.25, 0.5, 0.75], (len(m["vertices"]), 1)) if len(m["vertices"]) else None
    for b in driver_bins:
        r = subprocess.run([b, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (b, r.returncode, r.stdout, r.stderr)
        c = Cursor(np.frombuffer(open(outp, "rb").read(), "<f8"))
        same(c.mesh(), want, (name, p, b))
        lo, hi = c.take(3), c.take(3)
        v = m["vertices"]
        if len(v) and not np.isnan(v).any():
            assert lo.tolist() == v.min(axis=0).tolist() and hi.tolist() == v.max(axis=0).tolist()
        elif not len(v):
            assert lo.tolist() == hi.tolist() == [0.0, 0.0, 0.0]
        same(c.mesh(), joined(m, painted), (name, p, b, "operator+"))
        assert c.take(1)[0] == 1.0, r.stderr                 # cicp::ExtractTriangleMesh(volume, true, true): the host chain's rows
        assert c.at == len(c.v)
