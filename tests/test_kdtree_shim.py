"""open3d::KDTreeFlann of the stand-alone header set (include/Core/Geometry/KDTreeFlann.h, included from Core/Core.h) and the
batch overloads of open3d::cicp: tests/cpp/kdtree_driver.cpp compiles against it in both Eigen storage orders, builds a tree on
a PointCloud and one on a TriangleMesh, and its Search with each of the three KDTreeSearchParam kinds, query by query, and the
batch overloads give what the Python path (Context.kdtree) gives on the same inputs; the degenerate calls return what
tests/golden/kdtree.npz records of the reference (-1 for an empty tree and for knn or max_nn < 0, a negative radius as its
absolute value, knn > n a list of n)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import kdtree_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_kdtree  # noqa: E402
import build_shim  # noqa: E402

KNN, RADIUS, MAX_NN = 7, 0.12, 5


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_kdtree.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_kdtree.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("kdtree driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_kdtree.build()
    assert outs and all(os.path.exists(p) for p in outs)
    core = open(os.path.join(HERE, "..", "include", "Core", "Core.h")).read()
    assert '#include "Geometry/KDTreeFlann.h"' in core


class Cursor:
    def __init__(self, v):
        self.v, self.at = v, 0

    def take(self, n):
        out = self.v[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out

    def one(self):
        return float(self.take(1)[0])

    def list(self):
        k = int(self.one())
        if k < 0:
            return k, None, None
        return k, self.take(k).astype(np.int32), self.take(k).copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.gpu
def test_shim_gives_what_the_python_path_gives(lib, driver_bins, tmp_path):
    tree = S.cloud(500)
    q = np.concatenate([S.queries_around(tree, 20, 4), S.outside_queries(tree, RADIUS)[:4], S.far_queries(tree)[:1]])
    nq = len(q)
    ctx = lib.Context(0)
    with ctx.kdtree(tree) as kd:
        ki, kd2, kc = kd.search_knn(q, KNN)
        hi, hd2, hc = kd.search_hybrid(q, RADIUS, MAX_NN)
        off, ri, rd2 = kd.search_radius(q, RADIUS)
        big = kd.search_knn(q[:1], len(tree) + 5)
    ctx.close()
    assert (kc == KNN).all() and hc.max() == MAX_NN and hc.min() == 0 and np.diff(off).max() > MAX_NN
    g = np.load(os.path.join(HERE, "golden", "kdtree.npz"))
    assert (g["deg_empty_tree"] == -1).all() and (g["deg_knn_negative"] == -1).all() and (g["deg_max_nn_negative"] == -1).all()
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        for a in (tree, q):
            f.write(struct.pack("<i", len(a)))
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
        f.write(struct.pack("<idi", KNN, RADIUS, MAX_NN))
    for b in driver_bins:
        p = subprocess.run([b, inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        c = Cursor(np.frombuffer(open(outp, "rb").read(), "<f8"))
        for which in ("PointCloud", "TriangleMesh"):
            for i in range(nq):                                       # query by query: the vectors resized to the count
                k, idx, d2 = c.list()
                assert k == kc[i] and np.array_equal(idx, ki[i, :k]) and same_bits(d2, kd2[i, :k]), (which, "knn", i)
                k, idx, d2 = c.list()
                assert k == off[i + 1] - off[i] and np.array_equal(idx, ri[off[i]:off[i + 1]]), (which, "radius", i)
                assert same_bits(d2, rd2[off[i]:off[i + 1]]), (which, "radius", i)
                k, idx, d2 = c.list()
                assert k == hc[i] and np.array_equal(idx, hi[i, :k]) and same_bits(d2, hd2[i, :k]), (which, "hybrid", i)
            for cnt, idx, d2, cap in ((kc, ki, kd2, KNN), (hc, hi, hd2, MAX_NN)):       # the batch overloads: flat, padded
                assert c.one() == nq
                assert np.array_equal(c.take(nq).astype(np.int32), cnt)
                assert np.array_equal(c.take(nq * cap).astype(np.int32).reshape(nq, cap), idx)
                assert same_bits(c.take(nq * cap).reshape(nq, cap), d2)
            assert c.one() == nq
            assert np.array_equal(c.take(nq + 1).astype(np.int64), off)
            assert np.array_equal(c.take(len(ri)).astype(np.int32), ri) and same_bits(c.take(len(ri)), rd2)
        # the degenerate calls: what the fixture records of the reference
        assert c.take(5).tolist() == [-1.0] * 5                       # an empty tree
        assert c.take(4).tolist() == [-1.0] * 4                       # knn < 0, max_nn < 0
        assert c.one() == 7.0                                         # ... and the vectors are left alone
        assert c.take(4).tolist() == [0.0, 0.0, 0.0, 0.0]             # knn = 0 (and its vector), max_nn = 0, radius 0
        k, idx, d2 = c.list()                                         # a negative radius
        assert k == off[1] - off[0] and np.array_equal(idx, ri[:off[1]]) and same_bits(d2, rd2[:off[1]])
        k, idx, d2 = c.list()
        assert k == hc[0] and np.array_equal(idx, hi[0, :k]) and same_bits(d2, hd2[0, :k])
        k, idx, d2 = c.list()                                         # knn > n: the list holds n
        assert k == len(tree) and np.array_equal(idx, big[0][0, :k]) and same_bits(d2, big[1][0, :k])
        assert c.take(2).tolist() == [0.0, -1.0]                      # SetMatrixData with two rows: false, an empty tree
        assert c.one() == 1.0                                         # ... with three: the tree of the cloud
        k, idx, d2 = c.list()
        assert k == kc[0] and np.array_equal(idx, ki[0, :k]) and same_bits(d2, kd2[0, :k])
        assert c.take(2).tolist() == [0.0, -1.0]                      # a geometry of no points: false, an empty tree
        assert c.one() == -1.0                                        # a query of four rows
        assert c.at == len(c.v)
