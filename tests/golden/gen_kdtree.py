"""Generate tests/golden/kdtree.npz: what the compiled reference's KDTreeFlann returns for the inputs tests/test_kdtree.py
pins its numpy specification (tests/kdtree_spec.py) and the library with.  Run once where the reference checkout exists; the
fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory outside the repository, compiles it there against
the reference's Core/Geometry/KDTreeFlann.cpp, PointCloud.cpp, TriangleMesh.cpp and Core/Utility with the vendored Eigen and
flann, runs it and records, per case (the clouds and queries of tests/kdtree_spec.py):

  <case>_tree, <case>_queries                the inputs (n x 3, nq x 3 f64)
  <case>_<search>_cnt                        the return value of every query's Search (int32)
  <case>_<search>_idx_sha, _d2_sha           SHA-256 of all the lists end to end: int32 indices, f64 distances
  <case>_<search>_rows, _idx, _d2            the queries `rows` (evenly spaced: about 2,000 entries) with their lists end to end
  searches: knn<k>, hybrid<r>_<max_nn>, radius<r> (CASES below)

  cloud   2,000 random points; 257 queries around them (a third points of the tree), 12 just outside the six faces of the
          bounding box and 3 a thousand diagonals away.  The tree is built from a PointCloud.
  line    500 points on a line, 6 queries off it.  The tree is built from the vertices of a TriangleMesh.
  bound   partners one ulp below, on and one ulp above (double)(float)(r * r) for r = 0.3 (rounds up) and 0.2 (rounds down)

  deg_*   degenerate arguments on a 5-point tree: knn = 8 > n (the list holds n), knn = -1 and max_nn = -1 (-1), a search of
          an empty tree (-1 from each of the three), and a NEGATIVE radius (the reference squares it: the answer of |r|).
          knn = 0 is NOT run: flann's KNNSimpleResultSet(0) writes dist_index_[capacity_ - 1] = dist_index_[-1] in
          clear() (flann/util/result_set.h:124), out of bounds.  max_nn = 0 is not run either: radiusSearch then only COUNTS
          (nn_index.h:500-512) and KDTreeFlann resizes the vectors to that count without filling them.

It asserts what makes the comparison with the fixture total: for every query all accepted d2 of the specification are distinct
(so no list has a tie, and at every KNN or Hybrid cut the last listed and the first unlisted distance differ), the reference's
lists come back ascending, the reference's d2 are bit-equal to the specification's and its indices and counts equal.  With
that the digests pin every list of the fixture index for index.

With --time it also times the reference's tree build and the three searches on the inputs of tools/kdtree_probe.py (this
machine's CPU, one thread; printed, not stored).  Nothing compiled and no reference text is kept."""
import argparse
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VISMA_REF", "/root/reference")
O3D = os.path.join(REF, "thirdparty", "Open3D")
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="kdtree_")      # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kdtree_spec as S  # noqa: E402

# search: (type, cap, radius)
SEARCHES = {
    "cloud": [(S.KNN, 1, 0.0), (S.KNN, 30, 0.0), (S.KNN, 171, 0.0), (S.KNN, 2000, 0.0), (S.KNN, 2005, 0.0),
              (S.HYBRID, 10, 0.1), (S.HYBRID, 100, 0.1), (S.HYBRID, 171, 0.25), (S.RADIUS, 0, 0.1), (S.RADIUS, 0, 0.04)],
    "line": [(S.KNN, 30, 0.0), (S.KNN, 200, 0.0), (S.HYBRID, 30, 0.5), (S.RADIUS, 0, 0.5)],
    "bound": [(S.HYBRID, 30, 0.3), (S.RADIUS, 0, 0.3), (S.HYBRID, 30, 0.2), (S.RADIUS, 0, 0.2)],
}
CLOUD_CELL = 0.1          # the edge the outside queries are placed by: 0.4 and 3.7 cells beyond each face


def search_name(s):
    t, cap, r = s
    return "knn%d" % cap if t == S.KNN else "hybrid%g_%d" % (r, cap) if t == S.HYBRID else "radius%g" % r


def inputs(case):
    """-> (tree, queries, from_mesh)"""
    if case == "cloud":
        tree = S.cloud(2000)
        q = np.concatenate([S.queries_around(tree, 257, 7), S.outside_queries(tree, CLOUD_CELL), S.far_queries(tree)])
        return tree, q, False
    if case == "line":
        return S.line_cloud(0), S.line_queries(0), True
    tree, q = S.bound_case()
    return tree, q, False


def deg_inputs():
    return S.cloud(5), S.queries_around(S.cloud(5), 4, 9)


HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <Core/Geometry/KDTreeFlann.h>
#include <Core/Geometry/PointCloud.h>
#include <Core/Geometry/TriangleMesh.h>
using namespace open3d;
static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static std::vector<Eigen::Vector3d> points(FILE *f)
{
    int n; rd(f, &n, 4);
    std::vector<Eigen::Vector3d> v((size_t)n);
    for (auto &p : v) { double x[3]; rd(f, x, 24); p = Eigen::Vector3d(x[0], x[1], x[2]); }
    return v;
}
static int search(const KDTreeFlann &t, const Eigen::Vector3d &q, int type, int cap, double r, std::vector<int> &i, std::vector<double> &d)
{
    if (type == 0) return t.Search(q, KDTreeSearchParamKNN(cap), i, d);
    if (type == 1) return t.Search(q, KDTreeSearchParamRadius(r), i, d);
    return t.Search(q, KDTreeSearchParamHybrid(r, cap), i, d);
}
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int from_mesh, timing; rd(f, &from_mesh, 4); rd(f, &timing, 4);
    PointCloud pc; TriangleMesh mesh;
    pc.points_ = points(f);
    mesh.vertices_ = pc.points_;
    std::vector<Eigen::Vector3d> queries = points(f);
    double t0 = now();
    KDTreeFlann tree;
    const bool ok = from_mesh ? tree.SetGeometry(mesh) : tree.SetGeometry(pc);
    if (timing) wd(o, now() - t0);
    if (!ok && !pc.points_.empty()) return 3;
    int ns; rd(f, &ns, 4);
    std::vector<int> idx; std::vector<double> d2;
    for (int s = 0; s < ns; s++) {
        int type, cap; double r; rd(f, &type, 4); rd(f, &cap, 4); rd(f, &r, 8);
        t0 = now();
        long long total = 0;
        for (auto &q : queries) {
            const int k = search(tree, q, type, cap, r, idx, d2);
            if (timing) { total += k; continue; }
            wd(o, (double)k);
            if (k < 0) continue;
            if ((size_t)k != idx.size() || (size_t)k != d2.size()) return 4;
            for (int j = 0; j < k; j++) wd(o, (double)idx[j]);
            for (int j = 0; j < k; j++) wd(o, d2[j]);
        }
        if (timing) { wd(o, now() - t0); wd(o, (double)total); }
    }
    std::fclose(o);
    return 0;
}
'''


def build():
    os.makedirs(SCRATCH, exist_ok=True)
    src = os.path.join(SCRATCH, "harness.cpp")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(SCRATCH, "harness")
    core = os.path.join(O3D, "src", "Core")
    json = os.path.join(O3D, "3rdparty", "jsoncpp")
    # (sections of functions nothing here calls are dropped at the link, and with them their references to what is not here)
    cmd = ["g++", "-std=c++11", "-O2", "-w", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",
           "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"), "-I" + os.path.join(O3D, "3rdparty"),
           "-I" + O3D, "-I" + os.path.join(json, "include"), "-I" + os.path.join(O3D, "3rdparty", "flann"), src]
    cmd += [os.path.join(core, "Geometry", n + ".cpp") for n in ("KDTreeFlann", "PointCloud", "TriangleMesh")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("Eigen", "Console", "Helper", "IJsonConvertible")]
    cmd += [os.path.join(json, "json_" + n + ".cpp") for n in ("value", "reader", "writer")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def run(exe, tree, queries, searches, from_mesh=False, timing=False):
    """-> per search a list over the queries of (k, idx, d2); timing: the raw doubles"""
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii", int(from_mesh), int(timing)))
        for a in (tree, queries):
            f.write(struct.pack("<i", len(a)))
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
        f.write(struct.pack("<i", len(searches)))
        for t, cap, r in searches:
            f.write(struct.pack("<iid", t, cap, r))
    subprocess.check_call([exe, inp, outp])
    v = np.frombuffer(open(outp, "rb").read(), "<f8")
    if timing:
        return v
    at, out = 0, []
    for _ in searches:
        rows = []
        for _q in range(len(queries)):
            k = int(v[at]); at += 1
            if k < 0:
                rows.append((k, None, None))
                continue
            rows.append((k, v[at:at + k].astype(np.int32), v[at + k:at + 2 * k].copy()))
            at += 2 * k
        out.append(rows)
    assert at == len(v)
    return out


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def sample_rows(nq, longest):
    """evenly spaced queries, the first and the last among them: as many as keep the stored lists near 2,000 entries"""
    m = max(2, min(nq, 2000 // max(longest, 1)))
    return np.unique(np.round(np.linspace(0, nq - 1, m)).astype(np.int32))


def flat(rows):
    cnt = np.array([k for k, _, _ in rows], np.int32)
    idx = np.concatenate([i for _, i, _ in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    d2 = np.concatenate([d for _, _, d in rows] + [np.zeros(0)])
    return cnt, idx, d2


def spec_flat(tree, queries, s):
    """the specification's lists of a search as `flat` gives the reference's"""
    t, cap, r = s
    if t == S.RADIUS:
        off, idx, d2 = S.spec_radius(tree, queries, r)
        return np.diff(off).astype(np.int32), idx, d2
    idx, d2, cnt = S.spec_search(tree, queries, t, cap, r)
    live = np.arange(cap)[None, :] < cnt[:, None]
    return cnt, idx[live], d2[live]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def check_total(tree, queries, s):
    """every accepted d2 of a query distinct: no tie inside a list or at a cut"""
    d2, ok = S.spec_pairs(tree, queries, s[0], s[2])
    for row, keep in zip(d2, ok):
        v = np.sort(row[keep])
        assert (np.diff(v) > 0).all(), ("a tie", s)


def store(out, name, rows):
    cnt, idx, d2 = flat(rows)
    out[name + "_cnt"] = cnt
    out[name + "_idx_sha"], out[name + "_d2_sha"] = sha(idx), sha(d2)
    at = sample_rows(len(rows), int(cnt.max()))
    out[name + "_rows"] = at
    out[name + "_idx"] = np.concatenate([rows[i][1] for i in at] + [np.zeros(0, np.int32)]).astype(np.int32)
    out[name + "_d2"] = np.concatenate([rows[i][2] for i in at] + [np.zeros(0)])


def time_reference(exe):
    import kdtree_probe as P
    tree, queries = P.inputs(P.N, P.NQ)
    v = run(exe, tree, queries, [(S.KNN, P.KNN, 0.0), (S.HYBRID, P.MAX_NN, P.RADIUS), (S.RADIUS, 0, P.RADIUS)], timing=True)
    print("reference KDTreeFlann, %d points, %d queries, one thread:" % (len(tree), len(queries)))
    print("  build %.1f ms" % (v[0] * 1e3))
    for name, (t, total) in zip(("SearchKNN(%d)" % P.KNN, "SearchHybrid(%g, %d)" % (P.RADIUS, P.MAX_NN), "SearchRadius(%g)" % P.RADIUS),
                                v[1:].reshape(3, 2)):
        print("  %-28s %.1f ms, %d entries" % (name, t * 1e3, int(total)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    exe = build()
    if args.time:
        time_reference(exe)
        return
    out = {}
    for case, searches in SEARCHES.items():
        tree, queries, from_mesh = inputs(case)
        out[case + "_tree"], out[case + "_queries"] = tree, queries
        got = run(exe, tree, queries, searches, from_mesh)
        for s, rows in zip(searches, got):
            check_total(tree, queries, s)
            cnt, idx, d2 = flat(rows)
            for _, _, d in rows:
                assert (np.diff(d) > 0).all(), ("not ascending", case, s)
            wc, wi, wd = spec_flat(tree, queries, s)
            assert np.array_equal(cnt, wc), (case, s, "counts")
            assert same_bits(d2, wd), (case, s, "d2 differs from the specification's")
            assert np.array_equal(idx, wi), (case, s, "indices")
            store(out, "%s_%s" % (case, search_name(s)), rows)
    # degenerate arguments
    tree, queries = deg_inputs()
    out["deg_tree"], out["deg_queries"] = tree, queries
    got = run(exe, tree, queries, [(S.KNN, 8, 0.0), (S.KNN, -1, 0.0), (S.HYBRID, -1, 0.5), (S.RADIUS, 0, -0.5), (S.HYBRID, 3, -0.5),
                                   (S.RADIUS, 0, 0.5), (S.HYBRID, 3, 0.5)])
    out["deg_knn8_cnt"], out["deg_knn8_idx"], out["deg_knn8_d2"] = flat(got[0])
    assert (out["deg_knn8_cnt"] == 5).all()
    out["deg_knn_negative"] = np.array([k for k, _, _ in got[1]], np.int32)
    out["deg_max_nn_negative"] = np.array([k for k, _, _ in got[2]], np.int32)
    assert (out["deg_knn_negative"] == -1).all() and (out["deg_max_nn_negative"] == -1).all()
    out["deg_radius_negative_cnt"], out["deg_radius_negative_idx"], out["deg_radius_negative_d2"] = flat(got[3])
    out["deg_hybrid_negative_cnt"], out["deg_hybrid_negative_idx"], out["deg_hybrid_negative_d2"] = flat(got[4])
    for a, b in ((3, 5), (4, 6)):                                   # a negative radius: the answer of its absolute value
        assert all(np.array_equal(x, y) for x, y in zip(flat(got[a]), flat(got[b])))
    assert out["deg_radius_negative_cnt"].max() > 1
    empty = run(exe, np.zeros((0, 3)), queries, [(S.KNN, 3, 0.0), (S.RADIUS, 0, 0.5), (S.HYBRID, 3, 0.5)])
    out["deg_empty_tree"] = np.array([[k for k, _, _ in rows] for rows in empty], np.int32)
    assert (out["deg_empty_tree"] == -1).all()
    path = os.path.join(HERE, "kdtree.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
