"""Generate tests/golden/trimesh.npz: what the compiled reference's TriangleMesh (ComputeTriangleNormals,
ComputeVertexNormals, NormalizeNormals, the four steps of Purge, Transform) and DownSample.cpp (SelectDownSample,
CropTriangleMesh) make of the programs of tests/trimesh_cases.py.  tests/test_trimesh_spec.py pins the numpy specification
(tests/trimesh_spec.py) with it, and tests/test_trimesh.py the library with the specification.  Run once where the reference
checkout exists; the fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory outside the repository, compiles it there against
the reference's Core/Geometry (TriangleMesh.cpp, DownSample.cpp, PointCloud.cpp, KDTreeFlann.cpp) and Core/Utility, runs it
and records per case <c> and program <p>:

  <c>_<p>_counts           nv, nt, has vertex normals, has vertex colours, has triangle normals (the reference's HasX())
  <c>_<p>_removed          the rows each remove_* / Purge step of the program removed, in order
  <c>_<p>_sha              SHA-256 of the raw rows (tests/trimesh_cases.py: raw_rows)
  <c>_<p>_<attribute>      ... and the rows in full (f64 rows as their uint64 bits), where vertices + triangles <= trimesh_cases.FULL_ROWS
Bits are compared as trimesh_cases.bits gives them: every NaN as one pattern (the sign and payload of a NaN that an operation
makes are the hardware's, not the reference's).

It asserts the properties that make each case bite (a case cannot silently stop testing anything), and that the
specification equals the reference bit for bit (the tests repeat that from the fixture).

--time prints the reference's one-thread time of ComputeVertexNormals and Purge on the meshes of tools/trimesh_probe.py,
when given the .npz such a mesh was saved to (printed, not stored).  Nothing compiled and no reference text is kept."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VISMA_REF", "/root/reference")
O3D = os.path.join(REF, "thirdparty", "Open3D")
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="trimesh_")      # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
import trimesh_spec as T  # noqa: E402
import trimesh_cases as cases  # noqa: E402

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <Core/Geometry/TriangleMesh.h>
using namespace open3d;
struct Mesh : TriangleMesh {
    using TriangleMesh::RemoveDuplicatedVertices;
    using TriangleMesh::RemoveDuplicatedTriangles;
    using TriangleMesh::RemoveNonManifoldVertices;
    using TriangleMesh::RemoveNonManifoldTriangles;
};
static double rd(FILE *f) { double v; if (fread(&v, 8, 1, f) != 1) std::exit(2); return v; }
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void rows(FILE *f, std::vector<Eigen::Vector3d> &a, size_t n) { a.resize(n); for (auto &p : a) { p(0) = rd(f); p(1) = rd(f); p(2) = rd(f); } }
static void wrows(FILE *o, const std::vector<Eigen::Vector3d> &a) { wd(o, (double)a.size()); for (auto &p : a) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); } }
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    Mesh m;
    const size_t nv = (size_t)rd(f), nt = (size_t)rd(f);
    const bool vn = rd(f) != 0, vc = rd(f) != 0, tn = rd(f) != 0;
    rows(f, m.vertices_, nv);
    if (vn) rows(f, m.vertex_normals_, nv);
    if (vc) rows(f, m.vertex_colors_, nv);
    m.triangles_.resize(nt);
    for (auto &t : m.triangles_) { t(0) = (int)rd(f); t(1) = (int)rd(f); t(2) = (int)rd(f); }
    if (tn) rows(f, m.triangle_normals_, nt);
    const int nops = (int)rd(f);
    std::vector<double> removed, times;
    for (int k = 0; k < nops; k++) {
        const int op = (int)rd(f);
        const size_t v0 = m.vertices_.size(), t0 = m.triangles_.size();
        const double s = now();
        switch (op) {
        case 0: m.ComputeTriangleNormals(rd(f) != 0); break;
        case 1: m.ComputeVertexNormals(rd(f) != 0); break;
        case 2: m.NormalizeNormals(); break;
        case 3: m.RemoveDuplicatedVertices(); removed.push_back((double)(v0 - m.vertices_.size())); break;
        case 4: m.RemoveDuplicatedTriangles(); removed.push_back((double)(t0 - m.triangles_.size())); break;
        case 5: m.RemoveNonManifoldTriangles(); removed.push_back((double)(t0 - m.triangles_.size())); break;
        case 6: m.RemoveNonManifoldVertices(); removed.push_back((double)(v0 - m.vertices_.size())); break;
        case 7: {
            size_t a = m.vertices_.size(), b = m.triangles_.size();
            m.RemoveDuplicatedVertices(); removed.push_back((double)(a - m.vertices_.size()));
            m.RemoveDuplicatedTriangles(); removed.push_back((double)(b - m.triangles_.size())); b = m.triangles_.size();
            m.RemoveNonManifoldTriangles(); removed.push_back((double)(b - m.triangles_.size())); a = m.vertices_.size();
            m.RemoveNonManifoldVertices(); removed.push_back((double)(a - m.vertices_.size()));
            break;
        }
        case 8: {
            std::vector<size_t> idx((size_t)rd(f));
            for (auto &i : idx) i = (size_t)rd(f);
            auto out = SelectDownSample(m, idx);
            static_cast<TriangleMesh &>(m) = *out;
            break;
        }
        case 9: {
            Eigen::Vector3d lo, hi;
            for (int i = 0; i < 3; i++) lo(i) = rd(f);
            for (int i = 0; i < 3; i++) hi(i) = rd(f);
            auto out = CropTriangleMesh(m, lo, hi);
            static_cast<TriangleMesh &>(m) = *out;
            break;
        }
        case 10: {
            Eigen::Matrix4d M;
            for (int i = 0; i < 16; i++) M(i / 4, i % 4) = rd(f);
            m.Transform(M);
            break;
        }
        default: return 3;
        }
        times.push_back(now() - s);
    }
    wrows(o, m.vertices_); wrows(o, m.vertex_normals_); wrows(o, m.vertex_colors_);
    wd(o, (double)m.triangles_.size());
    for (auto &t : m.triangles_) { wd(o, t(0)); wd(o, t(1)); wd(o, t(2)); }
    wrows(o, m.triangle_normals_);
    wd(o, (double)m.HasVertexNormals()); wd(o, (double)m.HasVertexColors()); wd(o, (double)m.HasTriangleNormals());
    wd(o, (double)removed.size()); for (double r : removed) wd(o, r);
    wd(o, (double)times.size()); for (double r : times) wd(o, r);
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
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-w", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",
           "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"), "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D,
           "-I" + os.path.join(O3D, "3rdparty", "flann"), src]
    cmd += [os.path.join(core, "Geometry", n + ".cpp") for n in ("TriangleMesh", "DownSample", "PointCloud", "KDTreeFlann")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("Eigen", "Console", "Helper")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def reference(exe, m, program):
    """-> the reference's mesh (a specification dict), its removed counts and the seconds each step took"""
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    with open(inp, "wb") as f:
        f.write(cases.encode(m, program))
    subprocess.check_call([exe, inp, outp], stdout=subprocess.DEVNULL)
    v = np.frombuffer(open(outp, "rb").read(), "<f8")
    at = [0]

    def take(n):
        out = v[at[0]:at[0] + n]
        assert len(out) == n
        at[0] += n
        return out

    def rows():
        n = int(take(1)[0])
        return take(3 * n).reshape(n, 3).copy()

    vtx, vn, vc = rows(), rows(), rows()
    tri = rows().astype(np.int32)
    tn = rows()
    has = [bool(x) for x in take(3)]
    out = dict(vertices=vtx, vertex_normals=vn if has[0] else None, vertex_colors=vc if has[1] else None, triangles=tri,
               triangle_normals=tn if has[2] else None)
    removed = [int(x) for x in take(int(take(1)[0]))]
    times = take(int(take(1)[0])).tolist()
    assert at[0] == len(v)
    return out, removed, times


def same(a, b):
    for k in T.ATTRS:
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and (a[k].shape != b[k].shape or cases.bits(a[k]).tobytes() != cases.bits(b[k]).tobytes()):
            return False
    return True


def bite(name, results):
    """the properties that make a case test something, on the REFERENCE's results"""
    m, programs = cases.load()[name]
    ref = lambda p: results[p][0]
    rem = lambda p: results[p][1]
    if name == "soup":
        v = ref(0)["vertices"]
        assert len(v) == 441 + 8, len(v)                     # the grid, 2 NaN, +inf, -inf, two denormals, (7, 7, 1), (7, 7, 1 + ulp)
        assert np.count_nonzero(np.isnan(v[:, 0])) == 2      # the bit-identical NaN vertices did not merge
        assert np.count_nonzero(v[:, 0] == np.inf) == 1 and np.count_nonzero(v[:, 0] == -np.inf) == 1
        assert np.count_nonzero(v[:, 0] == 5e-324) == 1 and np.count_nonzero(v[:, 0] == 1e-323) == 1
        assert np.count_nonzero((v[:, 0] == 7.0) & (v[:, 1] == 7.0)) == 2          # one ulp apart in z: two vertices
        row0 = m["vertices"][:, 1] == 0.0
        assert np.signbit(m["vertices"][row0, 1]).any() and not np.signbit(m["vertices"][row0, 1]).all()
        assert np.count_nonzero(v[:, 1] == 0.0) == 21        # -0.0 and +0.0 welded
        assert rem(0) == [2410 - 449] and rem(1)[2] == 1     # the triangle over both +inf vertices degenerates once they are welded
    if name == "keys":
        # gone: two rotations of (0, 1, 2), (1, 0, 0) -- whose key is (0, 0, 1)'s --, (4, 5, 6) after (6, 4, 5), the second (0, 1, 0)
        assert rem(0) == [5], rem(0)
        t = ref(0)["triangles"].tolist()
        assert [0, 2, 1] in t and [0, 1, 0] in t and [0, 0, 1] in t and [1, 0, 0] not in t and [1, 2, 0] not in t
        assert rem(1) == [1, 6], rem(1)                      # welding vertex 6 onto 3 makes one more triangle coincide
        assert rem(2) == [4] and rem(4) == [1, 6, 3, 1], (rem(2), rem(4))   # ... and (3, 4, 6) degenerate; vertex 7 is unused
    if name == "fan":
        fwd = T.copy(m); T.compute_vertex_normals(fwd, False)
        rev = T.copy(m); T.compute_vertex_normals(rev, False, reverse=True)
        assert fwd["vertex_normals"][0].tobytes() != rev["vertex_normals"][0].tobytes()
        assert ref(0)["vertex_normals"][0].tobytes() == fwd["vertex_normals"][0].tobytes()
        mag = np.linalg.norm(ref(0)["triangle_normals"], axis=1)
        assert mag.max() / mag.min() > 2.0 ** 50
        assert ref(2)["vertex_normals"].tobytes() != ref(0)["vertex_normals"].tobytes()      # normalised triangle normals were used as they were
        assert ref(3)["vertex_normals"].tobytes() != ref(0)["vertex_normals"].tobytes()      # the second call added onto the first
    if name == "normalize":
        vn = ref(0)["vertex_normals"]
        assert vn[0].tolist() == [0, 0, 0] and vn[1].tolist() == [0, 0, 1] and np.isnan(vn[2, 1]) and vn[2, 0] == 1.0
        assert vn[3].tolist() == [0, 0, 0] and vn[4].tolist() == [1e-200, 1e-200, 0] and vn[7].tolist() == [0, 0, 1]
        tn = ref(2)["triangle_normals"]
        assert np.isinf(tn).any() and (tn[1] == 0).all()
    if name.startswith("tile"):
        assert all(r > 0 for r in rem(0)[:3]), rem(0)
        assert len(m["vertices"]) == len(m["triangles"]) == int(name[4:])
        assert 0 < len(ref(4)["triangles"]) and 0 < len(ref(5)["triangles"])
    if name == "big":
        assert len(m["triangles"]) > 262144 and rem(0) == [0, 106667, 0, 3000], rem(0)
    if name == "loose":
        assert rem(0) == [0, 0, 0, 5] and len(ref(0)["vertices"]) == 0
    if name == "crop":
        full = len(m["triangles"])
        # inclusive bounds: x 0.5 .. 1.5 (5 columns), y 0.5 .. 1.75 (6), less the NaN vertex inside and its six triangles
        assert len(ref(0)["vertices"]) == 5 * 6 - 1 and len(ref(0)["triangles"]) == 2 * 4 * 5 - 6, (len(ref(0)["vertices"]), len(ref(0)["triangles"]))
        assert len(ref(1)["vertices"]) == 0 and len(ref(2)["vertices"]) == 0
        assert 0 < len(ref(3)["triangles"]) < full
        assert len(ref(4)["triangles"]) < full               # the NaN vertex fails an infinite box
        assert len(ref(4)["vertices"]) == len(m["vertices"]) - 1
    if name == "select":
        assert len(ref(0)["triangles"]) == 4 and len(ref(1)["triangles"]) == len(m["triangles"]) - 2
        assert same(ref(2), ref(4)) and len(ref(2)["triangles"]) == len(m["triangles"]) and len(ref(3)["vertices"]) == 0
    if name == "transform":
        assert np.isnan(ref(1)["vertex_normals"]).any() and ref(0)["vertex_colors"].tobytes() == m["vertex_colors"].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", metavar="MESH.npz", help="vertices, triangles (and colors) of a mesh to time the reference on")
    args = ap.parse_args()
    exe = build()
    if args.time:
        z = np.load(args.time)
        m = T.mesh(z["vertices"], z["triangles"], None, z["colors"] if "colors" in z.files else None)
        _, _, t1 = reference(exe, m, [("cvn", 1)])
        _, removed, t2 = reference(exe, m, [("purge",)])
        print("reference on this CPU (one thread), %d vertices, %d triangles: ComputeVertexNormals %.1f ms, Purge %.1f ms (removed %s)"
              % (len(m["vertices"]), len(m["triangles"]), t1[0] * 1e3, t2[0] * 1e3, removed))
        return
    fix = {}
    for name in cases.NAMES:
        m, programs = cases.load()[name]
        results = []
        for p, program in enumerate(programs):
            ref, removed, _ = reference(exe, m, program)
            results.append((ref, removed))
            mine, mine_removed = cases.spec(name, p)
            assert mine_removed == removed, (name, p, mine_removed, removed)
            for k in T.ATTRS:
                assert (mine[k] is None) == (ref[k] is None), (name, p, k)
                if ref[k] is not None:
                    assert mine[k].shape == ref[k].shape and mine[k].dtype == ref[k].dtype, (name, p, k)
                    bad = np.nonzero((cases.bits(mine[k]) != cases.bits(ref[k])).any(axis=1))[0]
                    assert len(bad) == 0, (name, p, k, bad[:5], mine[k][bad[:3]], ref[k][bad[:3]])
            key = "%s_%d_" % (name, p)
            fix[key + "counts"] = np.array([len(ref["vertices"]), len(ref["triangles"]), ref["vertex_normals"] is not None,
                                            ref["vertex_colors"] is not None, ref["triangle_normals"] is not None], np.int64)
            fix[key + "removed"] = np.array(removed, np.int64)
            fix[key + "sha"] = np.frombuffer(hashlib.sha256(cases.raw_rows(ref)).digest(), np.uint8).copy()
            if len(ref["vertices"]) + len(ref["triangles"]) <= cases.FULL_ROWS:
                for k in T.ATTRS:
                    if ref[k] is not None:
                        fix[key + k] = cases.bits(ref[k])      # (f64 rows as uint64: a NaN is one pattern, trimesh_cases.bits)
            print("%s program %d: %d vertices, %d triangles, removed %s" % (name, p, len(ref["vertices"]), len(ref["triangles"]), removed))
        bite(name, results)
    out = os.path.join(HERE, "trimesh.npz")
    np.savez_compressed(out, **fix)
    print("trimesh.npz: %d bytes" % os.path.getsize(out))
    if os.path.getsize(out) > 512 * 1024:
        raise SystemExit("the fixture is larger than 512 KB")


if __name__ == "__main__":
    main()
