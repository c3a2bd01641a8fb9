// trimesh_driver.cpp -- open3d::TriangleMesh's computing members, SelectDownSample and CropTriangleMesh called with the
// reference's names and signatures, against the stand-alone header set.
// Usage: trimesh_driver <in.bin> <out.bin>
//   in : doubles (tests/trimesh_cases.py: encode).  nv, nt, has vertex normals, has vertex colours, has triangle normals, the
//        rows, then a program: n steps of {code, arguments} -- 0 ComputeTriangleNormals(b), 1 ComputeVertexNormals(b),
//        2 NormalizeNormals, 7 Purge, 8 SelectDownSample(n, indices), 9 CropTriangleMesh(min, max), 10 Transform(16, row-major)
//   out: doubles.  The mesh behind the program as {n, rows} for vertices, vertex normals, vertex colours, triangles, triangle
//        normals, then HasVertexNormals, HasVertexColors, HasTriangleNormals; GetMinBound and GetMaxBound of the INPUT mesh;
//        the mesh (input + input painted (0.25, 0.5, 0.75)) the same way; 1.0 if cicp::ExtractTriangleMesh(volume, true, true)
//        of a small UniformTSDFVolume equals ExtractTriangleMesh() + Purge() + ComputeVertexNormals() bit for bit, else 0.0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static double rd(FILE *f) { double v; if (fread(&v, 8, 1, f) != 1) std::exit(2); return v; }
static void wd(FILE *o, double v) { if (fwrite(&v, 8, 1, o) != 1) std::exit(4); }
static void rows(FILE *f, std::vector<Eigen::Vector3d> &a, size_t n) { a.resize(n); for (auto &p : a) { p(0) = rd(f); p(1) = rd(f); p(2) = rd(f); } }
static void wrows(FILE *o, const std::vector<Eigen::Vector3d> &a) { wd(o, (double)a.size()); for (const auto &p : a) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); } }
static void wmesh(FILE *o, const TriangleMesh &m)
{
    wrows(o, m.vertices_); wrows(o, m.vertex_normals_); wrows(o, m.vertex_colors_);
    wd(o, (double)m.triangles_.size());
    for (const auto &t : m.triangles_) { wd(o, t(0)); wd(o, t(1)); wd(o, t(2)); }
    wrows(o, m.triangle_normals_);
    wd(o, (double)m.HasVertexNormals()); wd(o, (double)m.HasVertexColors()); wd(o, (double)m.HasTriangleNormals());
}
static bool same_rows(const std::vector<Eigen::Vector3d> &a, const std::vector<Eigen::Vector3d> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a[0].data(), b[0].data(), a.size() * sizeof(a[0])) == 0);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    TriangleMesh m;
    const size_t nv = (size_t)rd(f), nt = (size_t)rd(f);
    const bool vn = rd(f) != 0, vc = rd(f) != 0, tn = rd(f) != 0;
    rows(f, m.vertices_, nv);
    if (vn) rows(f, m.vertex_normals_, nv);
    if (vc) rows(f, m.vertex_colors_, nv);
    m.triangles_.resize(nt);
    for (auto &t : m.triangles_) { t(0) = (int)rd(f); t(1) = (int)rd(f); t(2) = (int)rd(f); }
    if (tn) rows(f, m.triangle_normals_, nt);
    const TriangleMesh input = m;
    const int nops = (int)rd(f);
    for (int k = 0; k < nops; k++) {
        switch ((int)rd(f)) {
        case 0: m.ComputeTriangleNormals(rd(f) != 0); break;
        case 1: m.ComputeVertexNormals(rd(f) != 0); break;
        case 2: m.NormalizeNormals(); break;
        case 7: m.Purge(); break;
        case 8: {
            std::vector<size_t> idx((size_t)rd(f));
            for (auto &i : idx) i = (size_t)rd(f);
            std::shared_ptr<TriangleMesh> out = SelectDownSample(m, idx);
            m = *out;
            break;
        }
        case 9: {
            Eigen::Vector3d lo, hi;
            for (int i = 0; i < 3; i++) lo(i) = rd(f);
            for (int i = 0; i < 3; i++) hi(i) = rd(f);
            std::shared_ptr<TriangleMesh> out = CropTriangleMesh(m, lo, hi);
            m = *out;
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
    }
    wmesh(o, m);
    const Eigen::Vector3d lo = input.GetMinBound(), hi = input.GetMaxBound();
    for (int i = 0; i < 3; i++) wd(o, lo(i));
    for (int i = 0; i < 3; i++) wd(o, hi(i));
    TriangleMesh painted = input;
    painted.PaintUniformColor(Eigen::Vector3d(0.25, 0.5, 0.75));
    wmesh(o, input + painted);

    // the volume's mesh handed over on the device: 4^3 voxels of 0.25 in front of a flat 17 x 17 frame
    double handed = 0.0;
    {
        UniformTSDFVolume vol(1.0, 4, 0.75, TSDFVolumeColorType::RGB8, Eigen::Vector3d(-0.5, -0.5, 0.125));
        RGBDImage frame;
        frame.depth_.PrepareImage(17, 17, 1, 4);
        frame.color_.PrepareImage(17, 17, 3, 1);
        float *depth = reinterpret_cast<float *>(frame.depth_.data_.data());
        for (int i = 0; i < 17 * 17; i++) { depth[i] = 0.625f; for (int c = 0; c < 3; c++) frame.color_.data_[3 * i + c] = (uint8_t)(i + 40 * c); }
        vol.Integrate(frame, PinholeCameraIntrinsic(17, 17, 4.0, 4.0, 8.0, 8.0), Eigen::Matrix4d::Identity());
        TSDFVolume &base = vol;
        std::shared_ptr<TriangleMesh> host = base.ExtractTriangleMesh();
        host->Purge();
        host->ComputeVertexNormals();
        std::shared_ptr<TriangleMesh> device = cicp::ExtractTriangleMesh(base, true, true);
        handed = host->HasTriangles() && host->HasVertexNormals() && same_rows(host->vertices_, device->vertices_) &&
                         same_rows(host->vertex_normals_, device->vertex_normals_) && same_rows(host->vertex_colors_, device->vertex_colors_) &&
                         same_rows(host->triangle_normals_, device->triangle_normals_) && host->triangles_.size() == device->triangles_.size() &&
                         std::memcmp(host->triangles_[0].data(), device->triangles_[0].data(), host->triangles_.size() * sizeof(Eigen::Vector3i)) == 0
                     ? 1.0 : 0.0;
    }
    wd(o, handed);
    std::fclose(o);
    return 0;
}
