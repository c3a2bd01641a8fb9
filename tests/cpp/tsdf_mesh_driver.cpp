// tsdf_mesh_driver.cpp -- ExtractTriangleMesh called the way an Open3D caller does, against the stand-alone header set.
// Usage: tsdf_mesh_driver <in.bin> <out.bin>
//   in : int32 w, h, 4 doubles fx fy cx cy, int32 n frames, int32 resolution, colour type (0 none, 1 rgb8, 2 gray32), double
//        length, sdf_trunc, 3 doubles origin, then per frame 16 doubles extrinsic (row-major), w x h float depth, w x h x 3
//        bytes rgb, w x h float gray; behind the frames: int32 unit resolution, stride, colour type, frames to use, double
//        voxel_length, sdf_trunc of a ScalableTSDFVolume
//   out: doubles.  The mesh of the UniformTSDFVolume (on a context of the caller's, through the TSDFVolume interface) as
//        {n vertices, n colours, n triangles, the rows}; 1.0 if cicp::ColorMapOptimization took that mesh with zero
//        iterations and left one colour per vertex, else 0.0; the mesh of the ScalableTSDFVolume (the thread's context)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { if (fwrite(&v, 8, 1, o) != 1) std::exit(4); }
static void wmesh(FILE *o, const TriangleMesh &m)
{
    wd(o, (double)m.vertices_.size()); wd(o, (double)m.vertex_colors_.size()); wd(o, (double)m.triangles_.size());
    for (const auto &p : m.vertices_) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); }
    for (const auto &p : m.vertex_colors_) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); }
    for (const auto &t : m.triangles_) { wd(o, t(0)); wd(o, t(1)); wd(o, t(2)); }
}
struct Frame { Eigen::Matrix4d E; RGBDImage rgb, gray; };

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int32_t w, h, n, R, ctype;
    double k[4], length, trunc, org[3];
    rd(f, &w, 4); rd(f, &h, 4); rd(f, k, sizeof(k)); rd(f, &n, 4); rd(f, &R, 4); rd(f, &ctype, 4);
    rd(f, &length, 8); rd(f, &trunc, 8); rd(f, org, sizeof(org));
    std::vector<Frame> frames((size_t)n);
    for (auto &fr : frames) {
        double e[16];
        rd(f, e, sizeof(e));
        for (int i = 0; i < 16; i++) fr.E(i / 4, i % 4) = e[i];
        fr.rgb.depth_.PrepareImage(w, h, 1, 4); rd(f, fr.rgb.depth_.data_.data(), fr.rgb.depth_.data_.size());
        fr.rgb.color_.PrepareImage(w, h, 3, 1); rd(f, fr.rgb.color_.data_.data(), fr.rgb.color_.data_.size());
        fr.gray.depth_ = fr.rgb.depth_;
        fr.gray.color_.PrepareImage(w, h, 1, 4); rd(f, fr.gray.color_.data_.data(), fr.gray.color_.data_.size());
    }
    int32_t sR, stride, stype, nf;
    double vl, strunc;
    rd(f, &sR, 4); rd(f, &stride, 4); rd(f, &stype, 4); rd(f, &nf, 4); rd(f, &vl, 8); rd(f, &strunc, 8);
    const PinholeCameraIntrinsic camera(w, h, k[0], k[1], k[2], k[3]);

    visma_icp_ctx *ctx = nullptr;
    if (visma_icp_create(&ctx, 0) != VISMA_ICP_OK) return 3;
    {
        UniformTSDFVolume vol(ctx, length, R, trunc, (TSDFVolumeColorType)ctype, Eigen::Vector3d(org[0], org[1], org[2]));
        TSDFVolume &base = vol;                                          // (through the interface, as a pipeline holds it)
        for (const auto &fr : frames) base.Integrate(ctype == 2 ? fr.gray : fr.rgb, camera, fr.E);
        std::shared_ptr<TriangleMesh> mesh = base.ExtractTriangleMesh();
        wmesh(o, *mesh);
        // the next step of the pipeline takes it
        PinholeCameraTrajectory trajectory;
        trajectory.intrinsic_ = camera;
        std::vector<RGBDImage> images;
        for (const auto &fr : frames) { trajectory.extrinsic_.push_back(fr.E); images.push_back(fr.rgb); }
        ColorMapOptmizationOption option;
        option.maximum_iteration_ = 0;
        double took = 0.0;
        try {
            cicp::ColorMapOptimization(ctx, *mesh, images, trajectory, option);
            took = mesh->vertex_colors_.size() == mesh->vertices_.size() && mesh->HasTriangles() ? 1.0 : 0.0;
        } catch (const std::exception &e) {
            std::fprintf(stderr, "ColorMapOptimization: %s\n", e.what());
        }
        wd(o, took);
    }
    visma_icp_destroy(ctx);
    {
        ScalableTSDFVolume vol(vl, strunc, (TSDFVolumeColorType)stype, sR, stride);     // the thread's context
        for (int i = 0; i < nf; i++) vol.Integrate(stype == 2 ? frames[(size_t)i].gray : frames[(size_t)i].rgb, camera, frames[(size_t)i].E);
        wmesh(o, *vol.ExtractTriangleMesh());
    }
    std::fclose(o);
    return 0;
}
