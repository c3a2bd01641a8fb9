// colormap_driver.cpp -- color map optimization called the way an Open3D caller does, against the stand-alone header set.
// Usage: colormap_driver <in.bin> <out.bin>
//   in : int32 w, h, 4 doubles fx fy cx cy, int32 n frames, int32 n vertices, double maximum_iteration,
//        maximum_allowable_depth, then per frame 16 doubles extrinsic (row-major), w x h float depth, w x h x 3 bytes rgb,
//        then the vertices (3 doubles each)
//   out: doubles.  cicp::ColorMapOptimization on a TriangleMesh and a context of the caller's: the n extrinsics (row-major),
//        then the vertex colours; open3d::ColorMapOptimization's sibling on a PointCloud and the thread's context: the same
//        two; 1.0 if the non-rigid option threw std::invalid_argument and left poses and colours alone, else 0.0
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { if (fwrite(&v, 8, 1, o) != 1) std::exit(4); }
static void wresult(FILE *o, const PinholeCameraTrajectory &cam, const std::vector<Eigen::Vector3d> &colors)
{
    for (const auto &E : cam.extrinsic_)
        for (int i = 0; i < 16; i++) wd(o, E(i / 4, i % 4));
    for (const auto &c : colors) { wd(o, c(0)); wd(o, c(1)); wd(o, c(2)); }
}

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int32_t w, h, n, nv;
    double k[4], iterations, max_depth;
    rd(f, &w, 4); rd(f, &h, 4); rd(f, k, sizeof(k)); rd(f, &n, 4); rd(f, &nv, 4); rd(f, &iterations, 8); rd(f, &max_depth, 8);
    PinholeCameraTrajectory camera;
    camera.intrinsic_ = PinholeCameraIntrinsic(w, h, k[0], k[1], k[2], k[3]);
    std::vector<RGBDImage> frames((size_t)n);
    for (auto &fr : frames) {
        double e[16];
        rd(f, e, sizeof(e));
        Eigen::Matrix4d E;
        for (int i = 0; i < 16; i++) E(i / 4, i % 4) = e[i];
        camera.extrinsic_.push_back(E);
        fr.depth_.PrepareImage(w, h, 1, 4); rd(f, fr.depth_.data_.data(), fr.depth_.data_.size());
        fr.color_.PrepareImage(w, h, 3, 1); rd(f, fr.color_.data_.data(), fr.color_.data_.size());
    }
    TriangleMesh mesh;
    mesh.vertices_.resize((size_t)nv);
    for (auto &v : mesh.vertices_) { double p[3]; rd(f, p, sizeof(p)); v = Eigen::Vector3d(p[0], p[1], p[2]); }
    ColorMapOptmizationOption option;
    option.maximum_iteration_ = iterations;
    option.maximum_allowable_depth_ = max_depth;

    visma_icp_ctx *ctx = nullptr;
    if (visma_icp_create(&ctx, 0) != VISMA_ICP_OK) return 3;
    {
        PinholeCameraTrajectory cam = camera;
        cicp::ColorMapOptimization(ctx, mesh, frames, cam, option);
        wresult(o, cam, mesh.vertex_colors_);
    }
    visma_icp_destroy(ctx);
    {
        PinholeCameraTrajectory cam = camera;
        PointCloud cloud;
        cloud.points_ = mesh.vertices_;
        cicp::ColorMapOptimization(cloud, frames, cam, option);          // the thread's context
        wresult(o, cam, cloud.colors_);
    }
    {
        PinholeCameraTrajectory cam = camera;
        TriangleMesh other;
        other.vertices_ = mesh.vertices_;
        ColorMapOptmizationOption non_rigid = option;
        non_rigid.non_rigid_camera_coordinate_ = true;
        double threw = 0.0;
        try { ColorMapOptimization(other, frames, cam, non_rigid); } catch (const std::invalid_argument &) { threw = 1.0; }
        for (size_t i = 0; i < cam.extrinsic_.size(); i++)
            if (cam.extrinsic_[i] != camera.extrinsic_[i]) threw = 0.0;
        if (!other.vertex_colors_.empty()) threw = 0.0;
        wd(o, threw);
    }
    std::fclose(o);
    return 0;
}
