// colormap_warp_driver.cpp -- the non-rigid color map optimization called the way an Open3D caller does, against the
// stand-alone header set.
// Usage: colormap_warp_driver <in.bin> <out.bin>
//   in : int32 w, h, 4 doubles fx fy cx cy, int32 n frames, int32 n vertices, double maximum_iteration,
//        maximum_allowable_depth, int32 number_of_vertical_anchors, double non_rigid_anchor_point_weight, then per frame 16
//        doubles extrinsic (row-major), w x h float depth, w x h x 3 bytes rgb, then the vertices (3 doubles each)
//   out: doubles.  cicp::ColorMapOptimizationNonRigid on a TriangleMesh and a context of the caller's, the option's flag NOT
//        set: the n extrinsics (row-major), then the vertex colours; on a PointCloud and the thread's context, the flag set:
//        the same two; the staged calls of visma_icp.h (create_non_rigid ... run, get_colors, get_extrinsics): the same two;
//        then 1.0 if ColorMapOptimization with the flag set threw std::invalid_argument, named the new function and left
//        poses and colours alone, else 0.0
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    int32_t w, h, n, nv, anchors;
    double k[4], iterations, max_depth, weight;
    rd(f, &w, 4); rd(f, &h, 4); rd(f, k, sizeof(k)); rd(f, &n, 4); rd(f, &nv, 4); rd(f, &iterations, 8); rd(f, &max_depth, 8);
    rd(f, &anchors, 4); rd(f, &weight, 8);
    PinholeCameraTrajectory camera;
    camera.intrinsic_ = PinholeCameraIntrinsic(w, h, k[0], k[1], k[2], k[3]);
    std::vector<RGBDImage> frames((size_t)n);
    std::vector<double> E0;
    for (auto &fr : frames) {
        double e[16];
        rd(f, e, sizeof(e));
        E0.insert(E0.end(), e, e + 16);
        Eigen::Matrix4d E;
        for (int i = 0; i < 16; i++) E(i / 4, i % 4) = e[i];
        camera.extrinsic_.push_back(E);
        fr.depth_.PrepareImage(w, h, 1, 4); rd(f, fr.depth_.data_.data(), fr.depth_.data_.size());
        fr.color_.PrepareImage(w, h, 3, 1); rd(f, fr.color_.data_.data(), fr.color_.data_.size());
    }
    TriangleMesh mesh;
    mesh.vertices_.resize((size_t)nv);
    std::vector<double> V;
    for (auto &v : mesh.vertices_) { double p[3]; rd(f, p, sizeof(p)); v = Eigen::Vector3d(p[0], p[1], p[2]); V.insert(V.end(), p, p + 3); }
    ColorMapOptmizationOption option;
    option.maximum_iteration_ = iterations;
    option.maximum_allowable_depth_ = max_depth;
    option.number_of_vertical_anchors_ = anchors;
    option.non_rigid_anchor_point_weight_ = weight;

    visma_icp_ctx *ctx = nullptr;
    if (visma_icp_create(&ctx, 0) != VISMA_ICP_OK) return 3;
    {
        PinholeCameraTrajectory cam = camera;
        cicp::ColorMapOptimizationNonRigid(ctx, mesh, frames, cam, option);          // the flag is not set: it is not read
        wresult(o, cam, mesh.vertex_colors_);
    }
    {
        PinholeCameraTrajectory cam = camera;
        PointCloud cloud;
        cloud.points_ = mesh.vertices_;
        ColorMapOptmizationOption flagged = option;
        flagged.non_rigid_camera_coordinate_ = true;
        cicp::ColorMapOptimizationNonRigid(cloud, frames, cam, flagged);             // the thread's context
        wresult(o, cam, cloud.colors_);
    }
    {
        visma_icp_color_map_option co;
        visma_icp_color_map_option_default(&co);
        co.maximum_iteration = iterations; co.maximum_allowable_depth = max_depth; co.number_of_vertical_anchors = anchors;
        co.non_rigid_anchor_point_weight = weight;
        visma_icp_color_map *map = nullptr;
        if (visma_icp_color_map_create_non_rigid(ctx, w, h, n, k, &co, &map) != VISMA_ICP_OK) return 5;
        for (int i = 0; i < n; i++)
            if (visma_icp_color_map_set_image(ctx, map, i, (const float *)frames[(size_t)i].depth_.data_.data(), frames[(size_t)i].color_.data_.data(), 3,
                                              E0.data() + 16 * (size_t)i) != VISMA_ICP_OK) return 5;
        std::vector<double> E((size_t)n * 16), colors((size_t)nv * 3);
        if (visma_icp_color_map_set_vertices(ctx, map, V.data(), nv) != VISMA_ICP_OK || visma_icp_color_map_prepare(ctx, map, nullptr) != VISMA_ICP_OK ||
            visma_icp_color_map_run(ctx, map, -1, nullptr) != VISMA_ICP_OK || visma_icp_color_map_get_colors(ctx, map, colors.data(), nv) != VISMA_ICP_OK ||
            visma_icp_color_map_get_extrinsics(ctx, map, E.data()) != VISMA_ICP_OK || visma_icp_color_map_destroy(ctx, map) != VISMA_ICP_OK)
            return 5;
        for (double v : E) wd(o, v);
        for (double v : colors) wd(o, v);
    }
    visma_icp_destroy(ctx);
    {
        PinholeCameraTrajectory cam = camera;
        TriangleMesh other;
        other.vertices_ = mesh.vertices_;
        ColorMapOptmizationOption flagged = option;
        flagged.non_rigid_camera_coordinate_ = true;
        double threw = 0.0;
        try { ColorMapOptimization(other, frames, cam, flagged); }
        catch (const std::invalid_argument &e) { threw = std::strstr(e.what(), "ColorMapOptimizationNonRigid") ? 1.0 : 0.0; }
        for (size_t i = 0; i < cam.extrinsic_.size(); i++)
            if (cam.extrinsic_[i] != camera.extrinsic_[i]) threw = 0.0;
        if (!other.vertex_colors_.empty()) threw = 0.0;
        wd(o, threw);
    }
    std::fclose(o);
    return 0;
}
