// odometry_driver.cpp -- RGB-D odometry called the way an Open3D caller does, against the stand-alone header set.
// Usage: odometry_driver <in.bin> <out.bin>
//   in : int32 w, h, method (0 colour, 1 hybrid), n_levels, n_levels x int32 iterations, double max_depth_diff, min_depth,
//        max_depth, 4 doubles fx fy cx cy, 16 doubles odo_init (row-major), then four w x h float images: source gray,
//        source depth, target gray, target depth
//   out: per call {success, 16 doubles T, 36 doubles information}: cicp::ComputeRGBDOdometry on a context of its own, the
//        same on the thread's context, and a call whose target is one column narrower (a size mismatch)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { if (fwrite(&v, 8, 1, o) != 1) std::exit(4); }
static void image(FILE *f, Image &im, int w, int h)
{
    im.PrepareImage(w, h, 1, 4);
    rd(f, im.data_.data(), im.data_.size());
    *PointerAt<float>(im, 0, 0) = *PointerAt<float>(im, 0, 0, 0);          // (both forms address the same pixel)
}
static void write(FILE *o, const std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d> &r)
{
    wd(o, std::get<0>(r) ? 1.0 : 0.0);
    for (int i = 0; i < 16; i++) wd(o, std::get<1>(r)(i / 4, i % 4));
    for (int i = 0; i < 36; i++) wd(o, std::get<2>(r)(i / 6, i % 6));
}

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int32_t w, h, method, n;
    rd(f, &w, 4); rd(f, &h, 4); rd(f, &method, 4); rd(f, &n, 4);
    std::vector<int> its((size_t)n);
    rd(f, its.data(), 4 * (size_t)n);
    double od[3], k[4], init[16];
    rd(f, od, sizeof(od)); rd(f, k, sizeof(k)); rd(f, init, sizeof(init));
    RGBDImage source, target;
    image(f, source.color_, w, h); image(f, source.depth_, w, h); image(f, target.color_, w, h); image(f, target.depth_, w, h);
    const PinholeCameraIntrinsic camera(w, h, k[0], k[1], k[2], k[3]);
    const OdometryOption option(its, od[0], od[1], od[2]);
    Eigen::Matrix4d odo_init;
    for (int i = 0; i < 16; i++) odo_init(i / 4, i % 4) = init[i];
    const RGBDOdometryJacobianFromColorTerm color;
    const RGBDOdometryJacobianFromHybridTerm hybrid;
    const RGBDOdometryJacobian &jacobian = method == 0 ? static_cast<const RGBDOdometryJacobian &>(color) : hybrid;

    visma_icp_ctx *ctx = nullptr;
    if (visma_icp_create(&ctx, 0) != VISMA_ICP_OK) return 3;
    write(o, cicp::ComputeRGBDOdometry(ctx, source, target, camera, odo_init, jacobian, option));
    write(o, cicp::ComputeRGBDOdometry(source, target, camera, odo_init, jacobian, option));
    RGBDImage narrow;
    narrow.color_.PrepareImage(w - 1, h, 1, 4); narrow.depth_.PrepareImage(w - 1, h, 1, 4);
    write(o, cicp::ComputeRGBDOdometry(ctx, source, narrow, camera, odo_init, jacobian, option));
    visma_icp_destroy(ctx);
    std::fclose(o);
    return 0;
}
