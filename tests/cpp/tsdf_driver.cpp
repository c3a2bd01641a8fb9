// tsdf_driver.cpp -- TSDF integration called the way an Open3D caller does, against the stand-alone header set.
// Usage: tsdf_driver <in.bin> <out.bin>
//   in : int32 w, h, 4 doubles fx fy cx cy, int32 n frames, int32 resolution, colour type (0 none, 1 rgb8, 2 gray32), double
//        length, sdf_trunc, 3 doubles origin, then per frame 16 doubles extrinsic (row-major), w x h float depth, w x h x 3
//        bytes rgb, w x h float gray
//   out: doubles.  The volume (tsdf, weight, colour as the reference interleaves it) after the first and after the last
//        frame, on a context of the caller's; ExtractPointCloud and ExtractVoxelPointCloud of it as {n points, n normals, n
//        colours, the rows}; the same two extractions of a second volume on the thread's context after Reset() and the same
//        frames; CreatePointCloudFromDepthImage of frame 0 (identity, stride 4) and CreatePointCloudFromRGBDImage of frame 0
//        with the volume's colour (gray for a volume without); 1.0 if an Integrate with a depth image one column narrower
//        threw std::invalid_argument, else 0.0
//   in, behind the frames: int32 unit resolution, stride, colour type, frames to use, the pool's first capacity, double
//        voxel_length, sdf_trunc of a ScalableTSDFVolume
//   out, behind the above: per frame {n units, their indices}; per final unit, in that order, its volume; the two extractions
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { if (fwrite(&v, 8, 1, o) != 1) std::exit(4); }
static void wvec(FILE *o, const std::vector<Eigen::Vector3d> &v) { for (const auto &p : v) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); } }
static void wcloud(FILE *o, const PointCloud &pc)
{
    wd(o, (double)pc.points_.size()); wd(o, (double)pc.normals_.size()); wd(o, (double)pc.colors_.size());
    wvec(o, pc.points_); wvec(o, pc.normals_); wvec(o, pc.colors_);
}
static void wvol(FILE *o, const UniformTSDFVolume &v)
{
    std::vector<float> tsdf, weight;
    std::vector<Eigen::Vector3f> color;
    v.Download(tsdf, weight, color);
    for (float f : tsdf) wd(o, (double)f);
    for (float f : weight) wd(o, (double)f);
    for (const auto &c : color) { wd(o, (double)c(0)); wd(o, (double)c(1)); wd(o, (double)c(2)); }
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
    const PinholeCameraIntrinsic camera(w, h, k[0], k[1], k[2], k[3]);
    const TSDFVolumeColorType type = (TSDFVolumeColorType)ctype;
    const Eigen::Vector3d origin(org[0], org[1], org[2]);
    auto image = [&](const Frame &fr) -> const RGBDImage & { return ctype == 2 ? fr.gray : fr.rgb; };

    visma_icp_ctx *ctx = nullptr;
    if (visma_icp_create(&ctx, 0) != VISMA_ICP_OK) return 3;
    {
        UniformTSDFVolume vol(ctx, length, R, trunc, type, origin);
        TSDFVolume &base = vol;                                          // (through the interface, as a pipeline holds it)
        for (int i = 0; i < n; i++) {
            base.Integrate(image(frames[(size_t)i]), camera, frames[(size_t)i].E);
            if (i == 0 || i == n - 1) wvol(o, vol);
        }
        wcloud(o, *base.ExtractPointCloud());
        wcloud(o, *vol.ExtractVoxelPointCloud());
    }
    visma_icp_destroy(ctx);
    {
        UniformTSDFVolume vol(length, R, trunc, type, origin);           // the thread's context
        vol.Integrate(image(frames[0]), camera, frames[0].E);
        vol.Reset();
        for (const auto &fr : frames) vol.Integrate(image(fr), camera, fr.E);
        wcloud(o, *vol.ExtractPointCloud());
        wcloud(o, *vol.ExtractVoxelPointCloud());
        wcloud(o, *CreatePointCloudFromDepthImage(frames[0].rgb.depth_, camera, Eigen::Matrix4d::Identity(), 1000.0, 1000.0, 4));
        wcloud(o, *CreatePointCloudFromRGBDImage(ctype == 1 ? frames[0].rgb : frames[0].gray, camera));
        RGBDImage narrow = image(frames[0]);
        narrow.depth_.PrepareImage(w - 1, h, 1, 4);
        double threw = 0.0;
        try { vol.Integrate(narrow, camera, frames[0].E); } catch (const std::invalid_argument &) { threw = 1.0; }
        wd(o, threw);
    }
    {
        int32_t sR, stride, stype, nf, initial;
        double vl, strunc;
        rd(f, &sR, 4); rd(f, &stride, 4); rd(f, &stype, 4); rd(f, &nf, 4); rd(f, &initial, 4); rd(f, &vl, 8); rd(f, &strunc, 8);
        visma_icp_ctx *sctx = nullptr;
        if (visma_icp_create(&sctx, 0) != VISMA_ICP_OK) return 3;
        {
            ScalableTSDFVolume vol(sctx, vl, strunc, (TSDFVolumeColorType)stype, sR, stride, initial);
            for (int i = 0; i < nf; i++) {
                const Frame &fr = frames[(size_t)i];
                vol.Integrate(stype == 2 ? fr.gray : fr.rgb, camera, fr.E);
                const auto units = vol.Units();
                wd(o, (double)units.size());
                for (const auto &u : units) { wd(o, u(0)); wd(o, u(1)); wd(o, u(2)); }
            }
            std::vector<float> tsdf, weight;
            std::vector<Eigen::Vector3f> color;
            for (const auto &u : vol.Units()) {
                if (!vol.DownloadUnit(u, tsdf, weight, color)) return 5;
                for (float v : tsdf) wd(o, (double)v);
                for (float v : weight) wd(o, (double)v);
                for (const auto &c : color) { wd(o, (double)c(0)); wd(o, (double)c(1)); wd(o, (double)c(2)); }
            }
            if (vol.DownloadUnit(Eigen::Vector3i(100000, 0, 0), tsdf, weight, color)) return 6;
            wcloud(o, *vol.ExtractPointCloud());
            wcloud(o, *vol.ExtractVoxelPointCloud());
        }
        visma_icp_destroy(sctx);
    }
    std::fclose(o);
    return 0;
}
