// cloud_driver.cpp -- open3d::PointCloud's members and the free functions of Core/Geometry/PointCloud.h called with the
// reference's names and signatures, against the stand-alone header set.
// Usage: cloud_driver <in.bin> <out.bin>
//   in : doubles (tests/cloud_cases.py: encode).  n, has normals, has colours, the rows, then a program: k steps of {code,
//        arguments} -- 0 Transform(16, row-major), 1 NormalizeNormals, 2 PaintUniformColor(3), 4 GetMinBound / GetMaxBound,
//        5 SelectDownSample(n, indices), 6 UniformDownSample(k), 7 CropPointCloud(min, max), 8 OrientNormalsToAlignWithDirection(3),
//        9 OrientNormalsTowardsCameraLocation(3), 10 ComputePointCloudMeanAndCovariance, 11 ComputePointCloudMahalanobisDistance
//   out: doubles.  The cloud behind the program as {n, rows} for points, normals, colours, then HasNormals, HasColors; the
//        number of result doubles and the results of steps 4, 10 and 11 in order; the same program on a cicp::DevicePointCloud
//        (one upload, one download) the same way; 1.0 if cicp::ExtractPointCloud(volume) of a small UniformTSDFVolume,
//        downloaded, equals ExtractPointCloud() bit for bit, else 0.0; 1.0 if its Crop, VoxelDownSample, EstimateNormals on
//        the device equal CropPointCloud, VoxelDownSample, EstimateNormals of the host cloud bit for bit, else 0.0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static double rd(FILE *f) { double v; if (fread(&v, 8, 1, f) != 1) std::exit(2); return v; }
static void wd(FILE *o, double v) { if (fwrite(&v, 8, 1, o) != 1) std::exit(4); }
static void rows(FILE *f, std::vector<Eigen::Vector3d> &a, size_t n) { a.resize(n); for (auto &p : a) { p(0) = rd(f); p(1) = rd(f); p(2) = rd(f); } }
static void wrows(FILE *o, const std::vector<Eigen::Vector3d> &a) { wd(o, (double)a.size()); for (const auto &p : a) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); } }
static Eigen::Vector3d vec(const double *a) { return Eigen::Vector3d(a[0], a[1], a[2]); }
static void wcloud(FILE *o, const PointCloud &c, const std::vector<double> &results)
{
    wrows(o, c.points_); wrows(o, c.normals_); wrows(o, c.colors_);
    wd(o, (double)c.HasNormals()); wd(o, (double)c.HasColors());
    wd(o, (double)results.size());
    for (double r : results) wd(o, r);
}
static bool same_rows(const std::vector<Eigen::Vector3d> &a, const std::vector<Eigen::Vector3d> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a[0].data(), b[0].data(), a.size() * sizeof(a[0])) == 0);
}
static bool same_cloud(const PointCloud &a, const PointCloud &b)
{
    return same_rows(a.points_, b.points_) && same_rows(a.normals_, b.normals_) && same_rows(a.colors_, b.colors_);
}
static void push3(std::vector<double> &r, const Eigen::Vector3d &v) { for (int i = 0; i < 3; i++) r.push_back(v(i)); }
static void push_stats(std::vector<double> &r, const std::tuple<Eigen::Vector3d, Eigen::Matrix3d> &mc)
{
    push3(r, std::get<0>(mc));
    for (int i = 0; i < 9; i++) r.push_back(std::get<1>(mc)(i / 3, i % 3));
}

struct Step { int op; std::vector<double> arg; };

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    PointCloud input;
    const size_t n = (size_t)rd(f);
    const bool hn = rd(f) != 0, hc = rd(f) != 0;
    rows(f, input.points_, n);
    if (hn) rows(f, input.normals_, n);
    if (hc) rows(f, input.colors_, n);
    std::vector<Step> program((size_t)rd(f));
    for (Step &s : program) {
        s.op = (int)rd(f);
        size_t args = 0;
        switch (s.op) {
        case 0: args = 16; break;
        case 2: case 8: case 9: args = 3; break;
        case 5: args = (size_t)rd(f); break;
        case 6: args = 1; break;
        case 7: args = 6; break;
        case 1: case 4: case 10: case 11: break;
        default: return 3;
        }
        s.arg.resize(args);
        for (double &a : s.arg) a = rd(f);
    }

    // the reference's names on host clouds
    {
        PointCloud m = input;
        std::vector<double> results;
        for (const Step &s : program) {
            const double *a = s.arg.data();
            switch (s.op) {
            case 0: { Eigen::Matrix4d M; for (int i = 0; i < 16; i++) M(i / 4, i % 4) = a[i]; m.Transform(M); break; }
            case 1: m.NormalizeNormals(); break;
            case 2: m.PaintUniformColor(vec(a)); break;
            case 4: push3(results, m.GetMinBound()); push3(results, m.GetMaxBound()); break;
            case 5: { std::vector<size_t> idx(s.arg.begin(), s.arg.end()); std::shared_ptr<PointCloud> out = SelectDownSample(m, idx); m = *out; break; }
            case 6: { std::shared_ptr<PointCloud> out = UniformDownSample(m, (size_t)a[0]); m = *out; break; }
            case 7: { std::shared_ptr<PointCloud> out = CropPointCloud(m, vec(a), vec(a + 3)); m = *out; break; }
            case 8: OrientNormalsToAlignWithDirection(m, vec(a)); break;
            case 9: OrientNormalsTowardsCameraLocation(m, vec(a)); break;
            case 10: push_stats(results, ComputePointCloudMeanAndCovariance(m)); break;
            case 11: { const std::vector<double> d = ComputePointCloudMahalanobisDistance(m); results.insert(results.end(), d.begin(), d.end()); break; }
            }
        }
        wcloud(o, m, results);
    }
    // the same program on one resident cloud
    {
        cicp::DevicePointCloud d(input);
        std::vector<double> results;
        for (const Step &s : program) {
            const double *a = s.arg.data();
            switch (s.op) {
            case 0: { Eigen::Matrix4d M; for (int i = 0; i < 16; i++) M(i / 4, i % 4) = a[i]; d.Transform(M); break; }
            case 1: d.NormalizeNormals(); break;
            case 2: d.PaintUniformColor(vec(a)); break;
            case 4: push3(results, d.GetMinBound()); push3(results, d.GetMaxBound()); break;
            case 5: { std::vector<size_t> idx(s.arg.begin(), s.arg.end()); d = d.Select(idx); break; }
            case 6: d = d.UniformDownSample((size_t)a[0]); break;
            case 7: d = d.Crop(vec(a), vec(a + 3)); break;
            case 8: d.OrientNormalsToAlignWithDirection(vec(a)); break;
            case 9: d.OrientNormalsTowardsCameraLocation(vec(a)); break;
            case 10: push_stats(results, d.MeanAndCovariance()); break;
            case 11: { const std::vector<double> r = d.MahalanobisDistance(); results.insert(results.end(), r.begin(), r.end()); break; }
            }
        }
        wcloud(o, *d.Download(), results);
    }

    // the volume's cloud handed over on the device: 8^3 voxels of 0.125 in front of a tilted 33 x 33 frame
    double handed = 0.0, chained = 0.0;
    {
        UniformTSDFVolume vol(1.0, 8, 0.3, TSDFVolumeColorType::RGB8, Eigen::Vector3d(-0.5, -0.5, 0.125));
        RGBDImage frame;
        frame.depth_.PrepareImage(33, 33, 1, 4);
        frame.color_.PrepareImage(33, 33, 3, 1);
        float *depth = reinterpret_cast<float *>(frame.depth_.data_.data());
        for (int i = 0; i < 33 * 33; i++) {
            depth[i] = 0.5f + 0.006f * (float)(i % 33) + 0.003f * (float)(i / 33);
            for (int c = 0; c < 3; c++) frame.color_.data_[3 * i + c] = (uint8_t)(i + 40 * c);
        }
        vol.Integrate(frame, PinholeCameraIntrinsic(33, 33, 16.0, 16.0, 16.0, 16.0), Eigen::Matrix4d::Identity());
        TSDFVolume &base = vol;
        std::shared_ptr<PointCloud> host = base.ExtractPointCloud();
        cicp::DevicePointCloud device = cicp::ExtractPointCloud(base);
        handed = host->points_.size() > 20 && host->HasNormals() && host->HasColors() && same_cloud(*host, *device.Download()) ? 1.0 : 0.0;
        const Eigen::Vector3d lo(-0.4, -0.3, 0.0), hi(0.3, 0.4, 2.0);
        const KDTreeSearchParamHybrid param(0.3, 8);
        std::shared_ptr<PointCloud> down = VoxelDownSample(*CropPointCloud(*host, lo, hi), 0.2);
        EstimateNormals(*down, param);
        cicp::DevicePointCloud chain = device.Crop(lo, hi).VoxelDownSample(0.2);
        chain.EstimateNormals(param);
        chained = down->points_.size() > 3 && down->points_.size() < host->points_.size() && same_cloud(*down, *chain.Download()) ? 1.0 : 0.0;
    }
    wd(o, handed);
    wd(o, chained);
    std::fclose(o);
    return 0;
}
