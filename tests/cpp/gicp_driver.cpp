// gicp_driver.cpp -- generalized ICP called the way an Open3D caller does: cicp::TransformationEstimationGeneralized handed
// to the stock open3d::RegistrationICP of the stand-alone header set, then the estimator's own ComputeRMSE and
// ComputeTransformation (the host restatements) over the correspondences that came back.
// Usage: gicp_driver <in.bin> <out.bin>
//   in : int64 ns, int64 nt, double radius, double epsilon, int32 max_iteration, int32 pad,
//        ns*3 doubles (source), nt*3 doubles (target), ns*3 doubles (source normals), nt*3 doubles (target normals)
//   out: {16 doubles T (row-major), double fitness, double inlier_rmse, int64 n, n * 2 int32 correspondences} of
//        open3d::RegistrationICP(source, target, radius, I, cicp::TransformationEstimationGeneralized(epsilon),
//        ICPConvergenceCriteria(1e-6, 1e-6, max_iteration)); then, with the source moved by that T, double ComputeRMSE and
//        16 doubles ComputeTransformation over those correspondences; then one int32: 1 iff a run WITHOUT source normals
//        returned the initial transform and no correspondences
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "constrained_ICP.h"

using namespace open3d;

static void read_cloud(FILE *f, std::vector<Eigen::Vector3d> &v, int64_t n)
{
    v.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        double p[3];
        if (fread(p, 8, 3, f) != 3) std::exit(2);
        v[(size_t)i] = Eigen::Vector3d(p[0], p[1], p[2]);
    }
}

static int write_T(FILE *o, const Eigen::Matrix4d &M)
{
    double T[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) T[i * 4 + j] = M(i, j);
    return fwrite(T, 8, 16, o) == 16 ? 0 : 4;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t ns, nt;
    double radius, epsilon;
    int32_t iters, pad;
    if (fread(&ns, 8, 1, f) != 1 || fread(&nt, 8, 1, f) != 1 || fread(&radius, 8, 1, f) != 1 || fread(&epsilon, 8, 1, f) != 1 ||
        fread(&iters, 4, 1, f) != 1 || fread(&pad, 4, 1, f) != 1)
        return 2;
    PointCloud source, target;
    read_cloud(f, source.points_, ns);
    read_cloud(f, target.points_, nt);
    read_cloud(f, source.normals_, ns);
    read_cloud(f, target.normals_, nt);
    std::fclose(f);
    RegistrationResult one, none;
    double host_rmse = 0.0;
    Eigen::Matrix4d host_update = Eigen::Matrix4d::Identity();
    int32_t init_returned = 0;
    try {
        const cicp::TransformationEstimationGeneralized est(epsilon);
        one = open3d::RegistrationICP(source, target, radius, Eigen::Matrix4d::Identity(), est, ICPConvergenceCriteria(1e-6, 1e-6, iters));
        // the host restatements, over the source as the last pass saw it (points moved, normals turned)
        PointCloud moved = source;
        const Eigen::Matrix3d R = one.transformation_.block<3, 3>(0, 0);
        const Eigen::Vector3d t = one.transformation_.block<3, 1>(0, 3);
        for (size_t i = 0; i < moved.points_.size(); i++) {
            moved.points_[i] = R * source.points_[i] + t;
            moved.normals_[i] = R * source.normals_[i];
        }
        host_rmse = est.ComputeRMSE(moved, target, one.correspondence_set_);
        host_update = est.ComputeTransformation(moved, target, one.correspondence_set_);
        PointCloud bare = source;
        bare.normals_.clear();
        Eigen::Matrix4d init = Eigen::Matrix4d::Identity();
        init(0, 3) = 0.125;
        none = open3d::RegistrationICP(bare, target, radius, init, est, ICPConvergenceCriteria(1e-6, 1e-6, iters));
        init_returned = none.transformation_ == init && none.correspondence_set_.empty() ? 1 : 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const double fr[2] = {one.fitness_, one.inlier_rmse_};
    const int64_t n = (int64_t)one.correspondence_set_.size();
    if (write_T(o, one.transformation_) || fwrite(fr, 8, 2, o) != 2 || fwrite(&n, 8, 1, o) != 1) return 4;
    for (const auto &c : one.correspondence_set_) {
        const int32_t p[2] = {c[0], c[1]};
        if (fwrite(p, 4, 2, o) != 2) return 4;
    }
    if (fwrite(&host_rmse, 8, 1, o) != 1 || write_T(o, host_update) || fwrite(&init_returned, 4, 1, o) != 1) return 4;
    std::fclose(o);
    return 0;
}
