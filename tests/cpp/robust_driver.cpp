// robust_driver.cpp -- robust ICP called the way an Open3D caller does: the two estimator classes handed to the stock
// open3d::RegistrationICP of the stand-alone header set, and RegisterModelToScene with its `robust` argument.
// Usage: robust_driver <in.bin> <out.bin>
//   in : int64 ns, int64 nt, double radius, int32 kernel, int32 max_iteration, int32 rotation_level, int32 pad,
//        ns*3 doubles (source), nt*3 doubles (target), nt*3 doubles (target normals)
//   out: three times {16 doubles T (row-major), double fitness, double inlier_rmse, int64 n, n * 2 int32 correspondences}:
//        open3d::RegistrationICP(source, target, radius, I, cicp::TransformationEstimationPointToPointRobust(kernel),
//        ICPConvergenceCriteria(1e-6, 1e-6, max_iteration)), the same with cicp::TransformationEstimationPointToPlaneRobust,
//        then cicp::RegisterModelToScene(source, target, rotation_level, radius, false, &best, false, 1.0, &kernel);
//        then one int32: 1 iff RegisterModelToScene with keep = 0.5 AND robust weights returned an empty result
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

static int write_result(FILE *o, const RegistrationResult &r)
{
    double T[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) T[i * 4 + j] = r.transformation_(i, j);
    const double fr[2] = {r.fitness_, r.inlier_rmse_};
    const int64_t n = (int64_t)r.correspondence_set_.size();
    if (fwrite(T, 8, 16, o) != 16 || fwrite(fr, 8, 2, o) != 2 || fwrite(&n, 8, 1, o) != 1) return 4;
    for (const auto &c : r.correspondence_set_) {
        const int32_t p[2] = {c[0], c[1]};
        if (fwrite(p, 4, 2, o) != 2) return 4;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t ns, nt;
    double radius;
    int32_t kernel, iters, level, pad;
    if (fread(&ns, 8, 1, f) != 1 || fread(&nt, 8, 1, f) != 1 || fread(&radius, 8, 1, f) != 1 || fread(&kernel, 4, 1, f) != 1 ||
        fread(&iters, 4, 1, f) != 1 || fread(&level, 4, 1, f) != 1 || fread(&pad, 4, 1, f) != 1)
        return 2;
    PointCloud source, target;
    read_cloud(f, source.points_, ns);
    read_cloud(f, target.points_, nt);
    read_cloud(f, target.normals_, nt);
    std::fclose(f);
    source.normals_.assign((size_t)ns, Eigen::Vector3d(0.0, 0.0, 1.0));   // (RegistrationICP asks both clouds for normals)
    RegistrationResult one, plane, best, both;
    int32_t both_refused = 0;
    try {
        const cicp::RobustKernel k((cicp::RobustKernel::Type)kernel);
        one = open3d::RegistrationICP(source, target, radius, Eigen::Matrix4d::Identity(),
                                      cicp::TransformationEstimationPointToPointRobust(k), ICPConvergenceCriteria(1e-6, 1e-6, iters));
        plane = open3d::RegistrationICP(source, target, radius, Eigen::Matrix4d::Identity(),
                                        cicp::TransformationEstimationPointToPlaneRobust(k), ICPConvergenceCriteria(1e-6, 1e-6, iters));
        cicp::RegisterModelToScene(source, target, level, radius, false, &best, false, 1.0, &k);
        both.fitness_ = -1.0;
        const Eigen::Matrix4d Tb = cicp::RegisterModelToScene(source, target, level, radius, false, &both, false, 0.5, &k);
        both_refused = Tb.isIdentity() && both.fitness_ == -1.0 ? 1 : 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    if (int rc = write_result(o, one)) return rc;
    if (int rc = write_result(o, plane)) return rc;
    if (int rc = write_result(o, best)) return rc;
    if (fwrite(&both_refused, 4, 1, o) != 1) return 4;
    std::fclose(o);
    return 0;
}
