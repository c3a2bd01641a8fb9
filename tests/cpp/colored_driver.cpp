// colored_driver.cpp -- colored ICP called the way an Open3D caller does, against the stand-alone header set.
// Usage: colored_driver host|run <in.bin> <out.bin>
//   in : int64 ns, int64 nt, int64 K, double lambda_geometric, double radius, int32 max_iteration, int32 pad,
//        ns*3 doubles (source), nt*3 doubles (target), nt*3 doubles (target normals), ns*3 doubles (source colours),
//        nt*3 doubles (target colours), nt*3 doubles (the target's colour gradient), K * 2 int32 correspondences
//   host (no GPU): cicp::TransformationEstimationForColoredICP(lambda) with color_gradient_ set; out:
//        double lambda_geometric_ as the constructor left it, double ComputeRMSE, 16 doubles ComputeTransformation
//        (row-major), 38 doubles host statistics, double their cost, double ComputeRMSE and 16 doubles
//        ComputeTransformation WITHOUT a gradient (0 and the identity)
//   run  (GPU): open3d::RegistrationColoredICP(source, target, radius, I, ICPConvergenceCriteria(1e-6, 1e-6,
//        max_iteration), lambda); out: 16 doubles T, double fitness, double inlier_rmse, int64 n, n * 2 int32 correspondences
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    if (argc < 4) return 2;
    const bool host = std::strcmp(argv[1], "host") == 0;
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    int64_t ns, nt, K;
    double lambda, radius;
    int32_t iters, pad;
    if (fread(&ns, 8, 1, f) != 1 || fread(&nt, 8, 1, f) != 1 || fread(&K, 8, 1, f) != 1 || fread(&lambda, 8, 1, f) != 1 ||
        fread(&radius, 8, 1, f) != 1 || fread(&iters, 4, 1, f) != 1 || fread(&pad, 4, 1, f) != 1)
        return 2;
    PointCloud source, target;
    std::vector<Eigen::Vector3d> grad;
    read_cloud(f, source.points_, ns);
    read_cloud(f, target.points_, nt);
    read_cloud(f, target.normals_, nt);
    read_cloud(f, source.colors_, ns);
    read_cloud(f, target.colors_, nt);
    read_cloud(f, grad, nt);
    CorrespondenceSet corres((size_t)K);
    for (int64_t i = 0; i < K; i++) {
        int32_t p[2];
        if (fread(p, 4, 2, f) != 2) return 2;
        corres[(size_t)i] = Eigen::Vector2i(p[0], p[1]);
    }
    std::fclose(f);
    FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    try {
        if (host) {
            cicp::TransformationEstimationForColoredICP est(lambda);
            const double bare_rmse = est.ComputeRMSE(source, target, corres);
            const Eigen::Matrix4d bare_T = est.ComputeTransformation(source, target, corres);
            est.color_gradient_ = grad;
            const double rmse = est.ComputeRMSE(source, target, corres);
            const Eigen::Matrix4d T = est.ComputeTransformation(source, target, corres);
            double st[VISMA_ICP_NSTATS];
            const double cost = cicp::detail::host_stats_colored(source, target, corres, grad, est.lambda_geometric_, st);
            if (fwrite(&est.lambda_geometric_, 8, 1, o) != 1 || fwrite(&rmse, 8, 1, o) != 1 || write_T(o, T) ||
                fwrite(st, 8, VISMA_ICP_NSTATS, o) != VISMA_ICP_NSTATS || fwrite(&cost, 8, 1, o) != 1 ||
                fwrite(&bare_rmse, 8, 1, o) != 1 || write_T(o, bare_T))
                return 4;
        } else {
            const RegistrationResult one = open3d::RegistrationColoredICP(source, target, radius, Eigen::Matrix4d::Identity(),
                                                                          ICPConvergenceCriteria(1e-6, 1e-6, iters), lambda);
            const double fr[2] = {one.fitness_, one.inlier_rmse_};
            const int64_t n = (int64_t)one.correspondence_set_.size();
            if (write_T(o, one.transformation_) || fwrite(fr, 8, 2, o) != 2 || fwrite(&n, 8, 1, o) != 1) return 4;
            for (const auto &c : one.correspondence_set_) {
                const int32_t p[2] = {c[0], c[1]};
                if (fwrite(p, 4, 2, o) != 2) return 4;
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::fclose(o);
    return 0;
}
