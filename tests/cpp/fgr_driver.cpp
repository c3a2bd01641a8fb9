// fgr_driver.cpp -- FPFH and fast global registration called the way an Open3D caller does, against the stand-alone
// header set.
// Usage: fgr_driver host|run <in.bin> <out.bin>
//   in : int64 ns, int64 nt, int64 K, double division_factor, double maximum_correspondence_distance, double tuple_scale,
//        double radius, int32 use_absolute_scale, int32 decrease_mu, int32 iteration_number, int32 maximum_tuple_count,
//        int32 max_nn, int32 pad, int64 seed, ns*3 doubles (source), ns*3 doubles (source normals), nt*3 doubles (target),
//        nt*3 doubles (target normals), K * 2 int32 correspondences
//   host (no GPU): cicp::detail::fgr_optimize over the K pairs; out: 16 doubles T source-to-target (row-major), 16 doubles
//        the optimisation's own result
//   run  (GPU): open3d::ComputeFPFHFeature(cloud, KDTreeSearchParamHybrid(radius, max_nn)) of both clouds, then
//        open3d::cicp::FastGlobalRegistration(source, target, fs, ft, option, seed); out: 16 doubles T, ns * 33 doubles
//        the source's features, point-major
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
    int64_t ns, nt, K, seed;
    double d[4];
    int32_t iv[6];
    if (fread(&ns, 8, 1, f) != 1 || fread(&nt, 8, 1, f) != 1 || fread(&K, 8, 1, f) != 1 || fread(d, 8, 4, f) != 4 ||
        fread(iv, 4, 6, f) != 6 || fread(&seed, 8, 1, f) != 1)
        return 2;
    PointCloud source, target;
    read_cloud(f, source.points_, ns);
    read_cloud(f, source.normals_, ns);
    read_cloud(f, target.points_, nt);
    read_cloud(f, target.normals_, nt);
    CorrespondenceSet corres((size_t)K);
    for (int64_t i = 0; i < K; i++) {
        int32_t p[2];
        if (fread(p, 4, 2, f) != 2) return 2;
        corres[(size_t)i] = Eigen::Vector2i(p[0], p[1]);
    }
    std::fclose(f);
    const FastGlobalRegistrationOption option(d[0], iv[0] != 0, iv[1] != 0, d[1], iv[2], d[2], iv[3]);
    FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    try {
        if (host) {
            Eigen::Matrix4d opt;
            const Eigen::Matrix4d T = cicp::detail::fgr_optimize(source, target, corres, option, &opt);
            if (write_T(o, T) || write_T(o, opt)) return 4;
        } else {
            const KDTreeSearchParamHybrid search(d[3], iv[4]);
            const auto fs = open3d::ComputeFPFHFeature(source, search);
            const auto ft = open3d::ComputeFPFHFeature(target, search);
            const RegistrationResult r = cicp::FastGlobalRegistration(source, target, *fs, *ft, option, (uint64_t)seed);
            if (write_T(o, r.transformation_)) return 4;
            for (int64_t i = 0; i < ns; i++)
                for (int j = 0; j < 33; j++) {
                    const double v = fs->data_(j, i);
                    if (fwrite(&v, 8, 1, o) != 1) return 4;
                }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::fclose(o);
    return 0;
}
