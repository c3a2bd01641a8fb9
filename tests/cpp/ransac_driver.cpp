// ransac_driver.cpp -- RANSAC global registration called the way an Open3D caller does, against the stand-alone header set.
// Usage: ransac_driver errors|run <in.bin> <out.bin>
//   in : int64 ns, int64 nt, int64 K, int64 dim, double max_correspondence_distance, double edge similarity, double distance
//        threshold, double normal angle (a checker <= 0 is left out), int32 ransac_n, int32 max_iteration, int32
//        max_validation, int64 seed, ns*3 doubles (source), ns*3 (source normals), nt*3 (target), nt*3 (target normals),
//        ns*dim doubles (source features, point-major), nt*dim (target features), K * 2 int32 correspondences
//   errors (no GPU): the early returns and the reports of what the GPU cannot run -- each must give RegistrationResult()
//        before a context exists; exit status 5 where one does not (6, 7, 8: a checker's own Check on the host)
//   run  (GPU): cicp::RegistrationRANSACBasedOnFeatureMatching(..., seed) and cicp::RegistrationRANSACBasedOnCorrespondence(...,
//        seed); out: 16 doubles T, fitness, rmse, correspondence_set_.size(), then 16 doubles T, fitness, rmse
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

static void read_feature(FILE *f, Feature &feat, int64_t n, int64_t dim)
{
    feat.Resize((int)dim, (int)n);
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = 0; j < dim; j++) {
            double v;
            if (fread(&v, 8, 1, f) != 1) std::exit(2);
            feat.data_(j, i) = v;
        }
}

static int write_result(FILE *o, const RegistrationResult &r, bool with_count)
{
    double v[19];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) v[i * 4 + j] = r.transformation_(i, j);
    v[16] = r.fitness_; v[17] = r.inlier_rmse_; v[18] = (double)r.correspondence_set_.size();
    const size_t n = with_count ? 19 : 18;
    return fwrite(v, 8, n, o) == n ? 0 : 4;
}

static bool is_empty(const RegistrationResult &r)
{
    return r.transformation_ == Eigen::Matrix4d::Identity() && r.fitness_ == 0.0 && r.inlier_rmse_ == 0.0 && r.correspondence_set_.empty();
}

// a checker of the caller's own: the GPU cannot call it
class AlwaysTrue : public CorrespondenceChecker {
public:
    AlwaysTrue() : CorrespondenceChecker(false) {}
    bool Check(const PointCloud &, const PointCloud &, const CorrespondenceSet &, const Eigen::Matrix4d &) const override { return true; }
};

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const bool errors = std::strcmp(argv[1], "errors") == 0;
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    int64_t hd[4], seed;
    double d[4];
    int32_t iv[3];
    if (fread(hd, 8, 4, f) != 4 || fread(d, 8, 4, f) != 4 || fread(iv, 4, 3, f) != 3 || fread(&seed, 8, 1, f) != 1) return 2;
    const int64_t ns = hd[0], nt = hd[1], K = hd[2], dim = hd[3];
    PointCloud source, target;
    read_cloud(f, source.points_, ns);
    read_cloud(f, source.normals_, ns);
    read_cloud(f, target.points_, nt);
    read_cloud(f, target.normals_, nt);
    Feature fs, ft;
    read_feature(f, fs, ns, dim);
    read_feature(f, ft, nt, dim);
    CorrespondenceSet corres((size_t)K);
    for (int64_t i = 0; i < K; i++) {
        int32_t p[2];
        if (fread(p, 4, 2, f) != 2) return 2;
        corres[(size_t)i] = Eigen::Vector2i(p[0], p[1]);
    }
    std::fclose(f);
    const CorrespondenceCheckerBasedOnEdgeLength ce(d[1]);
    const CorrespondenceCheckerBasedOnDistance cd(d[2]);
    const CorrespondenceCheckerBasedOnNormal cn(d[3]);
    std::vector<std::reference_wrapper<const CorrespondenceChecker>> checkers;
    if (d[1] > 0.0) checkers.push_back(ce);
    if (d[2] > 0.0) checkers.push_back(cd);
    if (d[3] > 0.0) checkers.push_back(cn);
    const RANSACConvergenceCriteria criteria(iv[1], iv[2]);
    const TransformationEstimationPointToPoint p2p(false);
    FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    try {
        if (errors) {
            const AlwaysTrue own;
            std::vector<std::reference_wrapper<const CorrespondenceChecker>> with_own = checkers, twice = checkers;
            with_own.push_back(own);
            twice.push_back(ce); twice.push_back(ce);
            const CorrespondenceSet few(corres.begin(), corres.begin() + 3);
            Feature short_feature;
            short_feature.Resize((int)dim, (int)ns - 1);
            const CorrespondenceCheckerBasedOnDistance zero_distance(0.0), negative_distance(-1.0);
            const CorrespondenceCheckerBasedOnNormal zero_angle(0.0);
            const CorrespondenceCheckerBasedOnEdgeLength edge_off(0.0);
            std::vector<std::reference_wrapper<const CorrespondenceChecker>> d0, dneg, a0, e2;
            d0.push_back(zero_distance); dneg.push_back(negative_distance); a0.push_back(zero_angle);
            e2.push_back(edge_off); e2.push_back(ce);           // two of one class, the first with a threshold that is "off"
            const RegistrationResult r[] = {
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, 2, checkers, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, 9, checkers, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, 0.0, p2p, 4, checkers, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], TransformationEstimationPointToPlane(), 4, checkers, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], TransformationEstimationPointToPoint(true), 4, checkers, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, 4, with_own, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, 4, twice, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, 4, d0, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, 4, dneg, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, 4, a0, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, 4, e2, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(source, target, short_feature, ft, d[0], p2p, 4, checkers, criteria),
                open3d::RegistrationRANSACBasedOnFeatureMatching(PointCloud(), target, Feature(), ft, d[0], p2p, 4, checkers, criteria),
                open3d::RegistrationRANSACBasedOnCorrespondence(source, target, corres, d[0], p2p, 2, criteria),
                open3d::RegistrationRANSACBasedOnCorrespondence(source, target, corres, d[0], p2p, 9, criteria),
                open3d::RegistrationRANSACBasedOnCorrespondence(source, target, few, d[0], p2p, 6, criteria),
                open3d::RegistrationRANSACBasedOnCorrespondence(source, target, corres, -1.0, p2p, 6, criteria),
                open3d::RegistrationRANSACBasedOnCorrespondence(source, target, corres, d[0], TransformationEstimationPointToPlane(), 6, criteria),
                cicp::RegistrationRANSACBasedOnCorrespondence(source, target, corres, d[0], TransformationEstimationPointToPoint(true), 6, criteria, 7),
            };
            for (const RegistrationResult &x : r)
                if (!is_empty(x)) return 5;
            // the checkers' own Check on the host: an edge of one cloud against itself passes, against a stretched copy fails
            PointCloud stretched = source;
            for (auto &p : stretched.points_) p *= 2.0;
            const CorrespondenceSet same = {Eigen::Vector2i(0, 0), Eigen::Vector2i(5, 5), Eigen::Vector2i(9, 9)};
            if (!ce.Check(source, source, same, Eigen::Matrix4d::Identity()) || ce.Check(source, stretched, same, Eigen::Matrix4d::Identity()))
                return 6;
            if (!CorrespondenceCheckerBasedOnDistance(1e-9).Check(source, source, {Eigen::Vector2i(0, 0)}, Eigen::Matrix4d::Identity()) ||
                CorrespondenceCheckerBasedOnDistance(1e-9).Check(source, stretched, {Eigen::Vector2i(1, 1)}, Eigen::Matrix4d::Identity()))
                return 7;
            if (ce.require_pointcloud_alignment_ || !cd.require_pointcloud_alignment_ || !cn.require_pointcloud_alignment_) return 8;
        } else {
            const RegistrationResult a = cicp::RegistrationRANSACBasedOnFeatureMatching(source, target, fs, ft, d[0], p2p, iv[0], checkers,
                                                                                       criteria, (uint64_t)seed);
            if (write_result(o, a, true)) return 4;
            const RegistrationResult b = cicp::RegistrationRANSACBasedOnCorrespondence(source, target, corres, d[0], p2p, iv[0], criteria,
                                                                                      (uint64_t)seed);
            if (write_result(o, b, false)) return 4;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::fclose(o);
    return 0;
}
