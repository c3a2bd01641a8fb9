// axis_driver.cpp -- the estimators constrained to a rotation about one axis
// (cicp::TransformationEstimationPointToPointYaw / PointToPlaneYaw) and the
// upright option of RegisterModelToScene, called the way a VISMA caller would.
// Usage: axis_driver <mode> <in.bin> <out.bin>
//   in : int64 ns, int64 nt, double radius, int32 iters, int32 level, double init[16], double up[3],
//        ns*3 doubles, nt*3 doubles, [nt*3 target normals for the *_plane modes]
//   out: double T[16], fitness, rmse, K, extra
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "constrained_ICP.h"
#include "visma_geometry.hpp"

using namespace open3d;

// a user plugin that delegates to the constrained estimator: RegistrationICP does not recognise it, so the
// generic loop (GPU passes + this class's host solve) runs it
class MyYaw : public TransformationEstimation {
public:
    explicit MyYaw(const Eigen::Vector3d &up) : inner(up) {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::PointToPoint;
    }
    double ComputeRMSE(const PointCloud &s, const PointCloud &t, const CorrespondenceSet &c) const override
    {
        return inner.ComputeRMSE(s, t, c);
    }
    Eigen::Matrix4d ComputeTransformation(const PointCloud &s, const PointCloud &t,
                                          const CorrespondenceSet &c) const override
    {
        return inner.ComputeTransformation(s, t, c);
    }
    cicp::TransformationEstimationPointToPointYaw inner;
};

static void read_cloud(FILE *f, std::vector<Eigen::Vector3d> &v, int64_t n)
{
    v.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        double p[3];
        if (fread(p, 8, 3, f) != 3) std::exit(2);
        v[(size_t)i] = Eigen::Vector3d(p[0], p[1], p[2]);
    }
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::string mode = argv[1];
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    int64_t ns, nt; double radius; int32_t iters, level; double init_rm[16], up3[3];
    if (fread(&ns, 8, 1, f) != 1 || fread(&nt, 8, 1, f) != 1 || fread(&radius, 8, 1, f) != 1 ||
        fread(&iters, 4, 1, f) != 1 || fread(&level, 4, 1, f) != 1 || fread(init_rm, 8, 16, f) != 16 ||
        fread(up3, 8, 3, f) != 3)
        return 2;
    auto model = std::make_shared<PointCloud>();
    auto scene = std::make_shared<PointCloud>();
    read_cloud(f, model->points_, ns);
    read_cloud(f, scene->points_, nt);
    const bool plane = mode.size() > 6 && mode.compare(mode.size() - 6, 6, "_plane") == 0;
    if (plane) read_cloud(f, scene->normals_, nt);
    std::fclose(f);
    Eigen::Matrix4d init;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) init(i, j) = init_rm[i * 4 + j];
    const Eigen::Vector3d up(up3[0], up3[1], up3[2]);
    const ICPConvergenceCriteria crit(0.0, 0.0, iters);

    RegistrationResult result;
    double extra = 0.0;
    try {
        if (mode == "solve" || mode == "solve_plane") {            // explicit correspondences i <-> i, host only
            CorrespondenceSet c((size_t)ns);
            for (int64_t i = 0; i < ns; i++) c[(size_t)i] = Eigen::Vector2i((int)i, (int)i);
            if (plane) {
                cicp::TransformationEstimationPointToPlaneYaw e(up);
                result.transformation_ = e.ComputeTransformation(*model, *scene, c);
                result.inlier_rmse_ = e.ComputeRMSE(*model, *scene, c);
            } else {
                cicp::TransformationEstimationPointToPointYaw e(up);
                result.transformation_ = e.ComputeTransformation(*model, *scene, c);
                result.inlier_rmse_ = e.ComputeRMSE(*model, *scene, c);
            }
        } else if (mode == "icp_yaw") {
            result = open3d::RegistrationICP(*model, *scene, radius, init, cicp::TransformationEstimationPointToPointYaw(up), crit);
        } else if (mode == "icp_yaw_plane") {
            result = open3d::RegistrationICP(*model, *scene, radius, init, cicp::TransformationEstimationPointToPlaneYaw(up), crit);
        } else if (mode == "plugin") {
            result = open3d::RegistrationICP(*model, *scene, radius, init, MyYaw(up), crit);
        } else if (mode == "stock_around") {
            // a stock call, a constrained one, the stock call again: the third must equal the first bit for bit
            const RegistrationResult a = open3d::RegistrationICP(*model, *scene, radius, init,
                                                                 cicp::TransformationEstimationPointToPoint4DoF(), crit);
            (void)open3d::RegistrationICP(*model, *scene, radius, init, cicp::TransformationEstimationPointToPointYaw(up), crit);
            result = open3d::RegistrationICP(*model, *scene, radius, init, cicp::TransformationEstimationPointToPoint4DoF(), crit);
            extra = (result.transformation_ - a.transformation_).cwiseAbs().maxCoeff();
            if (result.correspondence_set_.size() != a.correspondence_set_.size()) extra = 1.0;
        } else if (mode == "upright" || mode == "free") {
            result.transformation_ = cicp::RegisterModelToScene(*model, *scene, level, radius, false, &result, mode == "upright");
        } else {
            return 2;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    double out[20];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) out[i * 4 + j] = result.transformation_(i, j);
    out[16] = result.fitness_;
    out[17] = result.inlier_rmse_;
    out[18] = (double)result.correspondence_set_.size();
    out[19] = extra;
    fwrite(out, 8, 20, o);
    std::fclose(o);
    return 0;
}
