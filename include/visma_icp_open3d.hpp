// visma_icp_open3d.hpp -- header-only C++/Eigen adapter between Open3D-shaped
// callers and the C ABI (visma_icp.h).
//
// It is written against the NAMES the reference's callers use
// (open3d::PointCloud::points_/normals_, CorrespondenceSet, RegistrationResult,
// ICPConvergenceCriteria, TransformationEstimation and its enum), so it
// compiles against the real Open3D 0.3.0 headers or against the stand-alone
// set in include/Core/.  Include one of them first.
//
//   open3d::cicp::RegistrationICP      same signature as open3d::RegistrationICP
//                                      (O3D/Core/Registration/Registration.h:102-107)
//   open3d::cicp::EvaluateRegistration (Registration.h:96-99)
//   open3d::cicp::RegisterModelToScene feh::RegisterModelToScene
//                                      (include/tool.h:40-42, src/annotation.cpp:29-64)
//                                      (keep < 1: trimmed ICP from every start)
//   open3d::cicp::TransformationEstimationPointToPointTrimmed(keep)
//                                      trimmed ICP through RegistrationICP: only the keep * |source| closest pairs
//                                      of every iteration enter the solve (a model against a partial scan)
//   open3d::cicp::TransformationEstimationPointToPointRobust(kernel) / ...PointToPlaneRobust(kernel)
//                                      robust ICP through RegistrationICP: every pair weighted by a function of its
//                                      own residual (cicp::RobustKernel: Huber, Tukey, Cauchy; the scale from the
//                                      median residual unless given) -- no overlap share needed
//   open3d::cicp::TransformationEstimationGeneralized(epsilon)
//                                      generalized ICP (plane-to-plane) through RegistrationICP: every pair weighted
//                                      by the inverse of the sum of both points' surface covariances; needs the
//                                      normals of BOTH clouds (a sampled CAD model has exact ones)
//   open3d::cicp::TransformationEstimationForColoredICP(lambda_geometric) / cicp::RegistrationColoredICP
//                                      colored ICP (O3D/Core/Registration/ColoredICP.h): a photometric row next to
//                                      the point-to-plane row of every pair; needs the target's normals and the
//                                      colours of BOTH clouds -- for textured surfaces whose geometry leaves a motion free
//   open3d::cicp::ComputeFPFHFeature / cicp::FastGlobalRegistration
//                                      registration WITHOUT an initial pose (O3D/Core/Registration/Feature.h,
//                                      FastGlobalRegistration.h): FPFH of both clouds, matched, tuple-tested and
//                                      optimised; its result is the `init` of any RegistrationICP above
//   open3d::cicp::GetInformationMatrixFromPointClouds / cicp::GlobalOptimization
//                                      multiway registration (O3D/Core/Registration/Registration.h:132-135,
//                                      GlobalOptimization.h): the information matrix of an edge on the GPU -- one call
//                                      for every edge of a PoseGraph --, then the line-process pose-graph optimisation
//                                      on the host.  WITHOUT the identity terms Open3D 0.3.0 adds to the matrix
//   open3d::cicp::ComputeRGBDOdometry  the odometry edge between two consecutive RGB-D frames and its information matrix
//   open3d::cicp::CreatePointCloudFromDepthImage / FromRGBDImage   the points behind a frame; and, with the stand-alone
//                                      header set, open3d::UniformTSDFVolume: frames with poses fused into a volume on the GPU
//                                      (O3D/Core/Odometry/Odometry.h): image pyramids, per-pixel pairs and the colour or
//                                      hybrid Gauss-Newton rows on the GPU
//   open3d::cicp::ColorMapOptimization camera poses refined against the vertices' intensities and the vertices re-coloured
//                                      (O3D/Core/ColorMap/ColorMapOptimization.h, rigid variant), on a TriangleMesh or a
//                                      PointCloud; with the stand-alone header set
//   open3d::cicp::ICPRefinement        the ICP call of feh::ICPRefinement
//                                      (src/evaluation.cpp:258-271)
//   open3d::cicp::ComputePointCloudToPointCloudDistance / ComputePointCloudNearestNeighborDistance
//                                      (O3D/Core/Geometry/PointCloud.h:161-183)
//
// No Eigen type crosses a binary boundary: the C ABI takes raw row-major
// doubles, so a translation unit built with -DEIGEN_DEFAULT_TO_ROW_MAJOR (as
// VISMA's CMakeLists.txt:11-12 does) and one built without it can both use
// this header.  Infrastructure failures (no GPU, HIP error) throw
// std::runtime_error; argument errors follow the reference (message on stderr,
// RegistrationResult(init) returned, Registration.cpp:148-157).
#pragma once

#include <Eigen/Core>
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <typeinfo>
#include <vector>

#include <Core/Registration/Feature.h>
#include <Core/Registration/FastGlobalRegistration.h>
#include <Core/Registration/CorrespondenceChecker.h>
#include <Core/Registration/PoseGraph.h>
#include <Core/Registration/GlobalOptimizationConvergenceCriteria.h>
#include <Core/Registration/GlobalOptimizationMethod.h>
#include <Core/Geometry/Image.h>
#include <Core/Geometry/RGBDImage.h>
#include <Core/Geometry/TriangleMesh.h>
#include <Core/Odometry/Odometry.h>
#ifdef VISMA_ICP_STANDALONE_OPEN3D_TYPES
#include <Core/Integration/UniformTSDFVolume.h>
#include <Core/Integration/ScalableTSDFVolume.h>
#include <Core/ColorMap/ColorMapOptimization.h>
#include <Core/Geometry/KDTreeFlann.h>
#endif

#include "visma_icp.h"
#include "visma_io.h"

namespace open3d {
namespace cicp {

// The plugin of include/constrained_ICP.h:14-30, made concrete: the reference
// class never overrides the pure virtual GetTransformationEstimationType()
// (O3D/Core/Registration/TransformationEstimation.h:58-59) and so cannot be
// instantiated against the vendored Open3D; this one can.
class TransformationEstimationPointToPoint4DoF : public TransformationEstimation {
public:
    TransformationEstimationPointToPoint4DoF(bool with_scaling = false)
        : with_scaling_(with_scaling) {}
    ~TransformationEstimationPointToPoint4DoF() override {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::PointToPoint;
    }
    inline double ComputeRMSE(const PointCloud &source, const PointCloud &target,
                              const CorrespondenceSet &corres) const override;
    inline Eigen::Matrix4d ComputeTransformation(const PointCloud &source,
                                                 const PointCloud &target,
                                                 const CorrespondenceSet &corres) const override;
    bool with_scaling_ = false;
};

// Orientation constrained ICP (the VISMA paper's estimator): the rotation turns about `up_` only (+Y: the frame of a
// scan whose floor normal has been turned onto +Y), the translation is free.  cicp::RegistrationICP runs both fully on
// the GPU (the thread context's visma_icp_set_rotation_axis, for that call only); ComputeTransformation solves the same
// 4-DoF update on the host (visma_icp_solve_from_stats_axis), so the generic plugin loop gets it too.
class TransformationEstimationPointToPointYaw : public TransformationEstimation {
public:
    TransformationEstimationPointToPointYaw(const Eigen::Vector3d &up = Eigen::Vector3d::UnitY()) : up_(up) {}
    ~TransformationEstimationPointToPointYaw() override {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::PointToPoint;
    }
    inline double ComputeRMSE(const PointCloud &source, const PointCloud &target,
                              const CorrespondenceSet &corres) const override;
    inline Eigen::Matrix4d ComputeTransformation(const PointCloud &source,
                                                 const PointCloud &target,
                                                 const CorrespondenceSet &corres) const override;
    Eigen::Vector3d up_;
};

class TransformationEstimationPointToPlaneYaw : public TransformationEstimation {
public:
    TransformationEstimationPointToPlaneYaw(const Eigen::Vector3d &up = Eigen::Vector3d::UnitY()) : up_(up) {}
    ~TransformationEstimationPointToPlaneYaw() override {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::PointToPlane;
    }
    inline double ComputeRMSE(const PointCloud &source, const PointCloud &target,
                              const CorrespondenceSet &corres) const override;
    inline Eigen::Matrix4d ComputeTransformation(const PointCloud &source,
                                                 const PointCloud &target,
                                                 const CorrespondenceSet &corres) const override;
    Eigen::Vector3d up_;
};

// Trimmed ICP (Chetverikov et al., ICPR 2002): per iteration only the floor(keep * |source|) pairs with the smallest
// distance enter the closed-form solve (visma_icp_run_trimmed; visma_icp.h states the rule).  keep = the share of the
// SOURCE the target can see; with it a radius several times the usual one becomes usable on a partial scan; a keep
// below the true overlap stalls.  What cicp::RegistrationICP returns for it:
//   correspondence_set_  the KEPT pairs of the last pass, sorted by source index (what a later solve should get)
//   fitness_             K / |source| over ALL pairs inside the radius (callers pick yaw winners by it)
//   inlier_rmse_         the TRIMMED rmse: over the kept pairs (the objective the loop minimises)
// ComputeTransformation(source, target, corres) solves over the corres it is given, like the other estimators.
class TransformationEstimationPointToPointTrimmed : public TransformationEstimation {
public:
    explicit TransformationEstimationPointToPointTrimmed(double keep = 1.0) : keep_(keep) {}
    ~TransformationEstimationPointToPointTrimmed() override {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::PointToPoint;
    }
    inline double ComputeRMSE(const PointCloud &source, const PointCloud &target,
                              const CorrespondenceSet &corres) const override;
    inline Eigen::Matrix4d ComputeTransformation(const PointCloud &source,
                                                 const PointCloud &target,
                                                 const CorrespondenceSet &corres) const override;
    double keep_ = 1.0;
};

// Robust ICP (visma_icp_run_robust; visma_icp.h states weights and scale): an M-estimator in place of the least-squares
// objective -- every pair of an iteration is weighted by a function of its own residual.  What later Open3D versions
// call RobustKernel.  scale = 0: the scale comes from the median residual of every pass (tune = 0: the family's
// 95 %-efficiency constant), so nothing about the overlap has to be known.
struct RobustKernel {
    enum Type { L2 = VISMA_ICP_ROBUST_L2, Huber = VISMA_ICP_ROBUST_HUBER, Tukey = VISMA_ICP_ROBUST_TUKEY, Cauchy = VISMA_ICP_ROBUST_CAUCHY };
    RobustKernel(Type type_ = Tukey, double scale_ = 0.0, double tune_ = 0.0, double min_scale_ = 0.0)
        : type(type_), scale(scale_), tune(tune_), min_scale(min_scale_) {}
    Type type;
    double scale = 0, tune = 0, min_scale = 0;
    visma_icp_robust c_config() const
    {
        visma_icp_robust c;
        c.kernel = (int)type; c.scale = scale; c.tune = tune; c.min_scale = min_scale;
        return c;
    }
};

// What cicp::RegistrationICP returns for the two robust estimators:
//   correspondence_set_  all K pairs of the last pass (their weights: visma_icp_get_pair_weights on the thread context)
//   fitness_             K / |source|, unweighted
//   inlier_rmse_         the ROBUST rmse sqrt(sum w |p - q|^2 / sum w) (what the loop's stop test looks at)
// ComputeTransformation(source, target, corres) solves unweighted over the corres it is given, like the other estimators.
class TransformationEstimationPointToPointRobust : public TransformationEstimation {
public:
    explicit TransformationEstimationPointToPointRobust(const RobustKernel &kernel = RobustKernel(), bool with_scaling = false)
        : kernel_(kernel), with_scaling_(with_scaling) {}
    ~TransformationEstimationPointToPointRobust() override {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::PointToPoint;
    }
    inline double ComputeRMSE(const PointCloud &source, const PointCloud &target,
                              const CorrespondenceSet &corres) const override;
    inline Eigen::Matrix4d ComputeTransformation(const PointCloud &source,
                                                 const PointCloud &target,
                                                 const CorrespondenceSet &corres) const override;
    RobustKernel kernel_;
    bool with_scaling_ = false;
};

class TransformationEstimationPointToPlaneRobust : public TransformationEstimation {
public:
    explicit TransformationEstimationPointToPlaneRobust(const RobustKernel &kernel = RobustKernel()) : kernel_(kernel) {}
    ~TransformationEstimationPointToPlaneRobust() override {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::PointToPlane;
    }
    inline double ComputeRMSE(const PointCloud &source, const PointCloud &target,
                              const CorrespondenceSet &corres) const override;
    inline Eigen::Matrix4d ComputeTransformation(const PointCloud &source,
                                                 const PointCloud &target,
                                                 const CorrespondenceSet &corres) const override;
    RobustKernel kernel_;
};

// Generalized ICP (Segal, Haehnel, Thrun, RSS 2009; visma_icp_run_gicp -- visma_icp.h states the step): the covariance of
// a point is that of a surface element with its normal, C = I - (1 - epsilon) n n^T, and every pair is weighted by
// (C_target + R C_source R^T)^-1.  What later Open3D versions call TransformationEstimationForGeneralizedICP, without
// covariance arrays.  Normals are used as given: unit length is the caller's business.  What cicp::RegistrationICP
// returns for it:
//   correspondence_set_  all K pairs of the last pass
//   fitness_, inlier_rmse_  K / |source| and the plain rmse over the K pairs (the loop's stop test looks at the
//                        Mahalanobis rmse sqrt(sum d^T M d / K): visma_icp_gicp_info)
// ComputeRMSE(source, target, corres) is that Mahalanobis rmse and ComputeTransformation the generalized step over the
// corres they are given, restated on the host; source.normals_ are taken as lying in the frame of source.points_.
class TransformationEstimationGeneralized : public TransformationEstimation {
public:
    explicit TransformationEstimationGeneralized(double epsilon = 1e-3) : epsilon_(epsilon) {}
    ~TransformationEstimationGeneralized() override {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::PointToPlane;
    }
    inline double ComputeRMSE(const PointCloud &source, const PointCloud &target,
                              const CorrespondenceSet &corres) const override;
    inline Eigen::Matrix4d ComputeTransformation(const PointCloud &source,
                                                 const PointCloud &target,
                                                 const CorrespondenceSet &corres) const override;
    double epsilon_ = 1e-3;
};

// Colored ICP (Park, Zhou, Koltun, ICCV 2017; O3D/Core/Registration/ColoredICP.cpp; visma_icp.h states the step).
// lambda_geometric outside [0, 1] becomes 0.968, as the reference's constructor does.  What cicp::RegistrationICP returns
// for it: all K pairs of the last pass, K / |source| and the plain rmse over them (what the loop's stop test compares).
// The library computes the target's colour gradient itself (Hybrid search: 2 x the correspondence distance, 30).
// ComputeRMSE(source, target, corres) is the reference's value -- the SUM r_g^2 + r_c^2, no root, no mean
// (ColoredICP.cpp:203-232) -- and ComputeTransformation the colored step over the corres they are given, restated on the
// host.  Both need the target's gradient in color_gradient_ (one per target point: cicp::ComputeColorGradient); without
// one of that size they return 0 and the identity.
class TransformationEstimationForColoredICP : public TransformationEstimation {
public:
    explicit TransformationEstimationForColoredICP(double lambda_geometric = 0.968) : lambda_geometric_(lambda_geometric)
    {
        if (!(lambda_geometric_ >= 0.0 && lambda_geometric_ <= 1.0)) lambda_geometric_ = 0.968;
    }
    ~TransformationEstimationForColoredICP() override {}
    TransformationEstimationType GetTransformationEstimationType() const override
    {
        return TransformationEstimationType::ColoredICP;
    }
    inline double ComputeRMSE(const PointCloud &source, const PointCloud &target,
                              const CorrespondenceSet &corres) const override;
    inline Eigen::Matrix4d ComputeTransformation(const PointCloud &source,
                                                 const PointCloud &target,
                                                 const CorrespondenceSet &corres) const override;
    double lambda_geometric_ = 0.968;
    std::vector<Eigen::Vector3d> color_gradient_;      // of the target, for the host restatements only
};

namespace detail {

inline void to_rowmajor(const Eigen::Matrix4d &M, double T[16])
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) T[i * 4 + j] = M(i, j);
}

inline Eigen::Matrix4d from_rowmajor(const double T[16])
{
    Eigen::Matrix4d M;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) M(i, j) = T[i * 4 + j];
    return M;
}

// One context per host thread (the ABI is thread-compatible, not thread-safe).
class ThreadContext {
public:
    ~ThreadContext() { if (ctx_) visma_icp_destroy(ctx_); }
    visma_icp_ctx *get()
    {
        if (!ctx_) {
            int device = 0;
            if (const char *e = std::getenv("VISMA_ICP_DEVICE")) device = std::atoi(e);
            const int rc = visma_icp_create(&ctx_, device);
            if (rc != VISMA_ICP_OK)
                throw std::runtime_error(std::string("visma_icp_create failed: ") +
                                         visma_icp_last_error(nullptr));
            // drop-in callers want the reference's correspondences: f64 search for the cloud
            // sizes where one flipped near-tie would show (VISMA_ICP_SEARCH_PRECISION=0/1/2 overrides)
            int prec = 1;
            if (const char *e = std::getenv("VISMA_ICP_SEARCH_PRECISION")) prec = std::atoi(e);
            visma_icp_set_search_precision(ctx_, prec);
        }
        return ctx_;
    }
    static ThreadContext &instance()
    {
        static thread_local ThreadContext tc;
        return tc;
    }

private:
    visma_icp_ctx *ctx_ = nullptr;
};

inline void check(visma_icp_ctx *ctx, int rc, const char *what)
{
    if (rc != VISMA_ICP_OK)
        throw std::runtime_error(std::string(what) + ": " + visma_icp_last_error(ctx));
}

// std::vector<Eigen::Vector3d> is contiguous AoS f64 with stride 3
inline const double *xyz(const std::vector<Eigen::Vector3d> &v)
{
    return v.empty() ? nullptr : v[0].data();
}

// `radius`: the max_correspondence_distance of the registration that follows (> 0: the library builds its search
// structure on the GPU while it is still staging the source, visma_icp_set_radius_hint)
template <typename Cloud>
inline visma_icp_ctx *upload(const Cloud &source, const Cloud &target, bool normals, double radius = 0.0)
{
    visma_icp_ctx *ctx = ThreadContext::instance().get();
    if (radius > 0.0) check(ctx, visma_icp_set_radius_hint(ctx, radius), "visma_icp_set_radius_hint");
    check(ctx, visma_icp_set_clouds_f64(ctx, xyz(source.points_), (int64_t)source.points_.size(), 3,
                                        xyz(target.points_), (int64_t)target.points_.size(), 3),
          "visma_icp_set_clouds_f64");
    if (normals)
        check(ctx, visma_icp_set_target_normals_f64(ctx, xyz(target.normals_),
                                                    (int64_t)target.normals_.size(), 3),
              "visma_icp_set_target_normals_f64");
    return ctx;
}

template <typename Result>
inline void fill_result(visma_icp_ctx *ctx, const visma_icp_result &r, size_t ns, Result &out)
{
    out.transformation_ = from_rowmajor(r.transformation);
    out.fitness_ = r.fitness;
    out.inlier_rmse_ = r.inlier_rmse;
    std::vector<int32_t> si(ns ? ns : 1), ti(ns ? ns : 1);
    int64_t k = 0;
    check(ctx, visma_icp_get_correspondences(ctx, si.data(), ti.data(), nullptr, &k),
          "visma_icp_get_correspondences");
    out.correspondence_set_.resize((size_t)k);
    for (int64_t i = 0; i < k; i++) out.correspondence_set_[i] = Eigen::Vector2i(si[i], ti[i]);
}

// ... of a trimmed run: the KEPT pairs (sorted by source index), fitness over all K, the trimmed rmse
template <typename Result>
inline void fill_result_trimmed(visma_icp_ctx *ctx, const visma_icp_result &r, const visma_icp_trim_info &info, size_t ns,
                                Result &out)
{
    out.transformation_ = from_rowmajor(r.transformation);
    out.fitness_ = r.fitness;
    out.inlier_rmse_ = info.trimmed_rmse;
    out.correspondence_set_.clear();
    if (r.num_correspondences <= 0) return;
    std::vector<int32_t> si(ns ? ns : 1), ti(ns ? ns : 1);
    std::vector<uint8_t> kept(ns ? ns : 1);
    int64_t k = 0;
    check(ctx, visma_icp_get_correspondences(ctx, si.data(), ti.data(), nullptr, &k),
          "visma_icp_get_correspondences");
    check(ctx, visma_icp_get_kept_mask(ctx, kept.data()), "visma_icp_get_kept_mask");
    out.correspondence_set_.reserve((size_t)info.kept);
    for (int64_t i = 0; i < k; i++)
        if (kept[(size_t)si[i]]) out.correspondence_set_.push_back(Eigen::Vector2i(si[i], ti[i]));
}

// 38 statistics of explicit correspondences, accumulated on the host in f64
// (same layout the reduction kernel produces; see visma_icp.h).
template <typename Cloud, typename Corr>
inline void host_stats(const Cloud &source, const Cloud &target, const Corr &corres, bool plane,
                       double st[VISMA_ICP_NSTATS])
{
    double JTJ[6][6] = {{0}}, JTr[6] = {0}, M[3][3] = {{0}}, r2 = 0.0;
    for (const auto &c : corres) {
        const Eigen::Vector3d &p = source.points_[c[0]];
        const Eigen::Vector3d &q = target.points_[c[1]];
        const int rows = plane ? 1 : 3;
        for (int k = 0; k < rows; k++) {
            Eigen::Vector3d n = plane ? Eigen::Vector3d(target.normals_[c[1]]) : Eigen::Vector3d::Zero();
            if (!plane) n[k] = 1.0;
            const Eigen::Vector3d a(p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2],
                                    p[0] * n[1] - p[1] * n[0]);  // p x n
            const double J[6] = {a[0], a[1], a[2], n[0], n[1], n[2]};
            const double r = (p - q).dot(n);
            for (int i = 0; i < 6; i++) {
                for (int j = 0; j < 6; j++) JTJ[i][j] += J[i] * J[j];
                JTr[i] += J[i] * r;
            }
            r2 += r * r;
        }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) M[i][j] += q[i] * p[j];
    }
    int o = 0;
    st[o++] = (double)corres.size();
    st[o++] = r2;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) st[o++] = JTJ[i][j];
    for (int i = 0; i < 6; i++) st[o++] = JTr[i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) st[o++] = M[i][j];
}

template <typename Cloud, typename Corr>
inline Eigen::Matrix4d host_update(const Cloud &s, const Cloud &t, const Corr &corres, bool plane,
                                   bool with_scaling)
{
    if (corres.empty()) return Eigen::Matrix4d::Identity();
    double st[VISMA_ICP_NSTATS], T[16];
    host_stats(s, t, corres, plane, st);
    visma_icp_solve_from_stats(st, plane ? VISMA_ICP_SOLVER_GN_EULER : VISMA_ICP_SOLVER_KABSCH,
                               with_scaling ? 1 : 0, T);
    return from_rowmajor(T);
}

// the 4-DoF update (rotation about `up` + translation) of explicit correspondences
template <typename Cloud, typename Corr>
inline Eigen::Matrix4d host_update_axis(const Cloud &s, const Cloud &t, const Corr &corres, bool plane,
                                        const Eigen::Vector3d &up)
{
    if (corres.empty() || (plane && !t.HasNormals())) return Eigen::Matrix4d::Identity();
    double st[VISMA_ICP_NSTATS], T[16];
    const double a[3] = {up[0], up[1], up[2]};
    host_stats(s, t, corres, plane, st);
    if (visma_icp_solve_from_stats_axis(st, plane ? 1 : 0, a, T) != VISMA_ICP_OK)
        throw std::invalid_argument("rotation axis is zero, near zero or not finite");
    return from_rowmajor(T);
}

// The generalized statistics of explicit correspondences (visma_icp.h: generalized ICP) on the host; source normals as
// they are (already in the frame of the source points).  Returns sum d^T M d.
template <typename Cloud, typename Corr>
inline double host_stats_gicp(const Cloud &source, const Cloud &target, const Corr &corres, double epsilon,
                              double st[VISMA_ICP_NSTATS])
{
    double A[6][6] = {{0}}, b[6] = {0}, r2 = 0.0, cost = 0.0;
    const double k1 = 1.0 - epsilon;
    for (const auto &c : corres) {
        const Eigen::Vector3d &p = source.points_[c[0]], &q = target.points_[c[1]];
        const Eigen::Vector3d &m = source.normals_[c[0]], &n = target.normals_[c[1]];
        const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
        double C[3][3], M[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) C[i][j] = (i == j ? 2.0 : 0.0) - k1 * (n[i] * n[j] + m[i] * m[j]);
        const double a00 = C[1][1] * C[2][2] - C[1][2] * C[1][2], a01 = C[0][2] * C[1][2] - C[0][1] * C[2][2];
        const double a02 = C[0][1] * C[1][2] - C[0][2] * C[1][1], a11 = C[0][0] * C[2][2] - C[0][2] * C[0][2];
        const double a12 = C[0][1] * C[0][2] - C[0][0] * C[1][2], a22 = C[0][0] * C[1][1] - C[0][1] * C[0][1];
        const double det = C[0][0] * a00 + C[0][1] * a01 + C[0][2] * a02;
        M[0][0] = a00 / det; M[0][1] = M[1][0] = a01 / det; M[0][2] = M[2][0] = a02 / det;
        M[1][1] = a11 / det; M[1][2] = M[2][1] = a12 / det; M[2][2] = a22 / det;
        // J = [-hat(p) | I]
        const double J[3][6] = {{0.0, p[2], -p[1], 1.0, 0.0, 0.0}, {-p[2], 0.0, p[0], 0.0, 1.0, 0.0}, {p[1], -p[0], 0.0, 0.0, 0.0, 1.0}};
        double MJ[3][6], e[3];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 6; j++) MJ[i][j] = M[i][0] * J[0][j] + M[i][1] * J[1][j] + M[i][2] * J[2][j];
            e[i] = M[i][0] * d[0] + M[i][1] * d[1] + M[i][2] * d[2];
        }
        for (int i = 0; i < 6; i++) {
            for (int j = i; j < 6; j++) A[i][j] += J[0][i] * MJ[0][j] + J[1][i] * MJ[1][j] + J[2][i] * MJ[2][j];
            b[i] += J[0][i] * e[0] + J[1][i] * e[1] + J[2][i] * e[2];
        }
        r2 += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        cost += d[0] * e[0] + d[1] * e[1] + d[2] * e[2];
    }
    int o = 0;
    st[o++] = (double)corres.size();
    st[o++] = r2;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) st[o++] = A[i][j];
    for (int i = 0; i < 6; i++) st[o++] = b[i];
    while (o < VISMA_ICP_NSTATS) st[o++] = 0.0;
    return cost;
}

// The colored statistics of explicit correspondences (visma_icp.h: colored ICP) on the host; grad: the target's colour
// gradient, one per target point.  Returns sum r_g^2 + r_c^2.
template <typename Cloud, typename Corr>
inline double host_stats_colored(const Cloud &source, const Cloud &target, const Corr &corres, const std::vector<Eigen::Vector3d> &grad,
                                 double lambda, double st[VISMA_ICP_NSTATS])
{
    double A[6][6] = {{0}}, b[6] = {0}, r2 = 0.0, cost = 0.0;
    const double sg = std::sqrt(lambda), sc = std::sqrt(1.0 - lambda);
    auto add_row = [&](const Eigen::Vector3d &p, const double v[3], double s, double r) {
        const double J[6] = {s * (p[1] * v[2] - p[2] * v[1]), s * (p[2] * v[0] - p[0] * v[2]), s * (p[0] * v[1] - p[1] * v[0]),
                             s * v[0], s * v[1], s * v[2]};
        for (int i = 0; i < 6; i++) {
            for (int j = i; j < 6; j++) A[i][j] += J[i] * J[j];
            b[i] += J[i] * r;
        }
    };
    for (const auto &c : corres) {
        const Eigen::Vector3d &p = source.points_[c[0]], &q = target.points_[c[1]];
        const Eigen::Vector3d &n = target.normals_[c[1]], &g = grad[c[1]];
        const Eigen::Vector3d &cs = source.colors_[c[0]], &ct = target.colors_[c[1]];
        const double is = (cs[0] + cs[1] + cs[2]) / 3.0, it = (ct[0] + ct[1] + ct[2]) / 3.0;
        const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
        const double dn = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
        const double e[3] = {(p[0] - dn * n[0]) - q[0], (p[1] - dn * n[1]) - q[1], (p[2] - dn * n[2]) - q[2]};
        const double rg = sg * dn, rc = sc * (is - ((g[0] * e[0] + g[1] * e[1] + g[2] * e[2]) + it));
        const double gn = g[0] * n[0] + g[1] * n[1] + g[2] * n[2];
        const double h[3] = {-(g[0] - gn * n[0]), -(g[1] - gn * n[1]), -(g[2] - gn * n[2])};   // -(I - n n^T) g
        const double nn[3] = {n[0], n[1], n[2]};
        add_row(p, nn, sg, rg);
        add_row(p, h, sc, rc);
        r2 += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        cost += rg * rg + rc * rc;
    }
    int o = 0;
    st[o++] = (double)corres.size();
    st[o++] = r2;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) st[o++] = A[i][j];
    for (int i = 0; i < 6; i++) st[o++] = b[i];
    while (o < VISMA_ICP_NSTATS) st[o++] = 0.0;
    return cost;
}

// the stock point-to-plane ComputeRMSE (TransformationEstimation.cpp:64-75, with its `err = r * r`)
template <typename Cloud, typename Corr>
inline double host_rmse_point_to_plane(const Cloud &s, const Cloud &t, const Corr &c)
{
    if (c.empty() || !t.HasNormals()) return 0.0;
    const auto &l = c.back();
    const double r = (s.points_[l[0]] - t.points_[l[1]]).dot(t.normals_[l[1]]);
    return std::sqrt(r * r / (double)c.size());
}

// The thread context's rotation axis for the duration of one call: set on entry (axis != NULL), cleared on every exit
// (exceptions included) -- the next call on this thread solves unconstrained again.
class AxisScope {
public:
    AxisScope(visma_icp_ctx *ctx, const Eigen::Vector3d *axis) : ctx_(nullptr)
    {
        if (!axis) return;
        const double a[3] = {(*axis)[0], (*axis)[1], (*axis)[2]};
        check(ctx, visma_icp_set_rotation_axis(ctx, a), "visma_icp_set_rotation_axis");
        ctx_ = ctx;
    }
    ~AxisScope() { if (ctx_) (void)visma_icp_set_rotation_axis(ctx_, nullptr); }
    AxisScope(const AxisScope &) = delete;
    AxisScope &operator=(const AxisScope &) = delete;

private:
    visma_icp_ctx *ctx_;
};

template <typename Cloud, typename Corr>
inline double host_rmse_point_to_point(const Cloud &s, const Cloud &t, const Corr &corres)
{
    if (corres.empty()) return 0.0;
    double e = 0.0;
    for (const auto &c : corres) e += (s.points_[c[0]] - t.points_[c[1]]).squaredNorm();
    return std::sqrt(e / (double)corres.size());
}

}  // namespace detail

// ---------------------------------------------------------------------------
// One NN pass at a given transformation: fitness / inlier_rmse / correspondences.
inline RegistrationResult EvaluateRegistration(
    const PointCloud &source, const PointCloud &target, double max_correspondence_distance,
    const Eigen::Matrix4d &transformation = Eigen::Matrix4d::Identity())
{
    RegistrationResult result(transformation);
    if (max_correspondence_distance <= 0.0) return result;
    visma_icp_ctx *ctx = detail::upload(source, target, false, max_correspondence_distance);
    double T[16];
    detail::to_rowmajor(transformation, T);
    visma_icp_result r;
    // zero iterations of the loop == exactly one NN pass at T
    detail::check(ctx, visma_icp_run(ctx, T, max_correspondence_distance, 0, 0.0, 0.0,
                                     VISMA_ICP_SOLVER_KABSCH, 0, &r), "visma_icp_run");
    detail::fill_result(ctx, r, source.points_.size(), result);
    return result;
}

// ---------------------------------------------------------------------------
// The ICP driver.  Point-to-point estimators (Open3D's stock one and the 4DoF
// class above -- identical arithmetic) and the point-to-plane estimator run
// fully on the GPU.  Any OTHER subclass of TransformationEstimation still
// works: the NN passes run on the GPU and the plugin's own virtual
// ComputeTransformation is called on the host each iteration, exactly as
// Registration.cpp:169-184 does.
inline RegistrationResult RegistrationICP(
    const PointCloud &source, const PointCloud &target, double max_correspondence_distance,
    const Eigen::Matrix4d &init = Eigen::Matrix4d::Identity(),
    const TransformationEstimation &estimation = TransformationEstimationPointToPoint4DoF(false),
    const ICPConvergenceCriteria &criteria = ICPConvergenceCriteria())
{
    if (max_correspondence_distance <= 0.0) {
        std::fprintf(stderr, "Error: Invalid max_correspondence_distance.\n");
        return RegistrationResult(init);
    }
    const TransformationEstimationType type = estimation.GetTransformationEstimationType();
    const bool plane = type == TransformationEstimationType::PointToPlane;
    if (plane && (!source.HasNormals() || !target.HasNormals())) {
        std::fprintf(stderr, "Error: TransformationEstimationPointToPlane requires "
                             "pre-computed normal vectors.\n");
        return RegistrationResult(init);
    }
    RegistrationResult result(init);
    visma_icp_ctx *ctx = detail::upload(source, target, plane, max_correspondence_distance);
    double T[16];
    detail::to_rowmajor(init, T);
    visma_icp_result r;

    // The built-in solves replace ComputeTransformation only for EXACTLY the three stock
    // estimators.  A user class derived from one of them may override the virtual methods: it
    // takes the generic plugin loop below, which calls them like the reference does
    // (Registration.cpp:172-173).
    const std::type_info &dyn = typeid(estimation);
    const auto *four = dyn == typeid(TransformationEstimationPointToPoint4DoF)
                           ? static_cast<const TransformationEstimationPointToPoint4DoF *>(&estimation) : nullptr;
    const auto *p2p = dyn == typeid(TransformationEstimationPointToPoint)
                          ? static_cast<const TransformationEstimationPointToPoint *>(&estimation) : nullptr;
    const auto *p2l = dyn == typeid(TransformationEstimationPointToPlane)
                          ? static_cast<const TransformationEstimationPointToPlane *>(&estimation) : nullptr;
    const auto *yaw_p2p = dyn == typeid(TransformationEstimationPointToPointYaw)
                              ? static_cast<const TransformationEstimationPointToPointYaw *>(&estimation) : nullptr;
    const auto *yaw_p2l = dyn == typeid(TransformationEstimationPointToPlaneYaw)
                              ? static_cast<const TransformationEstimationPointToPlaneYaw *>(&estimation) : nullptr;
    if (yaw_p2p || yaw_p2l) {
        detail::AxisScope axis(ctx, yaw_p2p ? &yaw_p2p->up_ : &yaw_p2l->up_);
        if (yaw_p2p)
            detail::check(ctx, visma_icp_run(ctx, T, max_correspondence_distance, criteria.max_iteration_,
                                             criteria.relative_fitness_, criteria.relative_rmse_,
                                             VISMA_ICP_SOLVER_KABSCH, 0, &r),
                          "visma_icp_run");
        else
            detail::check(ctx, visma_icp_run_point_to_plane(ctx, T, max_correspondence_distance,
                                                            criteria.max_iteration_, criteria.relative_fitness_,
                                                            criteria.relative_rmse_, &r),
                          "visma_icp_run_point_to_plane");
        detail::fill_result(ctx, r, source.points_.size(), result);
        return result;
    }
    if (dyn == typeid(TransformationEstimationPointToPointTrimmed)) {
        const auto *trim = static_cast<const TransformationEstimationPointToPointTrimmed *>(&estimation);
        if (!(trim->keep_ > 0.0 && trim->keep_ <= 1.0)) {
            std::fprintf(stderr, "Error: TransformationEstimationPointToPointTrimmed requires keep in (0, 1].\n");
            return RegistrationResult(init);
        }
        visma_icp_trim_info info;
        detail::check(ctx, visma_icp_run_trimmed(ctx, T, max_correspondence_distance, trim->keep_, criteria.max_iteration_,
                                                 criteria.relative_fitness_, criteria.relative_rmse_,
                                                 VISMA_ICP_SOLVER_KABSCH, 0, &r, &info),
                      "visma_icp_run_trimmed");
        detail::fill_result_trimmed(ctx, r, info, source.points_.size(), result);
        return result;
    }
    if (dyn == typeid(TransformationEstimationPointToPointRobust) || dyn == typeid(TransformationEstimationPointToPlaneRobust)) {
        const auto *rp = plane ? nullptr : static_cast<const TransformationEstimationPointToPointRobust *>(&estimation);
        const visma_icp_robust cfg = plane ? static_cast<const TransformationEstimationPointToPlaneRobust *>(&estimation)->kernel_.c_config()
                                           : rp->kernel_.c_config();
        visma_icp_robust_info info;
        detail::check(ctx, visma_icp_run_robust(ctx, T, max_correspondence_distance, &cfg, plane ? 1 : 0, criteria.max_iteration_,
                                                criteria.relative_fitness_, criteria.relative_rmse_,
                                                rp && rp->with_scaling_ ? 1 : 0, &r, &info),
                      "visma_icp_run_robust");
        detail::fill_result(ctx, r, source.points_.size(), result);
        result.inlier_rmse_ = info.robust_rmse;
        return result;
    }
    if (dyn == typeid(TransformationEstimationGeneralized)) {
        const auto *g = static_cast<const TransformationEstimationGeneralized *>(&estimation);
        if (!(g->epsilon_ > 0.0 && g->epsilon_ <= 1.0)) {
            std::fprintf(stderr, "Error: TransformationEstimationGeneralized requires epsilon in (0, 1].\n");
            return RegistrationResult(init);
        }
        detail::check(ctx, visma_icp_set_source_normals_f64(ctx, detail::xyz(source.normals_), (int64_t)source.normals_.size(), 3),
                      "visma_icp_set_source_normals_f64");
        visma_icp_gicp_info info;
        detail::check(ctx, visma_icp_run_gicp(ctx, T, max_correspondence_distance, g->epsilon_, criteria.max_iteration_,
                                              criteria.relative_fitness_, criteria.relative_rmse_, &r, &info),
                      "visma_icp_run_gicp");
        detail::fill_result(ctx, r, source.points_.size(), result);
        return result;
    }
    if (dyn == typeid(TransformationEstimationForColoredICP)) {
        const auto *c = static_cast<const TransformationEstimationForColoredICP *>(&estimation);
        if (!target.HasNormals() || !target.HasColors() || !source.HasColors()) {
            std::fprintf(stderr, "Error: TransformationEstimationForColoredICP requires target normals and the colours of both clouds.\n");
            return RegistrationResult(init);
        }
        detail::check(ctx, visma_icp_set_target_normals_f64(ctx, detail::xyz(target.normals_), (int64_t)target.normals_.size(), 3),
                      "visma_icp_set_target_normals_f64");
        detail::check(ctx, visma_icp_set_target_colors_f64(ctx, detail::xyz(target.colors_), (int64_t)target.colors_.size(), 3),
                      "visma_icp_set_target_colors_f64");
        detail::check(ctx, visma_icp_set_source_colors_f64(ctx, detail::xyz(source.colors_), (int64_t)source.colors_.size(), 3),
                      "visma_icp_set_source_colors_f64");
        visma_icp_colored_info info;
        detail::check(ctx, visma_icp_run_colored(ctx, T, max_correspondence_distance, c->lambda_geometric_, criteria.max_iteration_,
                                                 criteria.relative_fitness_, criteria.relative_rmse_, &r, &info),
                      "visma_icp_run_colored");
        detail::fill_result(ctx, r, source.points_.size(), result);
        return result;
    }
    if (four || p2p) {
        const bool scaling = four ? four->with_scaling_ : p2p->with_scaling_;
        detail::check(ctx, visma_icp_run(ctx, T, max_correspondence_distance, criteria.max_iteration_,
                                         criteria.relative_fitness_, criteria.relative_rmse_,
                                         VISMA_ICP_SOLVER_KABSCH, scaling ? 1 : 0, &r),
                      "visma_icp_run");
        detail::fill_result(ctx, r, source.points_.size(), result);
        return result;
    }
    if (p2l) {
        detail::check(ctx, visma_icp_run_point_to_plane(ctx, T, max_correspondence_distance,
                                                        criteria.max_iteration_,
                                                        criteria.relative_fitness_,
                                                        criteria.relative_rmse_, &r),
                      "visma_icp_run_point_to_plane");
        detail::fill_result(ctx, r, source.points_.size(), result);
        return result;
    }

    // Generic plugin: GPU NN passes + the plugin's host-side solve.
    Eigen::Matrix4d transformation = init;
    PointCloud pcd = source;
    if (!init.isIdentity()) pcd.Transform(init);
    auto nn = [&](RegistrationResult &out) {
        detail::to_rowmajor(transformation, T);
        detail::check(ctx, visma_icp_run(ctx, T, max_correspondence_distance, 0, 0.0, 0.0,
                                         VISMA_ICP_SOLVER_KABSCH, 0, &r), "visma_icp_run");
        detail::fill_result(ctx, r, source.points_.size(), out);
        out.transformation_ = transformation;
    };
    nn(result);
    for (int i = 0; i < criteria.max_iteration_; i++) {
        const Eigen::Matrix4d update =
            estimation.ComputeTransformation(pcd, target, result.correspondence_set_);
        transformation = update * transformation;
        pcd.Transform(update);
        const double bf = result.fitness_, br = result.inlier_rmse_;
        nn(result);
        if (std::abs(bf - result.fitness_) < criteria.relative_fitness_ &&
            std::abs(br - result.inlier_rmse_) < criteria.relative_rmse_)
            break;
    }
    return result;
}

// open3d::RegistrationColoredICP (O3D/Core/Registration/ColoredICP.h): the colour gradient of the target by the Hybrid
// search (2 x max_distance, 30), then RegistrationICP with the colored estimator.
inline RegistrationResult RegistrationColoredICP(const PointCloud &source, const PointCloud &target, double max_distance,
                                                 const Eigen::Matrix4d &init = Eigen::Matrix4d::Identity(),
                                                 const ICPConvergenceCriteria &criteria = ICPConvergenceCriteria(),
                                                 double lambda_geometric = 0.968)
{
    return cicp::RegistrationICP(source, target, max_distance, init, TransformationEstimationForColoredICP(lambda_geometric), criteria);
}

// The colour gradient per point of a cloud with normals and colours, as the library computes it for colored ICP
// (visma_icp_color_gradient): what TransformationEstimationForColoredICP::color_gradient_ takes.
inline std::vector<Eigen::Vector3d> ComputeColorGradient(const PointCloud &cloud, double radius, int max_nn = 30)
{
    std::vector<Eigen::Vector3d> g(cloud.points_.size(), Eigen::Vector3d::Zero());
    if (g.empty() || !cloud.HasNormals() || !cloud.HasColors()) return g;
    visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
    detail::check(ctx, visma_icp_color_gradient(ctx, detail::xyz(cloud.points_), (int64_t)g.size(), detail::xyz(cloud.normals_),
                                                detail::xyz(cloud.colors_), radius, max_nn, g[0].data()),
                  "visma_icp_color_gradient");
    return g;
}

// feh::RegisterModelToScene (src/annotation.cpp:29-64) with its JSON options
// as plain arguments: rotation_level yaw initialisations about +Y, a full ICP
// from each, the first result with strictly the most correspondences wins.
// upright = true: every ICP rotates about +Y only (the orientation constrained
// ICP of the paper; the yaw starts are upright, so is every result).
inline Eigen::Matrix4d RegisterModelToScene(const PointCloud &model, const PointCloud &scene,
                                            int rotation_level, double distance_threshold,
                                            bool point_to_plane = false,
                                            RegistrationResult *best_out = nullptr,
                                            bool upright = false, double keep = 1.0,
                                            const cicp::RobustKernel *robust = nullptr)
{
    RegistrationResult best;
    const Eigen::Vector3d up = Eigen::Vector3d::UnitY();
    if (robust && keep != 1.0) {
        std::fprintf(stderr, "Error: RegisterModelToScene takes robust weights or keep < 1, not both.\n");
        return best.transformation_;
    }
    if (robust && rotation_level > 0 && distance_threshold > 0.0 && (!point_to_plane || (model.HasNormals() && scene.HasNormals()))) {
        // a robust ICP from every start, the winner by K as always; *best_out: the robust estimator's result of the winning start
        visma_icp_ctx *ctx = detail::upload(model, scene, point_to_plane, distance_threshold);
        detail::AxisScope axis(ctx, upright ? &up : nullptr);
        const ICPConvergenceCriteria c;
        const visma_icp_robust cfg = robust->c_config();
        visma_icp_result b;
        visma_icp_robust_info bi;
        int level = -1;
        detail::check(ctx, visma_icp_run_yaw_sweep_robust(ctx, rotation_level, distance_threshold, &cfg, point_to_plane ? 1 : 0,
                                                          c.max_iteration_, c.relative_fitness_, c.relative_rmse_, &b, &level,
                                                          nullptr, &bi, nullptr),
                      "visma_icp_run_yaw_sweep_robust");
        best.transformation_ = detail::from_rowmajor(b.transformation);
        best.fitness_ = b.fitness;
        best.inlier_rmse_ = bi.robust_rmse;
        if (best_out) {
            *best_out = best;
            if (level >= 0) {
                // one robust pass at the winning transform materialises its pairs (and their weights on the context)
                visma_icp_result r;
                visma_icp_robust_info ri;
                detail::check(ctx, visma_icp_run_robust(ctx, b.transformation, distance_threshold, &cfg, point_to_plane ? 1 : 0, 0,
                                                        0.0, 0.0, 0, &r, &ri), "visma_icp_run_robust");
                detail::fill_result(ctx, r, model.points_.size(), *best_out);
                best_out->inlier_rmse_ = ri.robust_rmse;
            }
        }
        return best.transformation_;
    }
    if (robust && point_to_plane) {
        std::fprintf(stderr, "Error: TransformationEstimationPointToPlane requires pre-computed normal vectors.\n");
        return best.transformation_;
    }
    if (keep != 1.0 && !(keep > 0.0 && keep < 1.0)) {
        std::fprintf(stderr, "Error: RegisterModelToScene requires keep in (0, 1].\n");
        return best.transformation_;
    }
    if (keep != 1.0 && point_to_plane) std::fprintf(stderr, "Warning: keep applies to the point-to-point estimator only; ignored.\n");
    if (keep != 1.0 && !point_to_plane && rotation_level > 0 && distance_threshold > 0.0) {
        // trimmed ICP from every start (keep: the share of the model the scan can see), the winner by K as always;
        // *best_out: TransformationEstimationPointToPointTrimmed's result of the winning start
        visma_icp_ctx *ctx = detail::upload(model, scene, false, distance_threshold);
        detail::AxisScope axis(ctx, upright ? &up : nullptr);
        const ICPConvergenceCriteria c;
        visma_icp_result b;
        visma_icp_trim_info bi;
        int level = -1;
        detail::check(ctx, visma_icp_run_yaw_sweep_trimmed(ctx, rotation_level, distance_threshold, keep, c.max_iteration_,
                                                           c.relative_fitness_, c.relative_rmse_, VISMA_ICP_SOLVER_KABSCH,
                                                           &b, &level, nullptr, &bi, nullptr),
                      "visma_icp_run_yaw_sweep_trimmed");
        best.transformation_ = detail::from_rowmajor(b.transformation);
        if (best_out) {
            *best_out = best;
            if (level >= 0) {
                // one trimmed pass at the winning transform materialises its kept pairs
                visma_icp_result r;
                visma_icp_trim_info ri;
                detail::check(ctx, visma_icp_run_trimmed(ctx, b.transformation, distance_threshold, keep, 0, 0.0, 0.0,
                                                         VISMA_ICP_SOLVER_KABSCH, 0, &r, &ri), "visma_icp_run_trimmed");
                detail::fill_result_trimmed(ctx, r, ri, model.points_.size(), *best_out);
            }
        }
        return best.transformation_;
    }
    const bool plane_ready = point_to_plane && model.HasNormals() && scene.HasNormals();
    if ((!point_to_plane || plane_ready) && rotation_level > 0 && distance_threshold > 0.0) {
        // all levels in one library call (the sweep is advanced on the GPU), either estimator
        visma_icp_ctx *ctx = detail::upload(model, scene, point_to_plane, distance_threshold);
        detail::AxisScope axis(ctx, upright ? &up : nullptr);
        visma_icp_result b;
        int level = -1;
        const ICPConvergenceCriteria c;
        if (point_to_plane)
            detail::check(ctx, visma_icp_run_yaw_sweep_point_to_plane(ctx, rotation_level, distance_threshold,
                                                                      c.max_iteration_, c.relative_fitness_,
                                                                      c.relative_rmse_, &b, &level, nullptr),
                          "visma_icp_run_yaw_sweep_point_to_plane");
        else
            detail::check(ctx, visma_icp_run_yaw_sweep(ctx, rotation_level, distance_threshold,
                                                       c.max_iteration_, c.relative_fitness_,
                                                       c.relative_rmse_, VISMA_ICP_SOLVER_KABSCH, &b,
                                                       &level, nullptr),
                          "visma_icp_run_yaw_sweep");
        best.transformation_ = detail::from_rowmajor(b.transformation);
        best.fitness_ = b.fitness;
        best.inlier_rmse_ = b.inlier_rmse;
        if (best_out) {
            // re-evaluate at the winning transform to materialise its correspondences
            *best_out = level >= 0 ? cicp::EvaluateRegistration(model, scene, distance_threshold,
                                                          best.transformation_)
                                   : best;
        }
        return best.transformation_;
    }
    const double interval = 2.0 * M_PI / rotation_level;
    for (int i = 0; i < rotation_level; ++i) {
        const double a = interval * i, c = std::cos(a), s = std::sin(a);
        Eigen::Matrix4d init = Eigen::Matrix4d::Identity();
        init(0, 0) = c; init(0, 2) = s; init(2, 0) = -s; init(2, 2) = c;
        RegistrationResult r;
        if (upright && point_to_plane)
            r = cicp::RegistrationICP(model, scene, distance_threshold, init,
                                      TransformationEstimationPointToPlaneYaw(up), ICPConvergenceCriteria());
        else if (upright)
            r = cicp::RegistrationICP(model, scene, distance_threshold, init,
                                      TransformationEstimationPointToPointYaw(up), ICPConvergenceCriteria());
        else if (point_to_plane)
            r = cicp::RegistrationICP(model, scene, distance_threshold, init,
                                TransformationEstimationPointToPlane(), ICPConvergenceCriteria());
        else
            r = cicp::RegistrationICP(model, scene, distance_threshold, init,
                                TransformationEstimationPointToPoint4DoF(), ICPConvergenceCriteria());
        if (r.correspondence_set_.size() > best.correspondence_set_.size()) best = r;
    }
    if (best_out) *best_out = best;
    return best.transformation_;
}

// The per-object loop of feh::AnnotationTool (src/annotation.cpp:103-168) for MANY (model, scan) pairs at
// once: what the loop body hands to RegisterModelToScene, collected first, registered together by the
// library's native work queue (visma_icp_run_corpus: one host thread per GPU pulls chunks of pairs, each
// chunk's rotation_level yaw starts run as one batch), the loop's T3 per pair returned in order.
// `devices`: one queue worker (context, own stream) per entry -- the SAME GPU may be listed several times, and should:
// while one worker packs and uploads its next chunk, the others' searches have the device (three on one GPU: ~1.5x one).
// Empty = three workers on device 0.  Point-to-point estimator (ICP.point_to_plane = false).
// upright = true: every ICP rotates about +Y only (as RegisterModelToScene's).
inline std::vector<Eigen::Matrix4d> RegisterModelsToScenes(
    const std::vector<std::pair<std::shared_ptr<PointCloud>, std::shared_ptr<PointCloud>>> &model_scan_pairs,
    int rotation_level, double distance_threshold, const std::vector<int> &devices = std::vector<int>(),
    std::vector<RegistrationResult> *best_out = nullptr, bool upright = false)
{
    const size_t n = model_scan_pairs.size();
    std::vector<Eigen::Matrix4d> T(n, Eigen::Matrix4d::Identity());
    if (best_out) best_out->assign(n, RegistrationResult());
    if (n == 0 || rotation_level <= 0 || !(distance_threshold > 0.0)) return T;
    std::vector<visma_icp_corpus_item> items(n);
    for (size_t i = 0; i < n; i++) {
        const PointCloud &m = *model_scan_pairs[i].first, &sc = *model_scan_pairs[i].second;
        // std::vector<Eigen::Vector3d> is AoS f64 with stride 3 (static_assert in detail::upload)
        items[i].model_xyz = m.points_.empty() ? nullptr : m.points_[0].data();
        items[i].n_model = (int64_t)m.points_.size();
        items[i].scene_xyz = sc.points_.empty() ? nullptr : sc.points_[0].data();
        items[i].n_scene = (int64_t)sc.points_.size();
    }
    std::vector<visma_icp_ctx *> ctxs;
    const std::vector<int> devs = devices.empty() ? std::vector<int>(3, 0) : devices;   // (three workers on GPU 0)
    auto destroy_all = [&]() { for (visma_icp_ctx *c : ctxs) visma_icp_destroy(c); };
    for (int d : devs) {
        visma_icp_ctx *c = nullptr;
        if (visma_icp_create(&c, d) != VISMA_ICP_OK) { destroy_all(); throw std::runtime_error("visma_icp_create failed (no gfx950 GPU?)"); }
        ctxs.push_back(c);
        const double up[3] = {0.0, 1.0, 0.0};
        if (upright && visma_icp_set_rotation_axis(c, up) != VISMA_ICP_OK) {
            destroy_all();
            throw std::runtime_error("visma_icp_set_rotation_axis failed");
        }
    }
    const ICPConvergenceCriteria crit;
    visma_icp_corpus_params p;
    p.level = rotation_level; p.max_dist = distance_threshold; p.max_iter = crit.max_iteration_;
    p.rel_fitness = crit.relative_fitness_; p.rel_rmse = crit.relative_rmse_; p.solver = VISMA_ICP_SOLVER_KABSCH; p.chunk = 0;
    std::vector<visma_icp_corpus_result> res(n);
    char err[512];
    const int rc = visma_icp_run_corpus(ctxs.data(), (int)ctxs.size(), items.data(), (int64_t)n, &p, nullptr, res.data(), err, sizeof(err));
    destroy_all();
    if (rc != VISMA_ICP_OK) throw std::runtime_error(std::string("visma_icp_run_corpus: ") + err);
    for (size_t i = 0; i < n; i++) {
        T[i] = detail::from_rowmajor(res[i].best.transformation);
        if (best_out) {
            RegistrationResult &b = (*best_out)[i];
            b.transformation_ = T[i];
            b.fitness_ = res[i].best.fitness;
            b.inlier_rmse_ = res[i].best.inlier_rmse;
        }
    }
    return T;
}

// open3d::VoxelDownSample (O3D/Core/Geometry/DownSample.cpp:179-220) on the GPU:
// same points / normals / colours, bit for bit; voxels come out in ascending
// (ix,iy,iz) order instead of the reference's hash-map iteration order.
inline std::shared_ptr<PointCloud> VoxelDownSample(const PointCloud &input, double voxel_size)
{
    auto output = std::make_shared<PointCloud>();
    const int64_t n = (int64_t)input.points_.size();
    if (voxel_size <= 0.0 || n == 0) return output;
    visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
    const bool hn = input.HasNormals(), hc = input.HasColors();
    output->points_.resize((size_t)n);
    if (hn) output->normals_.resize((size_t)n);
    if (hc) output->colors_.resize((size_t)n);
    int64_t m = 0;
    detail::check(ctx, visma_icp_voxel_down_sample(
                           ctx, detail::xyz(input.points_), n, hn ? detail::xyz(input.normals_) : nullptr,
                           hc ? detail::xyz(input.colors_) : nullptr, voxel_size,
                           output->points_[0].data(), hn ? output->normals_[0].data() : nullptr,
                           hc ? output->colors_[0].data() : nullptr, &m),
                  "visma_icp_voxel_down_sample");
    output->points_.resize((size_t)m);
    if (hn) output->normals_.resize((size_t)m);
    if (hc) output->colors_.resize((size_t)m);
    return output;
}

namespace detail {
// a KDTreeSearchParam as the C ABI takes it: search_type 0 KNN | 1 Radius | 2 Hybrid, knn (max_nn), radius
inline void search_arguments(const KDTreeSearchParam &search_param, int *type, int *knn, double *radius)
{
    *type = 0; *knn = 0; *radius = 0.0;
    switch (search_param.GetSearchType()) {
    case KDTreeSearchParam::SearchType::Knn:
        *knn = static_cast<const KDTreeSearchParamKNN &>(search_param).knn_;
        break;
    case KDTreeSearchParam::SearchType::Radius:
        *type = 1;
        *radius = static_cast<const KDTreeSearchParamRadius &>(search_param).radius_;
        break;
    case KDTreeSearchParam::SearchType::Hybrid:
        *type = 2;
        *radius = static_cast<const KDTreeSearchParamHybrid &>(search_param).radius_;
        *knn = static_cast<const KDTreeSearchParamHybrid &>(search_param).max_nn_;
        break;
    }
}
}  // namespace detail

// open3d::EstimateNormals (O3D/Core/Geometry/EstimateNormals.cpp:114-153) on the GPU: the three
// KDTreeFlann searches, FastEigen3x3, (0,0,1) for fewer than 3 neighbours, the sign of existing normals
// kept.  What a caller runs before the point-to-plane estimator on clouds without normals
// (Registration.cpp:152-157 returns the initial transform otherwise).
inline bool EstimateNormals(PointCloud &cloud, const KDTreeSearchParam &search_param = KDTreeSearchParamKNN())
{
    const int64_t n = (int64_t)cloud.points_.size();
    const bool has_normal = cloud.HasNormals();
    int type = 0, knn = 0;
    double radius = 0.0;
    detail::search_arguments(search_param, &type, &knn, &radius);
    std::vector<Eigen::Vector3d> out((size_t)n);
    if (n > 0) {
        visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
        detail::check(ctx, visma_icp_estimate_normals(ctx, detail::xyz(cloud.points_), n,
                                                      has_normal ? detail::xyz(cloud.normals_) : nullptr, type, knn,
                                                      radius, out[0].data()),
                      "visma_icp_estimate_normals");
    }
    cloud.normals_.swap(out);
    return true;
}

// open3d::ComputeFPFHFeature (O3D/Core/Registration/Feature.cpp:112-157) on the GPU: column i of data_ is the FPFH of
// point i.  KNN and Hybrid searches with a list length in [2, 170]; a cloud without normals gives zeros, as the
// reference does.
inline std::shared_ptr<Feature> ComputeFPFHFeature(const PointCloud &input, const KDTreeSearchParam &search_param = KDTreeSearchParamKNN())
{
    auto feature = std::make_shared<Feature>();
    const int64_t n = (int64_t)input.points_.size();
    feature->Resize(VISMA_FPFH_DIM, (int)n);
    if (n == 0 || !input.HasNormals()) return feature;
    int type = 0, knn = 0;
    double radius = 0.0;
    switch (search_param.GetSearchType()) {
    case KDTreeSearchParam::SearchType::Knn:
        knn = static_cast<const KDTreeSearchParamKNN &>(search_param).knn_;
        break;
    case KDTreeSearchParam::SearchType::Radius:
        type = 1;
        break;
    case KDTreeSearchParam::SearchType::Hybrid:
        type = 2;
        radius = static_cast<const KDTreeSearchParamHybrid &>(search_param).radius_;
        knn = static_cast<const KDTreeSearchParamHybrid &>(search_param).max_nn_;
        break;
    }
    std::vector<double> rows((size_t)n * VISMA_FPFH_DIM);
    visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
    detail::check(ctx, visma_icp_compute_fpfh(ctx, detail::xyz(input.points_), n, detail::xyz(input.normals_), type, knn, radius,
                                              rows.data()),
                  "visma_icp_compute_fpfh");
    for (int64_t i = 0; i < n; i++)
        for (int j = 0; j < VISMA_FPFH_DIM; j++) feature->data_(j, i) = rows[(size_t)i * VISMA_FPFH_DIM + j];
    return feature;
}

using FastGlobalRegistrationOption = open3d::FastGlobalRegistrationOption;

namespace detail {

inline visma_icp_fgr_option fgr_option(const FastGlobalRegistrationOption &o)
{
    visma_icp_fgr_option c;
    c.division_factor = o.division_factor_; c.max_corr_dist = o.maximum_correspondence_distance_; c.tuple_scale = o.tuple_scale_;
    c.use_absolute_scale = o.use_absolute_scale_ ? 1 : 0; c.decrease_mu = o.decrease_mu_ ? 1 : 0;
    c.iteration_number = o.iteration_number_; c.maximum_tuple_count = o.maximum_tuple_count_;
    return c;
}

// point-major rows of a Feature (its columns), whatever the storage order of data_
inline std::vector<double> feature_rows(const Feature &f)
{
    const int64_t dim = (int64_t)f.data_.rows(), n = (int64_t)f.data_.cols();
    std::vector<double> rows((size_t)(dim * n));
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = 0; j < dim; j++) rows[(size_t)(i * dim + j)] = f.data_(j, i);
    return rows;
}

// fast global registration's optimisation over given pairs (source index, target index), host only
// (visma_icp_fgr_optimize): the transform source-to-target; opt_out (may be NULL) what OptimizePairwiseRegistration returned
inline Eigen::Matrix4d fgr_optimize(const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres,
                                    const FastGlobalRegistrationOption &option, Eigen::Matrix4d *opt_out = nullptr)
{
    std::vector<int32_t> si(corres.size()), ti(corres.size());
    for (size_t c = 0; c < corres.size(); c++) { si[c] = corres[c][0]; ti[c] = corres[c][1]; }
    const visma_icp_fgr_option o = fgr_option(option);
    double T[16], Topt[16];
    if (visma_icp_fgr_optimize(xyz(source.points_), (int64_t)source.points_.size(), xyz(target.points_),
                               (int64_t)target.points_.size(), si.data(), ti.data(), (int64_t)si.size(), &o, T, Topt) != VISMA_ICP_OK)
        throw std::runtime_error("visma_icp_fgr_optimize: bad arguments");
    if (opt_out) *opt_out = from_rowmajor(Topt);
    return from_rowmajor(T);
}

}  // namespace detail

// open3d::FastGlobalRegistration (O3D/Core/Registration/FastGlobalRegistration.cpp:347-375): matching on the GPU, the rest
// on the host.  The reference seeds rand() from the clock; here the tuple test draws from a Philox stream keyed by `seed`
// (visma_icp.h), 0 for the overload without one: a registration is reproducible.  The result holds the transformation
// only, as the reference's does.  Features of another dimension than 33, or not one per point: the identity, with a message.
inline RegistrationResult FastGlobalRegistration(const PointCloud &source, const PointCloud &target, const Feature &source_feature,
                                                 const Feature &target_feature, const FastGlobalRegistrationOption &option,
                                                 uint64_t seed)
{
    if (source_feature.Dimension() != VISMA_FPFH_DIM || target_feature.Dimension() != VISMA_FPFH_DIM ||
        source_feature.Num() != source.points_.size() || target_feature.Num() != target.points_.size() ||
        source.points_.empty() || target.points_.empty()) {
        std::fprintf(stderr, "Error: FastGlobalRegistration requires one 33-dimensional feature per point of two non-empty clouds.\n");
        return RegistrationResult(Eigen::Matrix4d::Identity());
    }
    const std::vector<double> fs = detail::feature_rows(source_feature), ft = detail::feature_rows(target_feature);
    const visma_icp_fgr_option o = detail::fgr_option(option);
    visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
    double T[16];
    detail::check(ctx, visma_icp_fast_global_registration(ctx, detail::xyz(source.points_), (int64_t)source.points_.size(), fs.data(),
                                                          detail::xyz(target.points_), (int64_t)target.points_.size(), ft.data(), &o,
                                                          seed, nullptr, 0, T, nullptr),
                  "visma_icp_fast_global_registration");
    return RegistrationResult(detail::from_rowmajor(T));
}

inline RegistrationResult FastGlobalRegistration(const PointCloud &source, const PointCloud &target, const Feature &source_feature,
                                                 const Feature &target_feature,
                                                 const FastGlobalRegistrationOption &option = FastGlobalRegistrationOption())
{
    return cicp::FastGlobalRegistration(source, target, source_feature, target_feature, option, 0);
}

namespace detail {

// RANSAC runs TransformationEstimationPointToPoint(false) only (the stock class or the 4DoF one, which is the same
// arithmetic without an axis); anything else is reported and the caller gets the reference's empty result
inline bool ransac_estimation_supported(const TransformationEstimation &estimation, const char *who)
{
    const std::type_info &dyn = typeid(estimation);
    const auto *p2p = dyn == typeid(TransformationEstimationPointToPoint) ? static_cast<const TransformationEstimationPointToPoint *>(&estimation) : nullptr;
    const auto *four = dyn == typeid(TransformationEstimationPointToPoint4DoF) ? static_cast<const TransformationEstimationPointToPoint4DoF *>(&estimation) : nullptr;
    if ((p2p && !p2p->with_scaling_) || (four && !four->with_scaling_)) return true;
    std::fprintf(stderr, "Error: %s: unsupported estimation (only TransformationEstimationPointToPoint(false) runs on the GPU).\n", who);
    return false;
}

}  // namespace detail

// open3d::RegistrationRANSACBasedOnFeatureMatching (O3D/Core/Registration/Registration.cpp:226-353) on the GPU
// (visma_icp.h, "RANSAC global registration").  The reference seeds rand() from the clock and races its threads for the
// validation count; here trial t draws from a Philox stream keyed by `seed` (0 for the overload without one) and the
// validated trials are the first max_validation_ that pass, in trial order: a registration is reproducible.  The checkers
// must be the three built-in classes, one of each at most, with a positive distance and a non-zero angle (the GPU cannot
// call a user's virtual Check); ransac_n lies in [3, 8].  Outside
// that, an estimation other than point-to-point without scaling, features that are not one per point, or the reference's
// own early returns: RegistrationResult(), with a message where the reference has none.
inline RegistrationResult RegistrationRANSACBasedOnFeatureMatching(
    const PointCloud &source, const PointCloud &target, const Feature &source_feature, const Feature &target_feature,
    double max_correspondence_distance, const TransformationEstimation &estimation, int ransac_n,
    const std::vector<std::reference_wrapper<const CorrespondenceChecker>> &checkers, const RANSACConvergenceCriteria &criteria,
    uint64_t seed)
{
    if (ransac_n < 3 || max_correspondence_distance <= 0.0) return RegistrationResult();
    if (!detail::ransac_estimation_supported(estimation, "RegistrationRANSACBasedOnFeatureMatching")) return RegistrationResult();
    visma_icp_ransac_option o = {ransac_n, criteria.max_iteration_, criteria.max_validation_, 0.0, 0.0, 0.0, 0};
    bool has_edge = false, has_distance = false, has_normal = false;
    for (const auto &c : checkers) {
        const std::type_info &dyn = typeid(c.get());
        if (dyn == typeid(CorrespondenceCheckerBasedOnEdgeLength) && !has_edge) {
            // (a similarity <= 0 rejects nothing in the reference either: the option's "off" is the same checker)
            has_edge = true;
            o.edge_length_similarity = static_cast<const CorrespondenceCheckerBasedOnEdgeLength &>(c.get()).similarity_threshold_;
        } else if (dyn == typeid(CorrespondenceCheckerBasedOnDistance) && !has_distance) {
            has_distance = true;
            o.distance_threshold = static_cast<const CorrespondenceCheckerBasedOnDistance &>(c.get()).distance_threshold_;
        } else if (dyn == typeid(CorrespondenceCheckerBasedOnNormal) && !has_normal) {
            has_normal = true;                                   // (cos is even: a negative angle is the same checker)
            o.normal_angle = std::fabs(static_cast<const CorrespondenceCheckerBasedOnNormal &>(c.get()).normal_angle_threshold_);
        }
        else {
            std::fprintf(stderr, "Error: RegistrationRANSACBasedOnFeatureMatching: unsupported checker (one each of the three "
                                 "built-in CorrespondenceChecker classes runs on the GPU).\n");
            return RegistrationResult();
        }
    }
    // in visma_icp_ransac_option a threshold <= 0 means "no checker"; the reference's distance checker at <= 0 rejects every
    // trial and its normal checker at 0 asks for a dot product >= 1: neither can be said there, so they are reported
    if ((has_distance && !(o.distance_threshold > 0.0)) || (has_normal && !(o.normal_angle > 0.0))) {
        std::fprintf(stderr, "Error: RegistrationRANSACBasedOnFeatureMatching: unsupported checker threshold (a distance and an angle "
                             "must be positive).\n");
        return RegistrationResult();
    }
    if (ransac_n > 8 || source.points_.empty() || target.points_.empty() || source_feature.Dimension() != target_feature.Dimension() ||
        source_feature.Dimension() < 1 || source_feature.Dimension() > 64 || source_feature.Num() != source.points_.size() ||
        target_feature.Num() != target.points_.size()) {
        std::fprintf(stderr, "Error: RegistrationRANSACBasedOnFeatureMatching: unsupported arguments (ransac_n in [3, 8], one feature "
                             "of 1 to 64 dimensions per point of two non-empty clouds).\n");
        return RegistrationResult();
    }
    const std::vector<double> fs = detail::feature_rows(source_feature), ft = detail::feature_rows(target_feature);
    const bool normals = source.HasNormals() && target.HasNormals();
    visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
    visma_icp_result r;
    detail::check(ctx, visma_icp_registration_ransac_feature_matching(
                           ctx, detail::xyz(source.points_), (int64_t)source.points_.size(), fs.data(), detail::xyz(target.points_),
                           (int64_t)target.points_.size(), ft.data(), (int)source_feature.Dimension(),
                           normals ? detail::xyz(source.normals_) : nullptr, normals ? detail::xyz(target.normals_) : nullptr,
                           max_correspondence_distance, &o, seed, nullptr, 0, &r, nullptr),
                  "visma_icp_registration_ransac_feature_matching");
    RegistrationResult result;
    if (r.num_correspondences > 0) detail::fill_result(ctx, r, source.points_.size(), result);
    return result;
}

inline RegistrationResult RegistrationRANSACBasedOnFeatureMatching(
    const PointCloud &source, const PointCloud &target, const Feature &source_feature, const Feature &target_feature,
    double max_correspondence_distance, const TransformationEstimation &estimation = TransformationEstimationPointToPoint(false),
    int ransac_n = 4, const std::vector<std::reference_wrapper<const CorrespondenceChecker>> &checkers = {},
    const RANSACConvergenceCriteria &criteria = RANSACConvergenceCriteria())
{
    return cicp::RegistrationRANSACBasedOnFeatureMatching(source, target, source_feature, target_feature, max_correspondence_distance,
                                                          estimation, ransac_n, checkers, criteria, 0);
}

// open3d::RegistrationRANSACBasedOnCorrespondence (Registration.cpp:188-224): fitness and rmse over the pair list, no
// correspondence set, as the reference returns it
inline RegistrationResult RegistrationRANSACBasedOnCorrespondence(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres, double max_correspondence_distance,
    const TransformationEstimation &estimation, int ransac_n, const RANSACConvergenceCriteria &criteria, uint64_t seed)
{
    if (ransac_n < 3 || (int)corres.size() < ransac_n || max_correspondence_distance <= 0.0) return RegistrationResult();
    if (!detail::ransac_estimation_supported(estimation, "RegistrationRANSACBasedOnCorrespondence")) return RegistrationResult();
    if (ransac_n > 8 || source.points_.empty() || target.points_.empty()) {
        std::fprintf(stderr, "Error: RegistrationRANSACBasedOnCorrespondence: unsupported arguments (ransac_n in [3, 8], two "
                             "non-empty clouds).\n");
        return RegistrationResult();
    }
    std::vector<int32_t> si(corres.size()), ti(corres.size());
    for (size_t c = 0; c < corres.size(); c++) { si[c] = corres[c][0]; ti[c] = corres[c][1]; }
    visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
    visma_icp_result r;
    detail::check(ctx, visma_icp_registration_ransac_correspondence(
                           ctx, detail::xyz(source.points_), (int64_t)source.points_.size(), detail::xyz(target.points_),
                           (int64_t)target.points_.size(), si.data(), ti.data(), (int64_t)si.size(), max_correspondence_distance,
                           ransac_n, criteria.max_iteration_, criteria.max_validation_, seed, nullptr, 0, &r, nullptr),
                  "visma_icp_registration_ransac_correspondence");
    RegistrationResult result(detail::from_rowmajor(r.transformation));
    result.fitness_ = r.fitness;
    result.inlier_rmse_ = r.inlier_rmse;
    return result;
}

inline RegistrationResult RegistrationRANSACBasedOnCorrespondence(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres, double max_correspondence_distance,
    const TransformationEstimation &estimation = TransformationEstimationPointToPoint(false), int ransac_n = 6,
    const RANSACConvergenceCriteria &criteria = RANSACConvergenceCriteria())
{
    return cicp::RegistrationRANSACBasedOnCorrespondence(source, target, corres, max_correspondence_distance, estimation, ransac_n,
                                                         criteria, 0);
}

// open3d::GetInformationMatrixFromPointClouds (Registration.cpp:355-413) on the GPU: sum G^T G over the pairs of a pass at
// `transformation`, G = [-hat(q) | I] with q the target point.  NOT the reference's value: it adds (1 + P) I, P its number
// of OpenMP threads; this is the pure sum, (5, 5) the number of pairs (visma_icp.h).
inline Eigen::Matrix6d GetInformationMatrixFromPointClouds(const PointCloud &source, const PointCloud &target,
                                                           double max_correspondence_distance,
                                                           const Eigen::Matrix4d &transformation)
{
    Eigen::Matrix6d G = Eigen::Matrix6d::Zero();
    if (source.points_.empty() || target.points_.empty() || !(max_correspondence_distance > 0.0)) return G;
    visma_icp_ctx *ctx = detail::upload(source, target, false, max_correspondence_distance);
    double T[16], out[36];
    detail::to_rowmajor(transformation, T);
    detail::check(ctx, visma_icp_information_matrix(ctx, T, max_correspondence_distance, out, nullptr), "visma_icp_information_matrix");
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) G(i, j) = out[i * 6 + j];
    return G;
}

// ... for every edge of a pose graph in one call: clouds[i] is the cloud of node i; edge e gets
// information_ = GetInformationMatrixFromPointClouds(clouds[source], clouds[target], max_distance, e.transformation_).
// Edges with the same target node share its upload.  An edge naming no cloud, or an empty cloud, keeps its matrix.
inline void GetInformationMatrixFromPointClouds(PoseGraph &pose_graph, const std::vector<const PointCloud *> &clouds,
                                                double max_correspondence_distance)
{
    std::vector<visma_icp_problem> probs;
    std::vector<size_t> which;
    for (size_t e = 0; e < pose_graph.edges_.size(); e++) {
        const PoseGraphEdge &t = pose_graph.edges_[e];
        if (t.source_node_id_ < 0 || t.target_node_id_ < 0 || (size_t)t.source_node_id_ >= clouds.size() ||
            (size_t)t.target_node_id_ >= clouds.size() || !clouds[t.source_node_id_] || !clouds[t.target_node_id_]) continue;
        const PointCloud &s = *clouds[t.source_node_id_], &q = *clouds[t.target_node_id_];
        if (s.points_.empty() || q.points_.empty()) continue;
        visma_icp_problem p;
        p.src_xyz = detail::xyz(s.points_); p.ns = (int64_t)s.points_.size();
        p.tgt_xyz = detail::xyz(q.points_); p.nt = (int64_t)q.points_.size();
        detail::to_rowmajor(t.transformation_, p.init);
        p.max_dist = max_correspondence_distance;
        probs.push_back(p);
        which.push_back(e);
    }
    if (probs.empty() || !(max_correspondence_distance > 0.0)) return;
    std::vector<double> out(probs.size() * 36);
    visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
    detail::check(ctx, visma_icp_information_matrices(ctx, probs.data(), (int)probs.size(), out.data(), nullptr),
                  "visma_icp_information_matrices");
    for (size_t k = 0; k < which.size(); k++)
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) pose_graph.edges_[which[k]].information_(i, j) = out[k * 36 + i * 6 + j];
}

namespace detail {

// a PoseGraph through visma_icp_global_optimization (whole) or visma_icp_pose_graph_optimize (one optimisation)
inline void run_pose_graph(PoseGraph &g, bool whole, int method, const GlobalOptimizationConvergenceCriteria &c,
                           const GlobalOptimizationOption &o)
{
    std::vector<double> poses(g.nodes_.size() * 16);
    for (size_t i = 0; i < g.nodes_.size(); i++) to_rowmajor(g.nodes_[i].pose_, &poses[i * 16]);
    std::vector<visma_icp_pose_graph_edge> edges(g.edges_.size());
    for (size_t e = 0; e < g.edges_.size(); e++) {
        const PoseGraphEdge &t = g.edges_[e];
        edges[e].source = t.source_node_id_; edges[e].target = t.target_node_id_;
        to_rowmajor(t.transformation_, edges[e].transformation);
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) edges[e].information[i * 6 + j] = t.information_(i, j);
        edges[e].uncertain = t.uncertain_ ? 1 : 0;
        edges[e].confidence = t.confidence_;
    }
    const visma_icp_global_optimization_criteria cc = {c.max_iteration_, c.min_relative_increment_, c.min_relative_residual_increment_,
                                                       c.min_right_term_, c.min_residual_, c.max_iteration_lm_,
                                                       c.upper_scale_factor_, c.lower_scale_factor_};
    const visma_icp_global_optimization_option oo = {o.max_correspondence_distance_, o.edge_prune_threshold_,
                                                     o.preference_loop_closure_, o.reference_node_};
    int ne = (int)edges.size();
    const int rc = whole ? visma_icp_global_optimization(poses.data(), (int)g.nodes_.size(), edges.data(), &ne, method, &cc, &oo)
                         : visma_icp_pose_graph_optimize(poses.data(), (int)g.nodes_.size(), edges.data(), ne, method, &cc, &oo);
    if (rc != VISMA_ICP_OK) {
        std::fprintf(stderr, "Error: pose-graph optimisation: an edge names a node outside the graph.\n");
        return;
    }
    for (size_t i = 0; i < g.nodes_.size(); i++) g.nodes_[i].pose_ = from_rowmajor(&poses[i * 16]);
    std::vector<PoseGraphEdge> kept;                         // the surviving edges as the library returns them, member by member
    for (int k = 0; k < ne; k++) {
        Eigen::Matrix6d info;
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) info(i, j) = edges[k].information[i * 6 + j];
        kept.push_back(PoseGraphEdge(edges[k].source, edges[k].target, from_rowmajor(edges[k].transformation), info,
                                     edges[k].uncertain != 0, edges[k].confidence));
    }
    g.edges_.swap(kept);
}

inline int pose_graph_method(const GlobalOptimizationMethod &method)
{
    return dynamic_cast<const GlobalOptimizationGaussNewton *>(&method) ? VISMA_ICP_GLOBAL_GAUSS_NEWTON
                                                                        : VISMA_ICP_GLOBAL_LEVENBERG_MARQUARDT;
}

}  // namespace detail

// open3d::GlobalOptimization (GlobalOptimization.cpp:641-662) on the host: both methods restated test by test
// (visma_icp.h).  `method`: a GlobalOptimizationGaussNewton selects Gauss-Newton, any other Levenberg-Marquardt.
inline void GlobalOptimization(PoseGraph &pose_graph, const GlobalOptimizationMethod &method,
                               const GlobalOptimizationConvergenceCriteria &criteria = GlobalOptimizationConvergenceCriteria(),
                               const GlobalOptimizationOption &option = GlobalOptimizationOption())
{
    detail::run_pose_graph(pose_graph, true, detail::pose_graph_method(method), criteria, option);
}

// ... with the reference's default method.  (No default argument above: the real Open3D headers declare the method
// classes without bodies a header-only adapter could construct.)
inline void GlobalOptimization(PoseGraph &pose_graph)
{
    detail::run_pose_graph(pose_graph, true, VISMA_ICP_GLOBAL_LEVENBERG_MARQUARDT, GlobalOptimizationConvergenceCriteria(),
                           GlobalOptimizationOption());
}

// open3d::ComputePointCloudToPointCloudDistance (O3D/Core/Geometry/PointCloud.cpp:122-142) on the GPU: for every
// source point the distance to the nearest target point, no radius, bit for bit the reference's (0 for every
// point when the target is empty).
inline std::vector<double> ComputePointCloudToPointCloudDistance(const PointCloud &source, const PointCloud &target)
{
    std::vector<double> distances(source.points_.size());
    if (!distances.empty()) {
        visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
        detail::check(ctx, visma_icp_point_cloud_distance(ctx, detail::xyz(source.points_),
                                                          (int64_t)source.points_.size(), detail::xyz(target.points_),
                                                          (int64_t)target.points_.size(), distances.data()),
                      "visma_icp_point_cloud_distance");
    }
    return distances;
}

// open3d::ComputePointCloudNearestNeighborDistance (PointCloud.cpp:200-219) on the GPU: for every point the
// distance to the nearest other point of the cloud (0 for a duplicate point and for a one-point cloud).
inline std::vector<double> ComputePointCloudNearestNeighborDistance(const PointCloud &input)
{
    std::vector<double> nn_dis(input.points_.size());
    if (!nn_dis.empty()) {
        visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
        detail::check(ctx, visma_icp_nearest_neighbor_distance(ctx, detail::xyz(input.points_),
                                                               (int64_t)input.points_.size(), nn_dis.data()),
                      "visma_icp_nearest_neighbor_distance");
    }
    return nn_dis;
}

// O3D/Core/Geometry/EstimateNormals.cpp:155-174
inline bool OrientNormalsToAlignWithDirection(PointCloud &cloud,
                                              const Eigen::Vector3d &orientation_reference = Eigen::Vector3d(0.0, 0.0, 1.0))
{
    for (auto &normal : cloud.normals_) {
        if (normal.norm() == 0.0) normal = orientation_reference;
        else if (normal.dot(orientation_reference) < 0.0) normal *= -1.0;
    }
    return true;
}

// O3D/Core/Geometry/EstimateNormals.cpp:176-204
inline bool OrientNormalsTowardsCameraLocation(PointCloud &cloud,
                                               const Eigen::Vector3d &camera_location = Eigen::Vector3d::Zero())
{
    const size_t n = cloud.HasNormals() ? cloud.points_.size() : 0;
    for (size_t i = 0; i < n; i++) {
        const Eigen::Vector3d towards = camera_location - cloud.points_[i];
        Eigen::Vector3d &normal = cloud.normals_[i];
        if (normal.norm() == 0.0) {
            normal = towards;
            if (normal.norm() == 0.0) normal = Eigen::Vector3d(0.0, 0.0, 1.0);
            else normal.normalize();
        } else if (normal.dot(towards) < 0.0) {
            normal *= -1.0;
        }
    }
    return true;
}

// open3d::ReadPointCloudFromPCD (O3D/IO/FileFormat/FilePCD.cpp:727-742): ascii, binary and
// binary_compressed files; the reader's values bit for bit (include/visma_io.h).
inline bool ReadPointCloudFromPCD(const std::string &filename, PointCloud &pointcloud)
{
    visma_io_cloud c;
    if (visma_io_read_pcd(filename.c_str(), &c) != VISMA_IO_OK) {
        std::fprintf(stderr, "Read PCD failed: %s\n", visma_io_last_error());
        return false;
    }
    pointcloud.points_.resize((size_t)c.n);
    pointcloud.normals_.resize((size_t)c.n_normals);
    pointcloud.colors_.resize((size_t)c.n_colors);
    for (int64_t i = 0; i < c.n; i++) pointcloud.points_[(size_t)i] = Eigen::Vector3d(c.xyz[3 * i], c.xyz[3 * i + 1], c.xyz[3 * i + 2]);
    for (int64_t i = 0; i < c.n_normals; i++)
        pointcloud.normals_[(size_t)i] = Eigen::Vector3d(c.normals[3 * i], c.normals[3 * i + 1], c.normals[3 * i + 2]);
    for (int64_t i = 0; i < c.n_colors; i++)
        pointcloud.colors_[(size_t)i] = Eigen::Vector3d(c.colors[3 * i], c.colors[3 * i + 1], c.colors[3 * i + 2]);
    visma_io_free_cloud(&c);
    return true;
}

// open3d::ReadPointCloudFromPLY (O3D/IO/FileFormat/FilePLY.cpp:206-264): the scene and scan
// clouds of both callers (src/evaluation.cpp:124,211; src/annotation.cpp:76-157).  Same
// points / normals / colours as the rply-based reader; false (and a message on stderr) on
// failure, like the reference.
inline bool ReadPointCloudFromPLY(const std::string &filename, PointCloud &pointcloud)
{
    visma_io_cloud c;
    if (visma_io_read_ply(filename.c_str(), &c) != VISMA_IO_OK) {
        std::fprintf(stderr, "Read PLY failed: %s\n", visma_io_last_error());
        return false;
    }
    pointcloud.points_.resize((size_t)c.n);
    pointcloud.normals_.resize((size_t)c.n_normals);
    pointcloud.colors_.resize((size_t)c.n_colors);
    for (int64_t i = 0; i < c.n; i++) pointcloud.points_[(size_t)i] = Eigen::Vector3d(c.xyz[3 * i], c.xyz[3 * i + 1], c.xyz[3 * i + 2]);
    for (int64_t i = 0; i < c.n_normals; i++)
        pointcloud.normals_[(size_t)i] = Eigen::Vector3d(c.normals[3 * i], c.normals[3 * i + 1], c.normals[3 * i + 2]);
    for (int64_t i = 0; i < c.n_colors; i++)
        pointcloud.colors_[(size_t)i] = Eigen::Vector3d(c.colors[3 * i], c.colors[3 * i + 1], c.colors[3 * i + 2]);
    visma_io_free_cloud(&c);
    return true;
}

// feh::ICPRefinement (src/evaluation.cpp:258-271) from the down-sampling on:
// scene = VoxelDownSample(scene, voxel_size); RegistrationICP(scene_est, scene, ...).
inline RegistrationResult ICPRefinement(const PointCloud &scene_raw, const PointCloud &scene_est,
                                        const Eigen::Matrix4d &T_scene_src, double voxel_size,
                                        double max_distance, bool use_point_to_plane)
{
    if (!use_point_to_plane && voxel_size > 0.0 && max_distance > 0.0 && !scene_raw.points_.empty() &&
        !scene_est.points_.empty()) {
        // the scene goes up once, is down-sampled on the device and becomes the target where it lies
        // (visma_icp_set_clouds_f64_voxel_target): the down-sampled cloud never crosses PCIe.  The result is the
        // one of the two separate steps below; its correspondence_set_ indexes the voxels in ascending order.
        visma_icp_ctx *ctx = detail::ThreadContext::instance().get();
        int64_t nt = 0;
        detail::check(ctx, visma_icp_set_clouds_f64_voxel_target(ctx, detail::xyz(scene_est.points_), (int64_t)scene_est.points_.size(), 3,
                                                                 detail::xyz(scene_raw.points_), (int64_t)scene_raw.points_.size(), 3,
                                                                 voxel_size, &nt),
                      "visma_icp_set_clouds_f64_voxel_target");
        const ICPConvergenceCriteria c;
        double T[16];
        detail::to_rowmajor(T_scene_src, T);
        visma_icp_result r;
        detail::check(ctx, visma_icp_run(ctx, T, max_distance, c.max_iteration_, c.relative_fitness_, c.relative_rmse_,
                                         VISMA_ICP_SOLVER_KABSCH, 0, &r), "visma_icp_run");
        RegistrationResult result(T_scene_src);
        detail::fill_result(ctx, r, scene_est.points_.size(), result);
        return result;
    }
    const std::shared_ptr<PointCloud> scene = cicp::VoxelDownSample(scene_raw, voxel_size);
    if (use_point_to_plane)
        return cicp::RegistrationICP(scene_est, *scene, max_distance, T_scene_src,
                                     TransformationEstimationPointToPlane());
    return cicp::RegistrationICP(scene_est, *scene, max_distance, T_scene_src);
}

// The registration call alone (scene already down-sampled by the caller).
inline RegistrationResult ICPRefinement(const PointCloud &scene, const PointCloud &scene_est,
                                        const Eigen::Matrix4d &T_scene_src, double max_distance,
                                        bool use_point_to_plane)
{
    if (use_point_to_plane)
        return cicp::RegistrationICP(scene_est, scene, max_distance, T_scene_src,
                               TransformationEstimationPointToPlane());
    return cicp::RegistrationICP(scene_est, scene, max_distance, T_scene_src);
}

// ---- 4DoF estimator methods (explicit-correspondence entry points) ----------
inline double TransformationEstimationPointToPoint4DoF::ComputeRMSE(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_rmse_point_to_point(source, target, corres);
}

inline Eigen::Matrix4d TransformationEstimationPointToPoint4DoF::ComputeTransformation(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_update(source, target, corres, false, with_scaling_);
}

inline double TransformationEstimationPointToPointTrimmed::ComputeRMSE(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_rmse_point_to_point(source, target, corres);
}

inline Eigen::Matrix4d TransformationEstimationPointToPointTrimmed::ComputeTransformation(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_update(source, target, corres, false, false);
}

inline double TransformationEstimationPointToPointRobust::ComputeRMSE(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_rmse_point_to_point(source, target, corres);
}

inline Eigen::Matrix4d TransformationEstimationPointToPointRobust::ComputeTransformation(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_update(source, target, corres, false, with_scaling_);
}

inline double TransformationEstimationPointToPlaneRobust::ComputeRMSE(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_rmse_point_to_plane(source, target, corres);
}

inline Eigen::Matrix4d TransformationEstimationPointToPlaneRobust::ComputeTransformation(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    if (!target.HasNormals()) return Eigen::Matrix4d::Identity();
    return detail::host_update(source, target, corres, true, false);
}

inline double TransformationEstimationGeneralized::ComputeRMSE(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    if (corres.empty() || !source.HasNormals() || !target.HasNormals()) return 0.0;
    double st[VISMA_ICP_NSTATS];
    return std::sqrt(detail::host_stats_gicp(source, target, corres, epsilon_, st) / (double)corres.size());
}

inline Eigen::Matrix4d TransformationEstimationGeneralized::ComputeTransformation(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    if (corres.empty() || !source.HasNormals() || !target.HasNormals()) return Eigen::Matrix4d::Identity();
    double st[VISMA_ICP_NSTATS], T[16];
    (void)detail::host_stats_gicp(source, target, corres, epsilon_, st);
    visma_icp_solve_from_stats(st, VISMA_ICP_SOLVER_GN_EULER, 0, T);
    return detail::from_rowmajor(T);
}

inline double TransformationEstimationForColoredICP::ComputeRMSE(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    if (corres.empty() || !target.HasNormals() || !target.HasColors() || !source.HasColors() ||
        color_gradient_.size() != target.points_.size())
        return 0.0;
    double st[VISMA_ICP_NSTATS];
    return detail::host_stats_colored(source, target, corres, color_gradient_, lambda_geometric_, st);
}

inline Eigen::Matrix4d TransformationEstimationForColoredICP::ComputeTransformation(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    if (corres.empty() || !target.HasNormals() || !target.HasColors() || !source.HasColors() ||
        color_gradient_.size() != target.points_.size())
        return Eigen::Matrix4d::Identity();
    double st[VISMA_ICP_NSTATS], T[16];
    (void)detail::host_stats_colored(source, target, corres, color_gradient_, lambda_geometric_, st);
    visma_icp_solve_from_stats(st, VISMA_ICP_SOLVER_GN_EULER, 0, T);
    return detail::from_rowmajor(T);
}

// ---- the estimators constrained to a rotation about up_ ----------------------
inline double TransformationEstimationPointToPointYaw::ComputeRMSE(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_rmse_point_to_point(source, target, corres);
}

inline Eigen::Matrix4d TransformationEstimationPointToPointYaw::ComputeTransformation(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_update_axis(source, target, corres, false, up_);
}

inline double TransformationEstimationPointToPlaneYaw::ComputeRMSE(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_rmse_point_to_plane(source, target, corres);
}

inline Eigen::Matrix4d TransformationEstimationPointToPlaneYaw::ComputeTransformation(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres) const
{
    return detail::host_update_axis(source, target, corres, true, up_);
}

// open3d::ComputeRGBDOdometry (Odometry.cpp:490-527) on the GPU: the odometry edge between two consecutive frames and its
// information matrix -> (success, the pose source camera -> target camera, the 6 x 6).  Both RGBDImages hold single-channel
// float images of one size (CreateRGBDImageFromColorAndDepth makes them); anything else gives (false, I, 0), as the
// reference's CheckRGBDImagePair does.  Without success: (false, I, 0) -- the reference returns I as the matrix there; the
// matrix is the pure sum (visma_icp.h: the deviations).  jacobian_method selects by its type: a
// RGBDOdometryJacobianFromColorTerm the colour term, anything else the hybrid term.
inline bool CheckRGBDImagePair(const RGBDImage &source, const RGBDImage &target)
{
    const Image *im[4] = {&source.color_, &source.depth_, &target.color_, &target.depth_};
    for (const Image *i : im)
        if (i->width_ != im[0]->width_ || i->height_ != im[0]->height_ || i->num_of_channels_ != 1 || i->bytes_per_channel_ != 4 ||
            !i->HasData()) return false;
    return true;
}

// ... on a context of the caller's
inline std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d> ComputeRGBDOdometry(
        visma_icp_ctx *ctx, const RGBDImage &source, const RGBDImage &target, const PinholeCameraIntrinsic &pinhole_camera_intrinsic,
        const Eigen::Matrix4d &odo_init = Eigen::Matrix4d::Identity(),
        const RGBDOdometryJacobian &jacobian_method = RGBDOdometryJacobianFromHybridTerm(), const OdometryOption &option = OdometryOption())
{
    typedef std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d> Out;
    const Out failed(false, Eigen::Matrix4d::Identity(), Eigen::Matrix6d::Zero());
    if (!CheckRGBDImagePair(source, target)) return failed;
    visma_icp_odometry_option opt;
    visma_icp_odometry_option_default(&opt);
    opt.n_levels = (int)option.iteration_number_per_pyramid_level_.size();
    for (int l = 0; l < opt.n_levels && l < VISMA_ICP_ODOMETRY_MAX_LEVELS; l++) opt.iterations[l] = option.iteration_number_per_pyramid_level_[l];
    opt.max_depth_diff = option.max_depth_diff_; opt.min_depth = option.min_depth_; opt.max_depth = option.max_depth_;
    const Eigen::Matrix3d &K = pinhole_camera_intrinsic.intrinsic_matrix_;
    const double k[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    const int method = typeid(jacobian_method) == typeid(RGBDOdometryJacobianFromColorTerm) ? VISMA_ICP_ODOMETRY_COLOR : VISMA_ICP_ODOMETRY_HYBRID;
    double init[16], T[16], info[36];
    detail::to_rowmajor(odo_init, init);
    visma_icp_odometry_result res = {};
    detail::check(ctx, visma_icp_rgbd_odometry(ctx, source.color_.width_, source.color_.height_, (const float *)source.color_.data_.data(),
                                               (const float *)source.depth_.data_.data(), (const float *)target.color_.data_.data(),
                                               (const float *)target.depth_.data_.data(), k, init, method, &opt, T, info, &res),
                  "visma_icp_rgbd_odometry");
    if (!res.success) return failed;
    Eigen::Matrix4d Tm;
    Eigen::Matrix6d Im;
    for (int i = 0; i < 16; i++) Tm(i / 4, i % 4) = T[i];
    for (int i = 0; i < 36; i++) Im(i / 6, i % 6) = info[i];
    return Out(true, Tm, Im);
}

// ... on this thread's context
inline std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d> ComputeRGBDOdometry(
        const RGBDImage &source, const RGBDImage &target, const PinholeCameraIntrinsic &pinhole_camera_intrinsic,
        const Eigen::Matrix4d &odo_init = Eigen::Matrix4d::Identity(),
        const RGBDOdometryJacobian &jacobian_method = RGBDOdometryJacobianFromHybridTerm(), const OdometryOption &option = OdometryOption())
{
    if (!CheckRGBDImagePair(source, target))                          // (before a context is made)
        return std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d>(false, Eigen::Matrix4d::Identity(), Eigen::Matrix6d::Zero());
    return ComputeRGBDOdometry(detail::ThreadContext::instance().get(), source, target, pinhole_camera_intrinsic, odo_init, jacobian_method, option);
}

// open3d::CreatePointCloudFromDepthImage / CreatePointCloudFromRGBDImage (PointCloudFactory.cpp) on the GPU.  A 16-bit depth
// image is converted on the host first (ConvertDepthToFloatImage); any other format gives an empty cloud, as the reference.
namespace detail {
inline std::shared_ptr<PointCloud> cloud_from_frame(visma_icp_ctx *ctx, const Image &depth, const Image *color, int color_type,
                                                    const PinholeCameraIntrinsic &intrinsic, const Eigen::Matrix4d &extrinsic, int stride)
{
    auto out = std::make_shared<PointCloud>();
    const Eigen::Matrix3d &K = intrinsic.intrinsic_matrix_;
    const double k[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    double E[16];
    to_rowmajor(extrinsic, E);
    const int w = depth.width_, h = depth.height_;
    if (w < 1 || h < 1 || stride < 1) return out;
    const int64_t cap = (((int64_t)w - 1) / stride + 1) * (((int64_t)h - 1) / stride + 1);
    std::vector<double> pts(3 * (size_t)cap), col(color ? 3 * (size_t)cap : 0);
    int64_t n = 0;
    if (color)
        check(ctx, visma_icp_point_cloud_from_rgbd(ctx, w, h, (const float *)depth.data_.data(), color->data_.data(), color_type, k, E,
                                                   pts.data(), col.data(), cap, &n), "visma_icp_point_cloud_from_rgbd");
    else
        check(ctx, visma_icp_point_cloud_from_depth(ctx, w, h, (const float *)depth.data_.data(), k, E, stride, pts.data(), cap, &n),
              "visma_icp_point_cloud_from_depth");
    out->points_.resize((size_t)n);
    for (size_t i = 0; i < (size_t)n; i++) out->points_[i] = Eigen::Vector3d(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    if (color) {
        out->colors_.resize((size_t)n);
        for (size_t i = 0; i < (size_t)n; i++) out->colors_[i] = Eigen::Vector3d(col[3 * i], col[3 * i + 1], col[3 * i + 2]);
    }
    return out;
}
}  // namespace detail

// what open3d::UniformTSDFVolume and ScalableTSDFVolume share (stand-alone header set): a volume of the context by its handle
namespace detail {
inline void tsdf_integrate(visma_icp_ctx *ctx, visma_icp_tsdf *volume, int color_type, const char *who, const RGBDImage &image,
                           const PinholeCameraIntrinsic &intrinsic, const Eigen::Matrix4d &extrinsic)
{
    const Image &d = image.depth_, &c = image.color_;
    const bool rgb = color_type == VISMA_ICP_TSDF_COLOR_RGB8, gray = color_type == VISMA_ICP_TSDF_COLOR_GRAY32;
    if (d.num_of_channels_ != 1 || d.bytes_per_channel_ != 4 || !d.HasData() || (rgb && (c.num_of_channels_ != 3 || c.bytes_per_channel_ != 1)) ||
        (gray && (c.num_of_channels_ != 1 || c.bytes_per_channel_ != 4)) ||
        ((rgb || gray) && (c.width_ != d.width_ || c.height_ != d.height_ || !c.HasData())))
        throw std::invalid_argument(std::string(who) + "Unsupported image format.");
    const Eigen::Matrix3d &K = intrinsic.intrinsic_matrix_;
    const double k[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    double E[16];
    to_rowmajor(extrinsic, E);
    const int rc = visma_icp_tsdf_integrate(ctx, volume, d.width_, d.height_, (const float *)d.data_.data(),
                                            (rgb || gray) ? (const void *)c.data_.data() : nullptr, k, intrinsic.width_, intrinsic.height_, E);
    if (rc == VISMA_ICP_ERR_INVALID) throw std::invalid_argument(std::string(who) + visma_icp_last_error(ctx));
    check(ctx, rc, "visma_icp_tsdf_integrate");
}
inline std::shared_ptr<PointCloud> tsdf_extract_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume, bool colored)
{
    auto out = std::make_shared<PointCloud>();
    int64_t n = 0;
    check(ctx, visma_icp_tsdf_extract_point_cloud(ctx, volume, &n), "visma_icp_tsdf_extract_point_cloud");
    out->points_.resize((size_t)n); out->normals_.resize((size_t)n); out->colors_.resize(colored ? (size_t)n : 0);
    // (std::vector<Eigen::Vector3d> is contiguous AoS f64 with stride 3)
    check(ctx, visma_icp_tsdf_get_point_cloud(ctx, volume, n ? out->points_[0].data() : nullptr, n ? out->normals_[0].data() : nullptr,
                                              colored && n ? out->colors_[0].data() : nullptr, n), "visma_icp_tsdf_get_point_cloud");
    return out;
}
inline std::shared_ptr<PointCloud> tsdf_extract_voxel_point_cloud(visma_icp_ctx *ctx, visma_icp_tsdf *volume)
{
    auto out = std::make_shared<PointCloud>();
    int64_t n = 0;
    check(ctx, visma_icp_tsdf_extract_voxel_point_cloud(ctx, volume, &n), "visma_icp_tsdf_extract_voxel_point_cloud");
    out->points_.resize((size_t)n); out->colors_.resize((size_t)n);
    check(ctx, visma_icp_tsdf_get_voxel_point_cloud(ctx, volume, n ? out->points_[0].data() : nullptr, n ? out->colors_[0].data() : nullptr, n),
          "visma_icp_tsdf_get_voxel_point_cloud");
    return out;
}
inline std::shared_ptr<TriangleMesh> tsdf_extract_triangle_mesh(visma_icp_ctx *ctx, visma_icp_tsdf *volume, bool colored)
{
    auto out = std::make_shared<TriangleMesh>();
    int64_t nv = 0, nt = 0;
    check(ctx, visma_icp_tsdf_extract_triangle_mesh(ctx, volume, &nv, &nt), "visma_icp_tsdf_extract_triangle_mesh");
    out->vertices_.resize((size_t)nv); out->vertex_colors_.resize(colored ? (size_t)nv : 0);
    std::vector<int32_t> tri(3 * (size_t)nt);
    check(ctx, visma_icp_tsdf_get_triangle_mesh(ctx, volume, nv ? out->vertices_[0].data() : nullptr,
                                                colored && nv ? out->vertex_colors_[0].data() : nullptr, nt ? tri.data() : nullptr, nv, nt),
          "visma_icp_tsdf_get_triangle_mesh");
    out->triangles_.resize((size_t)nt);
    for (size_t i = 0; i < (size_t)nt; i++) out->triangles_[i] = Eigen::Vector3i(tri[3 * i], tri[3 * i + 1], tri[3 * i + 2]);
    return out;
}
inline void tsdf_download(visma_icp_ctx *ctx, visma_icp_tsdf *volume, const int32_t *unit, size_t voxels, bool colored, std::vector<float> &tsdf,
                          std::vector<float> &weight, std::vector<Eigen::Vector3f> &color)
{
    tsdf.assign(voxels, 0.0f); weight.assign(voxels, 0.0f);
    std::vector<float> c(colored ? 3 * voxels : 0);
    check(ctx, visma_icp_tsdf_get_volume(ctx, volume, unit, tsdf.data(), weight.data(), colored ? c.data() : nullptr), "visma_icp_tsdf_get_volume");
    color.resize(colored ? voxels : 0);
    for (size_t i = 0; i < color.size(); i++) color[i] = Eigen::Vector3f(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
}
}  // namespace detail

// ... on a context of the caller's
inline std::shared_ptr<PointCloud> CreatePointCloudFromDepthImage(visma_icp_ctx *ctx, const Image &depth, const PinholeCameraIntrinsic &intrinsic,
                                                                  const Eigen::Matrix4d &extrinsic = Eigen::Matrix4d::Identity(),
                                                                  double depth_scale = 1000.0, double depth_trunc = 1000.0, int stride = 1)
{
    if (depth.num_of_channels_ == 1 && depth.bytes_per_channel_ == 2 && depth.HasData())
        return detail::cloud_from_frame(ctx, *ConvertDepthToFloatImage(depth, depth_scale, depth_trunc), nullptr, 0, intrinsic, extrinsic, stride);
    if (depth.num_of_channels_ == 1 && depth.bytes_per_channel_ == 4 && depth.HasData())
        return detail::cloud_from_frame(ctx, depth, nullptr, 0, intrinsic, extrinsic, stride);
    return std::make_shared<PointCloud>();
}
inline std::shared_ptr<PointCloud> CreatePointCloudFromRGBDImage(visma_icp_ctx *ctx, const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic,
                                                                 const Eigen::Matrix4d &extrinsic = Eigen::Matrix4d::Identity())
{
    const Image &d = image.depth_, &c = image.color_;
    if (d.num_of_channels_ == 1 && d.bytes_per_channel_ == 4 && d.HasData() && c.HasData() && c.width_ == d.width_ && c.height_ == d.height_) {
        if (c.bytes_per_channel_ == 1 && c.num_of_channels_ == 3)
            return detail::cloud_from_frame(ctx, d, &c, VISMA_ICP_TSDF_COLOR_RGB8, intrinsic, extrinsic, 1);
        if (c.bytes_per_channel_ == 4 && c.num_of_channels_ == 1)
            return detail::cloud_from_frame(ctx, d, &c, VISMA_ICP_TSDF_COLOR_GRAY32, intrinsic, extrinsic, 1);
    }
    return std::make_shared<PointCloud>();
}
// ... on this thread's context
inline std::shared_ptr<PointCloud> CreatePointCloudFromDepthImage(const Image &depth, const PinholeCameraIntrinsic &intrinsic,
                                                                  const Eigen::Matrix4d &extrinsic = Eigen::Matrix4d::Identity(),
                                                                  double depth_scale = 1000.0, double depth_trunc = 1000.0, int stride = 1)
{
    return CreatePointCloudFromDepthImage(detail::ThreadContext::instance().get(), depth, intrinsic, extrinsic, depth_scale, depth_trunc, stride);
}
inline std::shared_ptr<PointCloud> CreatePointCloudFromRGBDImage(const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic,
                                                                 const Eigen::Matrix4d &extrinsic = Eigen::Matrix4d::Identity())
{
    return CreatePointCloudFromRGBDImage(detail::ThreadContext::instance().get(), image, intrinsic, extrinsic);
}

#ifdef VISMA_ICP_STANDALONE_OPEN3D_TYPES
// open3d::ColorMapOptimization (ColorMapOptimization.cpp, rigid) on the GPU: the one-call entry point of visma_icp.h.  The
// non-rigid option and an image that is not float depth + RGB8 of the intrinsic's size throw std::invalid_argument.
// The NON-RIGID optimization (a warping field per image) is ColorMapOptimizationNonRigid, below: it reads the anchors and
// the weight from the option, whatever the option's flag says.
namespace detail {
inline void color_map_optimization(visma_icp_ctx *ctx, const std::vector<Eigen::Vector3d> &vertices, std::vector<Eigen::Vector3d> &colors,
                                   const std::vector<RGBDImage> &images, PinholeCameraTrajectory &camera,
                                   const ColorMapOptmizationOption &option, bool non_rigid = false)
{
    const char *who = non_rigid ? "[ColorMapOptimizationNonRigid] " : "[ColorMapOptimization] ";
    if (!non_rigid && option.non_rigid_camera_coordinate_)
        throw std::invalid_argument(std::string(who) + "non_rigid_camera_coordinate_ is set: call ColorMapOptimizationNonRigid.");
    const size_t n = images.size();
    if (n == 0 || camera.extrinsic_.size() != n) throw std::invalid_argument(std::string(who) + "one extrinsic per image, at least one.");
    const int w = images[0].depth_.width_, h = images[0].depth_.height_;
    std::vector<float> depth(n * (size_t)w * h);
    std::vector<uint8_t> color(n * (size_t)w * h * 3);
    std::vector<double> E(n * 16);
    for (size_t i = 0; i < n; i++) {
        const Image &d = images[i].depth_, &c = images[i].color_;
        if (d.width_ != w || d.height_ != h || c.width_ != w || c.height_ != h || d.num_of_channels_ != 1 || d.bytes_per_channel_ != 4 ||
            c.num_of_channels_ != 3 || c.bytes_per_channel_ != 1 || !d.HasData() || !c.HasData())
            throw std::invalid_argument(std::string(who) + "Unsupported image format.");
        std::memcpy(depth.data() + i * (size_t)w * h, d.data_.data(), (size_t)w * h * 4);
        std::memcpy(color.data() + i * (size_t)w * h * 3, c.data_.data(), (size_t)w * h * 3);
        to_rowmajor(camera.extrinsic_[i], E.data() + 16 * i);
    }
    const Eigen::Matrix3d &K = camera.intrinsic_.intrinsic_matrix_;
    const double k[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    visma_icp_color_map_option o;
    visma_icp_color_map_option_default(&o);
    o.number_of_vertical_anchors = option.number_of_vertical_anchors_;
    o.non_rigid_anchor_point_weight = option.non_rigid_anchor_point_weight_;
    o.maximum_iteration = option.maximum_iteration_;
    o.maximum_allowable_depth = option.maximum_allowable_depth_;
    o.depth_threshold_for_visiblity_check = option.depth_threshold_for_visiblity_check_;
    o.depth_threshold_for_discontinuity_check = option.depth_threshold_for_discontinuity_check_;
    o.half_dilation_kernel_size_for_discontinuity_map = option.half_dilation_kernel_size_for_discontinuity_map_;
    colors.assign(vertices.size(), Eigen::Vector3d::Zero());
    // (std::vector<Eigen::Vector3d> is contiguous AoS f64 with stride 3)
    const double *vp = vertices.empty() ? nullptr : vertices[0].data();
    double *cp = colors.empty() ? nullptr : colors[0].data();
    const int rc = non_rigid ? visma_icp_color_map_optimization_non_rigid(ctx, w, h, (int)n, k, depth.data(), color.data(), E.data(), vp,
                                                                          (int64_t)vertices.size(), &o, cp, nullptr)
                             : visma_icp_color_map_optimization(ctx, w, h, (int)n, k, depth.data(), color.data(), E.data(), vp,
                                                                (int64_t)vertices.size(), &o, cp);
    if (rc == VISMA_ICP_ERR_INVALID) throw std::invalid_argument(std::string(who) + visma_icp_last_error(ctx));
    check(ctx, rc, non_rigid ? "visma_icp_color_map_optimization_non_rigid" : "visma_icp_color_map_optimization");
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 16; a++) camera.extrinsic_[i](a / 4, a % 4) = E[16 * i + (size_t)a];
}
}  // namespace detail

// ... on a context of the caller's
inline void ColorMapOptimization(visma_icp_ctx *ctx, TriangleMesh &mesh, const std::vector<RGBDImage> &images_rgbd,
                                 PinholeCameraTrajectory &camera, const ColorMapOptmizationOption &option = ColorMapOptmizationOption())
{
    detail::color_map_optimization(ctx, mesh.vertices_, mesh.vertex_colors_, images_rgbd, camera, option);
}
// ... on the points of a cloud (what ExtractPointCloud gives): colors_ is written
inline void ColorMapOptimization(visma_icp_ctx *ctx, PointCloud &cloud, const std::vector<RGBDImage> &images_rgbd,
                                 PinholeCameraTrajectory &camera, const ColorMapOptmizationOption &option = ColorMapOptmizationOption())
{
    detail::color_map_optimization(ctx, cloud.points_, cloud.colors_, images_rgbd, camera, option);
}
// ... on this thread's context
inline void ColorMapOptimization(TriangleMesh &mesh, const std::vector<RGBDImage> &images_rgbd, PinholeCameraTrajectory &camera,
                                 const ColorMapOptmizationOption &option = ColorMapOptmizationOption())
{
    ColorMapOptimization(detail::ThreadContext::instance().get(), mesh, images_rgbd, camera, option);
}
inline void ColorMapOptimization(PointCloud &cloud, const std::vector<RGBDImage> &images_rgbd, PinholeCameraTrajectory &camera,
                                 const ColorMapOptmizationOption &option = ColorMapOptmizationOption())
{
    ColorMapOptimization(detail::ThreadContext::instance().get(), cloud, images_rgbd, camera, option);
}

// The non-rigid optimization (OptimizeImageCoorNonrigid; visma_icp.h states its deviations): number_of_vertical_anchors_
// and non_rigid_anchor_point_weight_ are read from the option whatever non_rigid_camera_coordinate_ says.  The fields
// themselves stay inside, as in the reference; the staged calls of visma_icp.h hand them out.
inline void ColorMapOptimizationNonRigid(visma_icp_ctx *ctx, TriangleMesh &mesh, const std::vector<RGBDImage> &images_rgbd,
                                         PinholeCameraTrajectory &camera, const ColorMapOptmizationOption &option = ColorMapOptmizationOption())
{
    detail::color_map_optimization(ctx, mesh.vertices_, mesh.vertex_colors_, images_rgbd, camera, option, true);
}
inline void ColorMapOptimizationNonRigid(visma_icp_ctx *ctx, PointCloud &cloud, const std::vector<RGBDImage> &images_rgbd,
                                         PinholeCameraTrajectory &camera, const ColorMapOptmizationOption &option = ColorMapOptmizationOption())
{
    detail::color_map_optimization(ctx, cloud.points_, cloud.colors_, images_rgbd, camera, option, true);
}
inline void ColorMapOptimizationNonRigid(TriangleMesh &mesh, const std::vector<RGBDImage> &images_rgbd, PinholeCameraTrajectory &camera,
                                         const ColorMapOptmizationOption &option = ColorMapOptmizationOption())
{
    ColorMapOptimizationNonRigid(detail::ThreadContext::instance().get(), mesh, images_rgbd, camera, option);
}
inline void ColorMapOptimizationNonRigid(PointCloud &cloud, const std::vector<RGBDImage> &images_rgbd, PinholeCameraTrajectory &camera,
                                         const ColorMapOptmizationOption &option = ColorMapOptmizationOption())
{
    ColorMapOptimizationNonRigid(detail::ThreadContext::instance().get(), cloud, images_rgbd, camera, option);
}
#endif

#ifdef VISMA_ICP_STANDALONE_OPEN3D_TYPES
// ---- open3d::KDTreeFlann for MANY queries in one call (visma_icp.h, "KDTreeFlann") ----
// A KDTreeFlann::Search is a launch and a round trip per query; these take every query at once and return flat arrays.
// KNN / Hybrid: indices and distance2 are queries.size() x knn (max_nn), row i padded with -1 and +inf behind its counts[i]
// entries.  Returns the number of queries, or -1 as the class does (an empty tree, knn or max_nn < 0); knn or max_nn = 0,
// and for Hybrid a radius of 0 or one that is not finite: rows of no entries.
namespace detail {
inline int kdtree_search_lists(const KDTreeFlann &tree, bool knn, const std::vector<Eigen::Vector3d> &queries, double radius, int cap,
                               std::vector<int> &indices, std::vector<double> &distance2, std::vector<int> &counts)
{
    static_assert(sizeof(int) == sizeof(int32_t), "the index arrays are handed to the C ABI as they are");
    if (!tree.handle() || cap < 0) return -1;
    const size_t nq = queries.size();
    indices.assign(nq * (size_t)cap, -1);
    distance2.assign(nq * (size_t)cap, std::numeric_limits<double>::infinity());
    counts.assign(nq, 0);
    radius = std::fabs(radius);                                     // (the reference squares it)
    if (nq == 0 || cap == 0 || (!knn && !(radius > 0.0 && std::isfinite(radius)))) return (int)nq;
    if (knn)
        check(tree.context(), visma_icp_kdtree_search_knn(tree.handle(), xyz(queries), (int64_t)nq, cap, indices.data(), distance2.data(), counts.data()),
              "visma_icp_kdtree_search_knn");
    else
        check(tree.context(), visma_icp_kdtree_search_hybrid(tree.handle(), xyz(queries), (int64_t)nq, radius, cap, indices.data(), distance2.data(),
                                                             counts.data()),
              "visma_icp_kdtree_search_hybrid");
    return (int)nq;
}
}  // namespace detail
inline int KDTreeSearchKNN(const KDTreeFlann &tree, const std::vector<Eigen::Vector3d> &queries, int knn, std::vector<int> &indices,
                           std::vector<double> &distance2, std::vector<int> &counts)
{
    return detail::kdtree_search_lists(tree, true, queries, 0.0, knn, indices, distance2, counts);
}
inline int KDTreeSearchHybrid(const KDTreeFlann &tree, const std::vector<Eigen::Vector3d> &queries, double radius, int max_nn,
                              std::vector<int> &indices, std::vector<double> &distance2, std::vector<int> &counts)
{
    return detail::kdtree_search_lists(tree, false, queries, radius, max_nn, indices, distance2, counts);
}
// Radius: CSR -- query i owns [offsets[i], offsets[i + 1]) of indices and distance2, offsets has queries.size() + 1 entries.
// Returns the number of queries, or -1 for an empty tree; a radius of 0 or one that is not finite: no entries.
inline int KDTreeSearchRadius(const KDTreeFlann &tree, const std::vector<Eigen::Vector3d> &queries, double radius,
                              std::vector<int64_t> &offsets, std::vector<int> &indices, std::vector<double> &distance2)
{
    if (!tree.handle()) return -1;
    const size_t nq = queries.size();
    offsets.assign(nq + 1, 0);
    indices.clear();
    distance2.clear();
    radius = std::fabs(radius);
    if (nq == 0 || !(radius > 0.0 && std::isfinite(radius))) return (int)nq;
    int64_t total = 0;
    detail::check(tree.context(), visma_icp_kdtree_search_radius(tree.handle(), detail::xyz(queries), (int64_t)nq, radius, offsets.data(), &total),
                  "visma_icp_kdtree_search_radius");
    indices.resize((size_t)total);
    distance2.resize((size_t)total);
    detail::check(tree.context(), visma_icp_kdtree_get_radius_result(tree.handle(), indices.data(), distance2.data()),
                  "visma_icp_kdtree_get_radius_result");
    return (int)nq;
}

// ---- open3d::TriangleMesh on the GPU (visma_icp.h, "TriangleMesh") ----
// DeviceTriangleMesh: a mesh resident on the device, for a chain of steps with one upload and one download -- or none: the
// mesh a TSDF volume extracted is taken where it lies (FromVolume).  The members of open3d::TriangleMesh and the free
// functions below are one such chain each.  An index outside [0, vertices) throws std::runtime_error.
class DeviceTriangleMesh {
public:
    DeviceTriangleMesh(visma_icp_ctx *ctx, const TriangleMesh &mesh) : ctx_(ctx)
    {
        const size_t nv = mesh.vertices_.size(), nt = mesh.triangles_.size();
        static_assert(sizeof(Eigen::Vector3i) == 3 * sizeof(int32_t), "triangles are uploaded as they lie");
        detail::check(ctx_, visma_icp_trimesh_create(ctx_, detail::xyz(mesh.vertices_), (int64_t)nv,
                                                     mesh.HasVertexNormals() ? detail::xyz(mesh.vertex_normals_) : nullptr,
                                                     mesh.HasVertexColors() ? detail::xyz(mesh.vertex_colors_) : nullptr,
                                                     nt ? mesh.triangles_[0].data() : nullptr, (int64_t)nt,
                                                     mesh.HasTriangleNormals() ? detail::xyz(mesh.triangle_normals_) : nullptr, &mesh_),
                      "visma_icp_trimesh_create");
    }
    explicit DeviceTriangleMesh(const TriangleMesh &mesh) : DeviceTriangleMesh(detail::ThreadContext::instance().get(), mesh) {}
    // the volume's last extracted mesh, copied device to device (ExtractTriangleMesh first: cicp::ExtractTriangleMesh does both)
    static DeviceTriangleMesh FromVolume(const TSDFVolume &volume)
    {
        DeviceTriangleMesh m(volume.Context(), nullptr);
        detail::check(m.ctx_, visma_icp_trimesh_from_tsdf(m.ctx_, volume.Handle(), &m.mesh_), "visma_icp_trimesh_from_tsdf");
        return m;
    }
    ~DeviceTriangleMesh() { if (mesh_) (void)visma_icp_trimesh_destroy(ctx_, mesh_); }
    DeviceTriangleMesh(DeviceTriangleMesh &&o) noexcept : ctx_(o.ctx_), mesh_(o.mesh_) { o.mesh_ = nullptr; }
    DeviceTriangleMesh(const DeviceTriangleMesh &) = delete;
    DeviceTriangleMesh &operator=(const DeviceTriangleMesh &) = delete;

    void NormalizeNormals() { detail::check(ctx_, visma_icp_trimesh_normalize_normals(ctx_, mesh_), "visma_icp_trimesh_normalize_normals"); }
    void ComputeTriangleNormals(bool normalized = true)
    {
        detail::check(ctx_, visma_icp_trimesh_compute_triangle_normals(ctx_, mesh_, normalized), "visma_icp_trimesh_compute_triangle_normals");
    }
    void ComputeVertexNormals(bool normalized = true)
    {
        detail::check(ctx_, visma_icp_trimesh_compute_vertex_normals(ctx_, mesh_, normalized), "visma_icp_trimesh_compute_vertex_normals");
    }
    void Transform(const Eigen::Matrix4d &T)
    {
        double t[16];
        for (int i = 0; i < 16; i++) t[i] = T(i / 4, i % 4);          // (either storage order)
        detail::check(ctx_, visma_icp_trimesh_transform(ctx_, mesh_, t), "visma_icp_trimesh_transform");
    }
    // -> the rows Purge's four steps removed
    std::vector<int64_t> Purge()
    {
        std::vector<int64_t> removed(4, 0);
        detail::check(ctx_, visma_icp_trimesh_purge(ctx_, mesh_, removed.data()), "visma_icp_trimesh_purge");
        return removed;
    }
    DeviceTriangleMesh Select(const std::vector<size_t> &indices) const
    {
        const std::vector<int64_t> idx(indices.begin(), indices.end());
        DeviceTriangleMesh out(ctx_, nullptr);
        detail::check(ctx_, visma_icp_trimesh_select(ctx_, mesh_, idx.data(), (int64_t)idx.size(), &out.mesh_), "visma_icp_trimesh_select");
        return out;
    }
    DeviceTriangleMesh Crop(const Eigen::Vector3d &min_bound, const Eigen::Vector3d &max_bound) const
    {
        DeviceTriangleMesh out(ctx_, nullptr);
        detail::check(ctx_, visma_icp_trimesh_crop(ctx_, mesh_, min_bound.data(), max_bound.data(), &out.mesh_), "visma_icp_trimesh_crop");
        return out;
    }
    // the device's rows into `mesh`: every attribute the device mesh has; one it does not have is left as it is where
    // keep_others (what the reference's in-place members do to arrays that do not fit the mesh), else cleared
    void Download(TriangleMesh &mesh, bool keep_others = false) const
    {
        int64_t nv = 0, nt = 0;
        int has = 0;
        detail::check(ctx_, visma_icp_trimesh_size(mesh_, &nv, &nt, &has), "visma_icp_trimesh_size");
        const bool vn = has & VISMA_ICP_TRIMESH_HAS_VERTEX_NORMALS, vc = has & VISMA_ICP_TRIMESH_HAS_VERTEX_COLORS,
                   tn = has & VISMA_ICP_TRIMESH_HAS_TRIANGLE_NORMALS;
        mesh.vertices_.resize((size_t)nv);
        mesh.triangles_.resize((size_t)nt);
        if (vn) mesh.vertex_normals_.resize((size_t)nv); else if (!keep_others) mesh.vertex_normals_.clear();
        if (vc) mesh.vertex_colors_.resize((size_t)nv); else if (!keep_others) mesh.vertex_colors_.clear();
        if (tn) mesh.triangle_normals_.resize((size_t)nt); else if (!keep_others) mesh.triangle_normals_.clear();
        detail::check(ctx_, visma_icp_trimesh_get(ctx_, mesh_, nv ? mesh.vertices_[0].data() : nullptr, vn ? mesh.vertex_normals_[0].data() : nullptr,
                                                  vc ? mesh.vertex_colors_[0].data() : nullptr, nt ? mesh.triangles_[0].data() : nullptr,
                                                  tn ? mesh.triangle_normals_[0].data() : nullptr, nv, nt),
                      "visma_icp_trimesh_get");
    }
    std::shared_ptr<TriangleMesh> Download() const
    {
        auto out = std::make_shared<TriangleMesh>();
        Download(*out);
        return out;
    }
    visma_icp_ctx *context() const { return ctx_; }
    visma_icp_trimesh *handle() const { return mesh_; }

private:
    DeviceTriangleMesh(visma_icp_ctx *ctx, std::nullptr_t) : ctx_(ctx) {}
    visma_icp_ctx *ctx_ = nullptr;
    visma_icp_trimesh *mesh_ = nullptr;
};

namespace detail {
// rows that are no attribute of a consistent mesh (the reference's NormalizeNormals and Transform walk vertex_normals_ and
// triangle_normals_ whatever their sizes): as the vertex normals of a mesh of as many vertices and no triangle
template <class Op>
inline void trimesh_normal_rows(visma_icp_ctx *ctx, std::vector<Eigen::Vector3d> &rows, Op op)
{
    if (rows.empty()) return;
    TriangleMesh carrier;
    carrier.vertices_ = rows;
    carrier.vertex_normals_ = rows;
    DeviceTriangleMesh d(ctx, carrier);
    op(d);
    d.Download(carrier);
    rows = carrier.vertex_normals_;
}
// the whole mesh through one step on the device; normals whose size does not fit the mesh go through `rows_op` on their own
template <class Op>
inline void trimesh_in_place(visma_icp_ctx *ctx, TriangleMesh &mesh, bool normals_too, Op op)
{
    const bool had_vn = mesh.HasVertexNormals(), had_vc = mesh.HasVertexColors(), had_tn = mesh.HasTriangleNormals();
    const bool loose_vn = normals_too && !had_vn, loose_tn = normals_too && !had_tn;
    DeviceTriangleMesh d(ctx, mesh);
    op(d);
    d.Download(mesh, true);
    // (an attribute the mesh had shrinks with it, to no rows too)
    if (had_vn && !mesh.HasVertexNormals()) mesh.vertex_normals_.resize(mesh.vertices_.size());
    if (had_vc && !mesh.HasVertexColors()) mesh.vertex_colors_.resize(mesh.vertices_.size());
    if (had_tn && !mesh.HasTriangleNormals()) mesh.triangle_normals_.resize(mesh.triangles_.size());
    if (loose_vn) trimesh_normal_rows(ctx, mesh.vertex_normals_, op);
    if (loose_tn) trimesh_normal_rows(ctx, mesh.triangle_normals_, op);
}
}  // namespace detail

// the members of open3d::TriangleMesh on a context of the caller's
inline void NormalizeNormals(visma_icp_ctx *ctx, TriangleMesh &mesh)
{
    detail::trimesh_in_place(ctx, mesh, true, [](DeviceTriangleMesh &d) { d.NormalizeNormals(); });
}
inline void Transform(visma_icp_ctx *ctx, TriangleMesh &mesh, const Eigen::Matrix4d &T)
{
    detail::trimesh_in_place(ctx, mesh, true, [&T](DeviceTriangleMesh &d) { d.Transform(T); });
}
inline void ComputeTriangleNormals(visma_icp_ctx *ctx, TriangleMesh &mesh, bool normalized = true)
{
    // (TriangleMesh.cpp:148: the normals are resized, then every row is written; vertex normals that do not fit the mesh are
    //  normalised all the same)
    const bool loose_vn = normalized && !mesh.HasVertexNormals();
    mesh.triangle_normals_.clear();
    detail::trimesh_in_place(ctx, mesh, false, [normalized](DeviceTriangleMesh &d) { d.ComputeTriangleNormals(normalized); });
    if (!mesh.HasTriangleNormals()) mesh.triangle_normals_.resize(mesh.triangles_.size());      // (a mesh without vertices)
    if (loose_vn) detail::trimesh_normal_rows(ctx, mesh.vertex_normals_, [](DeviceTriangleMesh &d) { d.NormalizeNormals(); });
}
inline void ComputeVertexNormals(visma_icp_ctx *ctx, TriangleMesh &mesh, bool normalized = true)
{
    // (TriangleMesh.cpp:162-165: triangle normals that fit are used as they are; resize(n, Zero) keeps the rows that exist)
    if (!mesh.HasTriangleNormals()) mesh.triangle_normals_.clear();
    mesh.vertex_normals_.resize(mesh.vertices_.size(), Eigen::Vector3d::Zero());
    detail::trimesh_in_place(ctx, mesh, false, [normalized](DeviceTriangleMesh &d) { d.ComputeVertexNormals(normalized); });
    if (!mesh.HasTriangleNormals()) mesh.triangle_normals_.resize(mesh.triangles_.size());
}
inline void Purge(visma_icp_ctx *ctx, TriangleMesh &mesh)
{
    detail::trimesh_in_place(ctx, mesh, false, [](DeviceTriangleMesh &d) { d.Purge(); });
}
inline std::shared_ptr<TriangleMesh> SelectDownSample(visma_icp_ctx *ctx, const TriangleMesh &input, const std::vector<size_t> &indices)
{
    return DeviceTriangleMesh(ctx, input).Select(indices).Download();
}
inline std::shared_ptr<TriangleMesh> CropTriangleMesh(visma_icp_ctx *ctx, const TriangleMesh &input, const Eigen::Vector3d &min_bound,
                                                      const Eigen::Vector3d &max_bound)
{
    return DeviceTriangleMesh(ctx, input).Crop(min_bound, max_bound).Download();
}
// ExtractTriangleMesh and what follows it in the reference pipeline, on the device, with ONE download: the volume's mesh is
// copied device to device, purged where asked, and given vertex normals (ComputeVertexNormals(normalized)) where asked
inline std::shared_ptr<TriangleMesh> ExtractTriangleMesh(TSDFVolume &volume, bool purge, bool vertex_normals, bool normalized = true)
{
    int64_t nv = 0, nt = 0;
    detail::check(volume.Context(), visma_icp_tsdf_extract_triangle_mesh(volume.Context(), volume.Handle(), &nv, &nt),
                  "visma_icp_tsdf_extract_triangle_mesh");
    DeviceTriangleMesh d = DeviceTriangleMesh::FromVolume(volume);
    if (purge) d.Purge();
    if (vertex_normals) d.ComputeVertexNormals(normalized);
    return d.Download();
}

// ---- open3d::PointCloud on the GPU (visma_icp.h, "PointCloud") ----
// DevicePointCloud: a cloud resident on the device, for a chain of steps with one upload and one download -- or none: the
// cloud a TSDF volume extracted is taken where it lies (FromVolume).  The free functions below are one such chain each.  A
// selected index outside [0, points) throws std::runtime_error, as do the OrientNormals* of a cloud without normals.
class DevicePointCloud {
public:
    DevicePointCloud(visma_icp_ctx *ctx, const PointCloud &cloud) : ctx_(ctx)
    {
        detail::check(ctx_, visma_icp_cloud_create(ctx_, detail::xyz(cloud.points_), (int64_t)cloud.points_.size(),
                                                   cloud.HasNormals() ? detail::xyz(cloud.normals_) : nullptr,
                                                   cloud.HasColors() ? detail::xyz(cloud.colors_) : nullptr, &cloud_),
                      "visma_icp_cloud_create");
    }
    explicit DevicePointCloud(const PointCloud &cloud) : DevicePointCloud(detail::ThreadContext::instance().get(), cloud) {}
    // the volume's last ExtractPointCloud (or, voxel_cloud, ExtractVoxelPointCloud), copied device to device (extract first:
    // cicp::ExtractPointCloud does both)
    static DevicePointCloud FromVolume(const TSDFVolume &volume, bool voxel_cloud = false)
    {
        DevicePointCloud c(volume.Context(), nullptr);
        detail::check(c.ctx_, visma_icp_cloud_from_tsdf(c.ctx_, volume.Handle(), voxel_cloud ? 1 : 0, &c.cloud_), "visma_icp_cloud_from_tsdf");
        return c;
    }
    ~DevicePointCloud() { if (cloud_) (void)visma_icp_cloud_destroy(ctx_, cloud_); }
    DevicePointCloud(DevicePointCloud &&o) noexcept : ctx_(o.ctx_), cloud_(o.cloud_) { o.cloud_ = nullptr; }
    DevicePointCloud &operator=(DevicePointCloud &&o) noexcept                       // (c = c.Crop(lo, hi): the old cloud is freed)
    {
        if (this != &o) {
            if (cloud_) (void)visma_icp_cloud_destroy(ctx_, cloud_);
            ctx_ = o.ctx_; cloud_ = o.cloud_;
            o.cloud_ = nullptr;
        }
        return *this;
    }
    DevicePointCloud(const DevicePointCloud &) = delete;
    DevicePointCloud &operator=(const DevicePointCloud &) = delete;

    size_t size() const
    {
        int64_t n = 0;
        detail::check(ctx_, visma_icp_cloud_size(cloud_, &n, nullptr), "visma_icp_cloud_size");
        return (size_t)n;
    }
    void Transform(const Eigen::Matrix4d &T)
    {
        double t[16];
        for (int i = 0; i < 16; i++) t[i] = T(i / 4, i % 4);          // (either storage order)
        detail::check(ctx_, visma_icp_cloud_transform(ctx_, cloud_, t), "visma_icp_cloud_transform");
    }
    void NormalizeNormals() { detail::check(ctx_, visma_icp_cloud_normalize_normals(ctx_, cloud_), "visma_icp_cloud_normalize_normals"); }
    void PaintUniformColor(const Eigen::Vector3d &color)
    {
        detail::check(ctx_, visma_icp_cloud_paint_uniform_color(ctx_, cloud_, color.data()), "visma_icp_cloud_paint_uniform_color");
    }
    DevicePointCloud &operator+=(const DevicePointCloud &other)
    {
        detail::check(ctx_, visma_icp_cloud_append(ctx_, cloud_, other.cloud_), "visma_icp_cloud_append");
        return *this;
    }
    Eigen::Vector3d GetMinBound() const { return Bounds().first; }
    Eigen::Vector3d GetMaxBound() const { return Bounds().second; }
    std::pair<Eigen::Vector3d, Eigen::Vector3d> Bounds() const
    {
        Eigen::Vector3d lo, hi;
        detail::check(ctx_, visma_icp_cloud_bounds(ctx_, cloud_, lo.data(), hi.data()), "visma_icp_cloud_bounds");
        return std::make_pair(lo, hi);
    }
    DevicePointCloud Select(const std::vector<size_t> &indices) const
    {
        const std::vector<int64_t> idx(indices.begin(), indices.end());
        DevicePointCloud out(ctx_, nullptr);
        detail::check(ctx_, visma_icp_cloud_select(ctx_, cloud_, idx.data(), (int64_t)idx.size(), &out.cloud_), "visma_icp_cloud_select");
        return out;
    }
    DevicePointCloud UniformDownSample(size_t every_k_points) const
    {
        DevicePointCloud out(ctx_, nullptr);
        const int64_t k = every_k_points > (size_t)std::numeric_limits<int64_t>::max() ? std::numeric_limits<int64_t>::max() : (int64_t)every_k_points;
        detail::check(ctx_, visma_icp_cloud_uniform_down_sample(ctx_, cloud_, k, &out.cloud_), "visma_icp_cloud_uniform_down_sample");
        return out;
    }
    DevicePointCloud Crop(const Eigen::Vector3d &min_bound, const Eigen::Vector3d &max_bound) const
    {
        DevicePointCloud out(ctx_, nullptr);
        detail::check(ctx_, visma_icp_cloud_crop(ctx_, cloud_, min_bound.data(), max_bound.data(), &out.cloud_), "visma_icp_cloud_crop");
        return out;
    }
    DevicePointCloud VoxelDownSample(double voxel_size) const
    {
        DevicePointCloud out(ctx_, nullptr);
        detail::check(ctx_, visma_icp_cloud_voxel_down_sample(ctx_, cloud_, voxel_size, &out.cloud_), "visma_icp_cloud_voxel_down_sample");
        return out;
    }
    void EstimateNormals(const KDTreeSearchParam &search_param = KDTreeSearchParamKNN())
    {
        int type = 0, knn = 0;
        double radius = 0.0;
        detail::search_arguments(search_param, &type, &knn, &radius);
        detail::check(ctx_, visma_icp_cloud_estimate_normals(ctx_, cloud_, type, knn, radius), "visma_icp_cloud_estimate_normals");
    }
    void OrientNormalsToAlignWithDirection(const Eigen::Vector3d &orientation_reference = Eigen::Vector3d(0.0, 0.0, 1.0))
    {
        detail::check(ctx_, visma_icp_cloud_orient_normals_to_align_with_direction(ctx_, cloud_, orientation_reference.data()),
                      "visma_icp_cloud_orient_normals_to_align_with_direction");
    }
    void OrientNormalsTowardsCameraLocation(const Eigen::Vector3d &camera_location = Eigen::Vector3d::Zero())
    {
        detail::check(ctx_, visma_icp_cloud_orient_normals_towards_camera_location(ctx_, cloud_, camera_location.data()),
                      "visma_icp_cloud_orient_normals_towards_camera_location");
    }
    std::tuple<Eigen::Vector3d, Eigen::Matrix3d> MeanAndCovariance() const
    {
        Eigen::Vector3d mean;
        double cov[9];
        detail::check(ctx_, visma_icp_cloud_mean_and_covariance(ctx_, cloud_, mean.data(), cov), "visma_icp_cloud_mean_and_covariance");
        Eigen::Matrix3d C;
        for (int i = 0; i < 9; i++) C(i / 3, i % 3) = cov[i];          // (either storage order)
        return std::make_tuple(mean, C);
    }
    std::vector<double> MahalanobisDistance() const
    {
        std::vector<double> out(size());
        detail::check(ctx_, visma_icp_cloud_mahalanobis_distance(ctx_, cloud_, out.data()), "visma_icp_cloud_mahalanobis_distance");
        return out;
    }
    // the device's rows into `cloud`; an attribute the device cloud does not have is cleared
    void Download(PointCloud &cloud) const
    {
        int64_t n = 0;
        int has = 0;
        detail::check(ctx_, visma_icp_cloud_size(cloud_, &n, &has), "visma_icp_cloud_size");
        const bool hn = has & VISMA_ICP_CLOUD_HAS_NORMALS, hc = has & VISMA_ICP_CLOUD_HAS_COLORS;
        cloud.points_.resize((size_t)n);
        cloud.normals_.resize(hn ? (size_t)n : 0);
        cloud.colors_.resize(hc ? (size_t)n : 0);
        detail::check(ctx_, visma_icp_cloud_get(ctx_, cloud_, n ? cloud.points_[0].data() : nullptr, hn ? cloud.normals_[0].data() : nullptr,
                                                hc ? cloud.colors_[0].data() : nullptr, n),
                      "visma_icp_cloud_get");
    }
    std::shared_ptr<PointCloud> Download() const
    {
        auto out = std::make_shared<PointCloud>();
        Download(*out);
        return out;
    }
    visma_icp_ctx *context() const { return ctx_; }
    visma_icp_cloud *handle() const { return cloud_; }

private:
    DevicePointCloud(visma_icp_ctx *ctx, std::nullptr_t) : ctx_(ctx) {}
    visma_icp_ctx *ctx_ = nullptr;
    visma_icp_cloud *cloud_ = nullptr;
};

// the free functions of Core/Geometry/PointCloud.h on a context of the caller's: one upload, one operation, one download
inline std::shared_ptr<PointCloud> SelectDownSample(visma_icp_ctx *ctx, const PointCloud &input, const std::vector<size_t> &indices)
{
    return DevicePointCloud(ctx, input).Select(indices).Download();
}
inline std::shared_ptr<PointCloud> UniformDownSample(visma_icp_ctx *ctx, const PointCloud &input, size_t every_k_points)
{
    return DevicePointCloud(ctx, input).UniformDownSample(every_k_points).Download();
}
inline std::shared_ptr<PointCloud> CropPointCloud(visma_icp_ctx *ctx, const PointCloud &input, const Eigen::Vector3d &min_bound,
                                                  const Eigen::Vector3d &max_bound)
{
    return DevicePointCloud(ctx, input).Crop(min_bound, max_bound).Download();
}
inline std::tuple<Eigen::Vector3d, Eigen::Matrix3d> ComputePointCloudMeanAndCovariance(visma_icp_ctx *ctx, const PointCloud &input)
{
    return DevicePointCloud(ctx, input).MeanAndCovariance();
}
inline std::vector<double> ComputePointCloudMahalanobisDistance(visma_icp_ctx *ctx, const PointCloud &input)
{
    return DevicePointCloud(ctx, input).MahalanobisDistance();
}
// ExtractPointCloud with the cloud left on the device: what follows it in the reference pipeline (crop, VoxelDownSample,
// EstimateNormals) runs there, and Download() is the one copy to the host
inline DevicePointCloud ExtractPointCloud(TSDFVolume &volume)
{
    int64_t n = 0;
    detail::check(volume.Context(), visma_icp_tsdf_extract_point_cloud(volume.Context(), volume.Handle(), &n), "visma_icp_tsdf_extract_point_cloud");
    return DevicePointCloud::FromVolume(volume);
}
#endif

}  // namespace cicp

#ifdef VISMA_ICP_STANDALONE_OPEN3D_TYPES
// Stand-alone header set: give the stock names their bodies too.
inline void ColorMapOptimization(TriangleMesh &mesh, const std::vector<RGBDImage> &images_rgbd, PinholeCameraTrajectory &camera,
                                 const ColorMapOptmizationOption &option)
{
    cicp::ColorMapOptimization(mesh, images_rgbd, camera, option);
}
inline std::shared_ptr<PointCloud> CreatePointCloudFromDepthImage(const Image &depth, const PinholeCameraIntrinsic &intrinsic,
                                                                  const Eigen::Matrix4d &extrinsic, double depth_scale, double depth_trunc,
                                                                  int stride)
{
    return cicp::CreatePointCloudFromDepthImage(depth, intrinsic, extrinsic, depth_scale, depth_trunc, stride);
}
inline std::shared_ptr<PointCloud> CreatePointCloudFromRGBDImage(const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic,
                                                                 const Eigen::Matrix4d &extrinsic)
{
    return cicp::CreatePointCloudFromRGBDImage(image, intrinsic, extrinsic);
}
// open3d::TriangleMesh (Core/Geometry/TriangleMesh.h): the members that compute, on this thread's context
inline void TriangleMesh::NormalizeNormals() { cicp::NormalizeNormals(cicp::detail::ThreadContext::instance().get(), *this); }
inline void TriangleMesh::Transform(const Eigen::Matrix4d &transformation)
{
    cicp::Transform(cicp::detail::ThreadContext::instance().get(), *this, transformation);
}
inline void TriangleMesh::ComputeTriangleNormals(bool normalized)
{
    cicp::ComputeTriangleNormals(cicp::detail::ThreadContext::instance().get(), *this, normalized);
}
inline void TriangleMesh::ComputeVertexNormals(bool normalized)
{
    cicp::ComputeVertexNormals(cicp::detail::ThreadContext::instance().get(), *this, normalized);
}
inline void TriangleMesh::Purge() { cicp::Purge(cicp::detail::ThreadContext::instance().get(), *this); }
inline std::shared_ptr<TriangleMesh> SelectDownSample(const TriangleMesh &input, const std::vector<size_t> &indices)
{
    return cicp::SelectDownSample(cicp::detail::ThreadContext::instance().get(), input, indices);
}
inline std::shared_ptr<TriangleMesh> CropTriangleMesh(const TriangleMesh &input, const Eigen::Vector3d &min_bound, const Eigen::Vector3d &max_bound)
{
    return cicp::CropTriangleMesh(cicp::detail::ThreadContext::instance().get(), input, min_bound, max_bound);
}
// open3d::KDTreeFlann (Core/Geometry/KDTreeFlann.h): the tree is an object of the context, resident on the GPU
inline KDTreeFlann::~KDTreeFlann()
{
    if (tree_) (void)visma_icp_kdtree_destroy(tree_);
}
inline bool KDTreeFlann::SetRawData(const double *xyz, size_t n)
{
    if (tree_) (void)visma_icp_kdtree_destroy(tree_);
    tree_ = nullptr;
    dataset_size_ = 0;
    if (n == 0) return false;                                       // (KDTreeFlann.cpp:195-198: "Failed due to no data")
    if (!ctx_) ctx_ = cicp::detail::ThreadContext::instance().get();
    cicp::detail::check(ctx_, visma_icp_kdtree_create(ctx_, xyz, (int64_t)n, &tree_), "visma_icp_kdtree_create");
    dataset_size_ = n;
    return true;
}
inline bool KDTreeFlann::SetMatrixData(const Eigen::MatrixXd &data)
{
    if (data.rows() != 3) { SetRawData(nullptr, 0); return false; }
    std::vector<double> xyz((size_t)data.cols() * 3);               // (either storage order)
    for (Eigen::Index j = 0; j < data.cols(); j++)
        for (int k = 0; k < 3; k++) xyz[(size_t)j * 3 + k] = data(k, j);
    return SetRawData(xyz.data(), (size_t)data.cols());
}
inline bool KDTreeFlann::SetGeometry(const PointCloud &geometry) { return SetRawData(cicp::detail::xyz(geometry.points_), geometry.points_.size()); }
inline bool KDTreeFlann::SetGeometry(const TriangleMesh &geometry) { return SetRawData(cicp::detail::xyz(geometry.vertices_), geometry.vertices_.size()); }
template <typename T>
inline int KDTreeFlann::Search(const T &query, const KDTreeSearchParam &param, std::vector<int> &indices, std::vector<double> &distance2) const
{
    switch (param.GetSearchType()) {
    case KDTreeSearchParam::SearchType::Knn: return SearchKNN(query, ((const KDTreeSearchParamKNN &)param).knn_, indices, distance2);
    case KDTreeSearchParam::SearchType::Radius: return SearchRadius(query, ((const KDTreeSearchParamRadius &)param).radius_, indices, distance2);
    case KDTreeSearchParam::SearchType::Hybrid:
        return SearchHybrid(query, ((const KDTreeSearchParamHybrid &)param).radius_, ((const KDTreeSearchParamHybrid &)param).max_nn_, indices, distance2);
    default: return -1;
    }
}
template <typename T>
inline int KDTreeFlann::SearchKNN(const T &query, int knn, std::vector<int> &indices, std::vector<double> &distance2) const
{
    if (!tree_ || query.rows() != 3 || knn < 0) return -1;          // KDTreeFlann.cpp:124-128
    const std::vector<Eigen::Vector3d> q(1, Eigen::Vector3d(query(0), query(1), query(2)));
    std::vector<int> count;
    cicp::KDTreeSearchKNN(*this, q, knn, indices, distance2, count);
    indices.resize((size_t)count[0]);
    distance2.resize((size_t)count[0]);
    return count[0];
}
template <typename T>
inline int KDTreeFlann::SearchRadius(const T &query, double radius, std::vector<int> &indices, std::vector<double> &distance2) const
{
    if (!tree_ || query.rows() != 3) return -1;                     // KDTreeFlann.cpp:149-151
    const std::vector<Eigen::Vector3d> q(1, Eigen::Vector3d(query(0), query(1), query(2)));
    std::vector<int64_t> offsets;
    cicp::KDTreeSearchRadius(*this, q, radius, offsets, indices, distance2);
    return (int)offsets[1];
}
template <typename T>
inline int KDTreeFlann::SearchHybrid(const T &query, double radius, int max_nn, std::vector<int> &indices, std::vector<double> &distance2) const
{
    if (!tree_ || query.rows() != 3 || max_nn < 0) return -1;       // KDTreeFlann.cpp:172-175
    const std::vector<Eigen::Vector3d> q(1, Eigen::Vector3d(query(0), query(1), query(2)));
    std::vector<int> count;
    cicp::KDTreeSearchHybrid(*this, q, radius, max_nn, indices, distance2, count);
    indices.resize((size_t)count[0]);
    distance2.resize((size_t)count[0]);
    return count[0];
}
// open3d::UniformTSDFVolume (Core/Integration/UniformTSDFVolume.h): the volume is an object of the context, resident on the GPU
inline void UniformTSDFVolume::Create(visma_icp_ctx *ctx)
{
    ctx_ = ctx;
    cicp::detail::check(ctx_, visma_icp_tsdf_create_uniform(ctx_, length_, resolution_, sdf_trunc_, (int)color_type_, origin_.data(), &volume_),
                        "visma_icp_tsdf_create_uniform");
}
inline UniformTSDFVolume::UniformTSDFVolume(double length, int resolution, double sdf_trunc, TSDFVolumeColorType color_type,
                                            const Eigen::Vector3d &origin)
    : TSDFVolume(length / (double)resolution, sdf_trunc, color_type), origin_(origin), length_(length), resolution_(resolution),
      voxel_num_(resolution * resolution * resolution)
{
    Create(cicp::detail::ThreadContext::instance().get());
}
inline UniformTSDFVolume::UniformTSDFVolume(visma_icp_ctx *ctx, double length, int resolution, double sdf_trunc,
                                            TSDFVolumeColorType color_type, const Eigen::Vector3d &origin)
    : TSDFVolume(length / (double)resolution, sdf_trunc, color_type), origin_(origin), length_(length), resolution_(resolution),
      voxel_num_(resolution * resolution * resolution)
{
    Create(ctx);
}
inline UniformTSDFVolume::~UniformTSDFVolume()
{
    if (volume_) (void)visma_icp_tsdf_destroy(ctx_, volume_);
}
inline void UniformTSDFVolume::Reset() { cicp::detail::check(ctx_, visma_icp_tsdf_reset(ctx_, volume_), "visma_icp_tsdf_reset"); }
inline void UniformTSDFVolume::Integrate(const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic, const Eigen::Matrix4d &extrinsic)
{
    cicp::detail::tsdf_integrate(ctx_, volume_, (int)color_type_, "[UniformTSDFVolume::Integrate] ", image, intrinsic, extrinsic);
}
inline std::shared_ptr<PointCloud> UniformTSDFVolume::ExtractPointCloud()
{
    return cicp::detail::tsdf_extract_point_cloud(ctx_, volume_, color_type_ != TSDFVolumeColorType::None);
}
inline std::shared_ptr<TriangleMesh> UniformTSDFVolume::ExtractTriangleMesh()
{
    return cicp::detail::tsdf_extract_triangle_mesh(ctx_, volume_, color_type_ != TSDFVolumeColorType::None);
}
inline std::shared_ptr<PointCloud> UniformTSDFVolume::ExtractVoxelPointCloud() { return cicp::detail::tsdf_extract_voxel_point_cloud(ctx_, volume_); }
inline void UniformTSDFVolume::Download(std::vector<float> &tsdf, std::vector<float> &weight, std::vector<Eigen::Vector3f> &color) const
{
    cicp::detail::tsdf_download(ctx_, volume_, nullptr, (size_t)voxel_num_, color_type_ != TSDFVolumeColorType::None, tsdf, weight, color);
}
// open3d::ScalableTSDFVolume (Core/Integration/ScalableTSDFVolume.h)
inline ScalableTSDFVolume::ScalableTSDFVolume(visma_icp_ctx *ctx, double voxel_length, double sdf_trunc, TSDFVolumeColorType color_type,
                                              int volume_unit_resolution, int depth_sampling_stride, int initial_units)
    : TSDFVolume(voxel_length, sdf_trunc, color_type), volume_unit_resolution_(volume_unit_resolution),
      volume_unit_length_(voxel_length * volume_unit_resolution), depth_sampling_stride_(depth_sampling_stride), ctx_(ctx)
{
    cicp::detail::check(ctx_, visma_icp_tsdf_create_scalable(ctx_, voxel_length_, sdf_trunc_, (int)color_type_, volume_unit_resolution_,
                                                             depth_sampling_stride_, initial_units, &volume_),
                        "visma_icp_tsdf_create_scalable");
}
inline ScalableTSDFVolume::ScalableTSDFVolume(double voxel_length, double sdf_trunc, TSDFVolumeColorType color_type, int volume_unit_resolution,
                                              int depth_sampling_stride)
    : ScalableTSDFVolume(cicp::detail::ThreadContext::instance().get(), voxel_length, sdf_trunc, color_type, volume_unit_resolution,
                         depth_sampling_stride, 0)
{
}
inline ScalableTSDFVolume::~ScalableTSDFVolume()
{
    if (volume_) (void)visma_icp_tsdf_destroy(ctx_, volume_);
}
inline void ScalableTSDFVolume::Reset() { cicp::detail::check(ctx_, visma_icp_tsdf_reset(ctx_, volume_), "visma_icp_tsdf_reset"); }
inline void ScalableTSDFVolume::Integrate(const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic, const Eigen::Matrix4d &extrinsic)
{
    cicp::detail::tsdf_integrate(ctx_, volume_, (int)color_type_, "[ScalableTSDFVolume::Integrate] ", image, intrinsic, extrinsic);
}
inline std::shared_ptr<PointCloud> ScalableTSDFVolume::ExtractPointCloud()
{
    return cicp::detail::tsdf_extract_point_cloud(ctx_, volume_, color_type_ != TSDFVolumeColorType::None);
}
inline std::shared_ptr<TriangleMesh> ScalableTSDFVolume::ExtractTriangleMesh()
{
    return cicp::detail::tsdf_extract_triangle_mesh(ctx_, volume_, color_type_ != TSDFVolumeColorType::None);
}
inline std::shared_ptr<PointCloud> ScalableTSDFVolume::ExtractVoxelPointCloud() { return cicp::detail::tsdf_extract_voxel_point_cloud(ctx_, volume_); }
inline std::vector<Eigen::Vector3i> ScalableTSDFVolume::Units() const
{
    int64_t n = 0;
    cicp::detail::check(ctx_, visma_icp_tsdf_get_units(ctx_, volume_, nullptr, 0, &n), "visma_icp_tsdf_get_units");
    std::vector<int32_t> k(3 * (size_t)n + 3);
    cicp::detail::check(ctx_, visma_icp_tsdf_get_units(ctx_, volume_, k.data(), n, &n), "visma_icp_tsdf_get_units");
    std::vector<Eigen::Vector3i> out((size_t)n);
    for (size_t i = 0; i < out.size(); i++) out[i] = Eigen::Vector3i(k[3 * i], k[3 * i + 1], k[3 * i + 2]);
    return out;
}
inline bool ScalableTSDFVolume::DownloadUnit(const Eigen::Vector3i &index, std::vector<float> &tsdf, std::vector<float> &weight,
                                             std::vector<Eigen::Vector3f> &color) const
{
    for (const auto &u : Units())
        if (u == index) {
            const int32_t key[3] = {index(0), index(1), index(2)};
            const size_t n = (size_t)volume_unit_resolution_ * volume_unit_resolution_ * volume_unit_resolution_;
            cicp::detail::tsdf_download(ctx_, volume_, key, n, color_type_ != TSDFVolumeColorType::None, tsdf, weight, color);
            return true;
        }
    return false;
}
inline double TransformationEstimationPointToPoint::ComputeRMSE(
    const PointCloud &s, const PointCloud &t, const CorrespondenceSet &c) const
{
    return cicp::detail::host_rmse_point_to_point(s, t, c);
}
inline Eigen::Matrix4d TransformationEstimationPointToPoint::ComputeTransformation(
    const PointCloud &s, const PointCloud &t, const CorrespondenceSet &c) const
{
    return cicp::detail::host_update(s, t, c, false, with_scaling_);
}
// NB the reference's point-to-plane ComputeRMSE assigns `err = r * r` instead of
// accumulating (TransformationEstimation.cpp:70), i.e. it returns
// sqrt(r_last^2 / K).  RegistrationICP never calls it; we keep its value.
inline double TransformationEstimationPointToPlane::ComputeRMSE(
    const PointCloud &s, const PointCloud &t, const CorrespondenceSet &c) const
{
    if (c.empty() || !t.HasNormals()) return 0.0;
    const auto &l = c.back();
    const double r = (s.points_[l[0]] - t.points_[l[1]]).dot(t.normals_[l[1]]);
    return std::sqrt(r * r / (double)c.size());
}
inline Eigen::Matrix4d TransformationEstimationPointToPlane::ComputeTransformation(
    const PointCloud &s, const PointCloud &t, const CorrespondenceSet &c) const
{
    if (c.empty() || !t.HasNormals()) return Eigen::Matrix4d::Identity();
    return cicp::detail::host_update(s, t, c, true, false);
}
inline std::shared_ptr<PointCloud> VoxelDownSample(const PointCloud &input, double voxel_size)
{
    return cicp::VoxelDownSample(input, voxel_size);
}
inline std::shared_ptr<PointCloud> SelectDownSample(const PointCloud &input, const std::vector<size_t> &indices)
{
    return cicp::SelectDownSample(cicp::detail::ThreadContext::instance().get(), input, indices);
}
inline std::shared_ptr<PointCloud> UniformDownSample(const PointCloud &input, size_t every_k_points)
{
    return cicp::UniformDownSample(cicp::detail::ThreadContext::instance().get(), input, every_k_points);
}
inline std::shared_ptr<PointCloud> CropPointCloud(const PointCloud &input, const Eigen::Vector3d &min_bound, const Eigen::Vector3d &max_bound)
{
    return cicp::CropPointCloud(cicp::detail::ThreadContext::instance().get(), input, min_bound, max_bound);
}
inline std::tuple<Eigen::Vector3d, Eigen::Matrix3d> ComputePointCloudMeanAndCovariance(const PointCloud &input)
{
    return cicp::ComputePointCloudMeanAndCovariance(cicp::detail::ThreadContext::instance().get(), input);
}
inline std::vector<double> ComputePointCloudMahalanobisDistance(const PointCloud &input)
{
    return cicp::ComputePointCloudMahalanobisDistance(cicp::detail::ThreadContext::instance().get(), input);
}
inline Eigen::Matrix6d GetInformationMatrixFromPointClouds(const PointCloud &source, const PointCloud &target,
                                                           double max_correspondence_distance,
                                                           const Eigen::Matrix4d &transformation)
{
    return cicp::GetInformationMatrixFromPointClouds(source, target, max_correspondence_distance, transformation);
}
inline std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d> ComputeRGBDOdometry(
        const RGBDImage &source, const RGBDImage &target, const PinholeCameraIntrinsic &pinhole_camera_intrinsic, const Eigen::Matrix4d &odo_init,
        const RGBDOdometryJacobian &jacobian_method, const OdometryOption &option)
{
    return cicp::ComputeRGBDOdometry(source, target, pinhole_camera_intrinsic, odo_init, jacobian_method, option);
}
inline void GlobalOptimizationGaussNewton::OptimizePoseGraph(PoseGraph &pose_graph,
                                                             const GlobalOptimizationConvergenceCriteria &criteria,
                                                             const GlobalOptimizationOption &option) const
{
    cicp::detail::run_pose_graph(pose_graph, false, VISMA_ICP_GLOBAL_GAUSS_NEWTON, criteria, option);
}
inline void GlobalOptimizationLevenbergMarquardt::OptimizePoseGraph(PoseGraph &pose_graph,
                                                                    const GlobalOptimizationConvergenceCriteria &criteria,
                                                                    const GlobalOptimizationOption &option) const
{
    cicp::detail::run_pose_graph(pose_graph, false, VISMA_ICP_GLOBAL_LEVENBERG_MARQUARDT, criteria, option);
}
inline void GlobalOptimization(PoseGraph &pose_graph, const GlobalOptimizationMethod &method,
                               const GlobalOptimizationConvergenceCriteria &criteria, const GlobalOptimizationOption &option)
{
    cicp::GlobalOptimization(pose_graph, method, criteria, option);
}
inline std::shared_ptr<PoseGraph> CreatePoseGraphWithoutInvalidEdges(const PoseGraph &pose_graph,
                                                                     const GlobalOptimizationOption &option)
{
    std::shared_ptr<PoseGraph> pruned = std::make_shared<PoseGraph>();
    pruned->nodes_ = pose_graph.nodes_;
    for (const PoseGraphEdge &t : pose_graph.edges_)
        if (!t.uncertain_ || t.confidence_ > option.edge_prune_threshold_) pruned->edges_.push_back(t);
    return pruned;
}
inline RegistrationResult EvaluateRegistration(const PointCloud &source, const PointCloud &target,
                                               double max_correspondence_distance,
                                               const Eigen::Matrix4d &transformation)
{
    return cicp::EvaluateRegistration(source, target, max_correspondence_distance, transformation);
}
inline RegistrationResult RegistrationColoredICP(const PointCloud &source, const PointCloud &target, double max_distance,
                                                 const Eigen::Matrix4d &init = Eigen::Matrix4d::Identity(),
                                                 const ICPConvergenceCriteria &criteria = ICPConvergenceCriteria(),
                                                 double lambda_geometric = 0.968)
{
    return cicp::RegistrationColoredICP(source, target, max_distance, init, criteria, lambda_geometric);
}
inline std::shared_ptr<Feature> ComputeFPFHFeature(const PointCloud &input, const KDTreeSearchParam &search_param)
{
    return cicp::ComputeFPFHFeature(input, search_param);
}
inline RegistrationResult FastGlobalRegistration(const PointCloud &source, const PointCloud &target, const Feature &source_feature,
                                                 const Feature &target_feature, const FastGlobalRegistrationOption &option)
{
    return cicp::FastGlobalRegistration(source, target, source_feature, target_feature, option);
}
inline RegistrationResult RegistrationRANSACBasedOnCorrespondence(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres, double max_correspondence_distance,
    const TransformationEstimation &estimation, int ransac_n, const RANSACConvergenceCriteria &criteria)
{
    return cicp::RegistrationRANSACBasedOnCorrespondence(source, target, corres, max_correspondence_distance, estimation, ransac_n,
                                                         criteria);
}
inline RegistrationResult RegistrationRANSACBasedOnFeatureMatching(
    const PointCloud &source, const PointCloud &target, const Feature &source_feature, const Feature &target_feature,
    double max_correspondence_distance, const TransformationEstimation &estimation, int ransac_n,
    const std::vector<std::reference_wrapper<const CorrespondenceChecker>> &checkers, const RANSACConvergenceCriteria &criteria)
{
    return cicp::RegistrationRANSACBasedOnFeatureMatching(source, target, source_feature, target_feature, max_correspondence_distance,
                                                          estimation, ransac_n, checkers, criteria);
}
inline bool ReadPointCloudFromPLY(const std::string &filename, PointCloud &pointcloud)
{
    return cicp::ReadPointCloudFromPLY(filename, pointcloud);
}
inline bool ReadPointCloudFromPCD(const std::string &filename, PointCloud &pointcloud)
{
    return cicp::ReadPointCloudFromPCD(filename, pointcloud);
}
inline bool EstimateNormals(PointCloud &cloud, const KDTreeSearchParam &search_param)
{
    return cicp::EstimateNormals(cloud, search_param);
}
inline std::vector<double> ComputePointCloudToPointCloudDistance(const PointCloud &source, const PointCloud &target)
{
    return cicp::ComputePointCloudToPointCloudDistance(source, target);
}
inline std::vector<double> ComputePointCloudNearestNeighborDistance(const PointCloud &input)
{
    return cicp::ComputePointCloudNearestNeighborDistance(input);
}
inline bool OrientNormalsToAlignWithDirection(PointCloud &cloud, const Eigen::Vector3d &orientation_reference)
{
    return cicp::OrientNormalsToAlignWithDirection(cloud, orientation_reference);
}
inline bool OrientNormalsTowardsCameraLocation(PointCloud &cloud, const Eigen::Vector3d &camera_location)
{
    return cicp::OrientNormalsTowardsCameraLocation(cloud, camera_location);
}
inline RegistrationResult RegistrationICP(const PointCloud &source, const PointCloud &target,
                                          double max_correspondence_distance,
                                          const Eigen::Matrix4d &init,
                                          const TransformationEstimation &estimation,
                                          const ICPConvergenceCriteria &criteria)
{
    return cicp::RegistrationICP(source, target, max_correspondence_distance, init, estimation,
                                 criteria);
}

// ---- Image: the reference's Image.h, ImageFactory.cpp, RGBDImage.h and RGBDImageFactory.cpp on the GPU ---------------------
namespace cicp {

// DeviceImage: an image resident on the device, for a chain of steps with one upload and one download -- or none, where the
// chain ends in a volume or in the odometry.  Every step that makes an image returns a new DeviceImage.  An EMPTY DeviceImage
// (no handle) stands for the pair of NULLs visma_icp_image_rgbd answers images of different sizes with.
class DeviceImage {
public:
    DeviceImage(visma_icp_ctx *ctx, const Image &image) : ctx_(ctx)
    {
        if (image.num_of_channels_ == 0) return;             // the reference's empty Image: every operation on it gives it again
        detail::check(ctx_, visma_icp_image_create(ctx_, image.width_, image.height_, image.num_of_channels_, image.bytes_per_channel_,
                                                   image.data_.data(), &img_), "visma_icp_image_create");
    }
    explicit DeviceImage(const Image &image) : DeviceImage(detail::ThreadContext::instance().get(), image) {}
    DeviceImage(visma_icp_ctx *ctx, visma_icp_image *adopted) : ctx_(ctx), img_(adopted) {}
    ~DeviceImage() { if (img_) (void)visma_icp_image_destroy(ctx_, img_); }
    DeviceImage(DeviceImage &&o) noexcept : ctx_(o.ctx_), img_(o.img_) { o.img_ = nullptr; }
    DeviceImage &operator=(DeviceImage &&o) noexcept
    {
        if (this != &o) {
            if (img_) (void)visma_icp_image_destroy(ctx_, img_);
            ctx_ = o.ctx_; img_ = o.img_; o.img_ = nullptr;
        }
        return *this;
    }
    DeviceImage(const DeviceImage &) = delete;
    DeviceImage &operator=(const DeviceImage &) = delete;

    visma_icp_ctx *Context() const { return ctx_; }
    visma_icp_image *Handle() const { return img_; }
    // the one copy to the host; the empty Image for an empty DeviceImage
    std::shared_ptr<Image> Download() const
    {
        auto out = std::make_shared<Image>();
        if (!img_) return out;
        int w, h, c, b;
        detail::check(ctx_, visma_icp_image_info(img_, &w, &h, &c, &b), "visma_icp_image_info");
        out->PrepareImage(w, h, c, b);
        detail::check(ctx_, visma_icp_image_get(ctx_, img_, out->data_.data(), (int64_t)out->data_.size()), "visma_icp_image_get");
        return out;
    }
    DeviceImage ToFloat(Image::ColorToIntensityConversionType type = Image::ColorToIntensityConversionType::Weighted) const
    {
        return make("visma_icp_image_to_float", [&](visma_icp_image **o) {
            return visma_icp_image_to_float(ctx_, img_, type == Image::ColorToIntensityConversionType::Equal ? VISMA_ICP_IMAGE_EQUAL : VISMA_ICP_IMAGE_WEIGHTED, o); });
    }
    DeviceImage DepthToFloat(double depth_scale = 1000.0, double depth_trunc = 3.0) const
    {
        return make("visma_icp_image_depth_to_float", [&](visma_icp_image **o) { return visma_icp_image_depth_to_float(ctx_, img_, depth_scale, depth_trunc, o); });
    }
    DeviceImage FromFloat(int bytes) const
    {
        return make("visma_icp_image_from_float", [&](visma_icp_image **o) { return visma_icp_image_from_float(ctx_, img_, bytes, o); });
    }
    DeviceImage Filter(Image::FilterType type) const
    {
        return make("visma_icp_image_filter", [&](visma_icp_image **o) { return visma_icp_image_filter(ctx_, img_, (int)type, o); });
    }
    DeviceImage Filter(const std::vector<double> &dx, const std::vector<double> &dy) const
    {
        return make("visma_icp_image_filter_separable", [&](visma_icp_image **o) {
            return visma_icp_image_filter_separable(ctx_, img_, dx.data(), (int)dx.size(), dy.data(), (int)dy.size(), o); });
    }
    DeviceImage FilterHorizontal(const std::vector<double> &kernel) const
    {
        return make("visma_icp_image_filter_horizontal", [&](visma_icp_image **o) {
            return visma_icp_image_filter_horizontal(ctx_, img_, kernel.data(), (int)kernel.size(), o); });
    }
    DeviceImage Flip() const { return make("visma_icp_image_flip", [&](visma_icp_image **o) { return visma_icp_image_flip(ctx_, img_, o); }); }
    DeviceImage Downsample() const { return make("visma_icp_image_downsample", [&](visma_icp_image **o) { return visma_icp_image_downsample(ctx_, img_, o); }); }
    DeviceImage Dilate(int half_kernel_size = 1) const
    {
        return make("visma_icp_image_dilate", [&](visma_icp_image **o) { return visma_icp_image_dilate(ctx_, img_, half_kernel_size, o); });
    }
    DeviceImage Copy() const { return make("visma_icp_image_copy", [&](visma_icp_image **o) { return visma_icp_image_copy(ctx_, img_, o); }); }
    DeviceImage &LinearTransform(double scale = 1.0, double offset = 0.0)
    {
        if (img_) detail::check(ctx_, visma_icp_image_linear_transform(ctx_, img_, scale, offset), "visma_icp_image_linear_transform");
        return *this;
    }
    DeviceImage &ClipIntensity(double min = 0.0, double max = 1.0)
    {
        if (img_) detail::check(ctx_, visma_icp_image_clip_intensity(ctx_, img_, min, max), "visma_icp_image_clip_intensity");
        return *this;
    }
    std::vector<DeviceImage> Pyramid(size_t num_of_levels, bool with_gaussian_filter = true) const
    {
        std::vector<visma_icp_image *> h(num_of_levels, nullptr);
        if (img_) detail::check(ctx_, visma_icp_image_pyramid(ctx_, img_, (int)num_of_levels, with_gaussian_filter ? 1 : 0, h.data()), "visma_icp_image_pyramid");
        std::vector<DeviceImage> out;
        for (visma_icp_image *i : h)
            if (i) out.emplace_back(ctx_, i);
        return out;
    }
    // CreateRGBDImageFrom*: -> (color, depth); two empty DeviceImages for images of different sizes
    static std::pair<DeviceImage, DeviceImage> RGBD(const DeviceImage &color, const DeviceImage &depth, int format, double depth_scale = 1000.0,
                                                    double depth_trunc = 3.0, bool convert_rgb_to_intensity = true)
    {
        visma_icp_image *c = nullptr, *d = nullptr;
        detail::check(color.ctx_, visma_icp_image_rgbd(color.ctx_, color.img_, depth.img_, format, depth_scale, depth_trunc, convert_rgb_to_intensity ? 1 : 0, &c, &d),
                      "visma_icp_image_rgbd");
        return std::pair<DeviceImage, DeviceImage>(DeviceImage(color.ctx_, c), DeviceImage(color.ctx_, d));
    }

private:
    template <class F>
    DeviceImage make(const char *what, F f) const
    {
        visma_icp_image *o = nullptr;
        if (img_) detail::check(ctx_, f(&o), what);
        return DeviceImage(ctx_, o);
    }
    visma_icp_ctx *ctx_;
    visma_icp_image *img_ = nullptr;
};

// ComputeRGBDOdometry of four resident 1 x float images (the gray and the depth of the source and of the target)
inline std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d> ComputeRGBDOdometry(
        const DeviceImage &source_color, const DeviceImage &source_depth, const DeviceImage &target_color, const DeviceImage &target_depth,
        const PinholeCameraIntrinsic &pinhole_camera_intrinsic, const Eigen::Matrix4d &odo_init = Eigen::Matrix4d::Identity(),
        const RGBDOdometryJacobian &jacobian_method = RGBDOdometryJacobianFromHybridTerm(), const OdometryOption &option = OdometryOption())
{
    typedef std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d> Out;
    visma_icp_ctx *ctx = source_color.Context();
    visma_icp_odometry_option opt;
    visma_icp_odometry_option_default(&opt);
    opt.n_levels = (int)option.iteration_number_per_pyramid_level_.size();
    for (int l = 0; l < opt.n_levels && l < VISMA_ICP_ODOMETRY_MAX_LEVELS; l++) opt.iterations[l] = option.iteration_number_per_pyramid_level_[l];
    opt.max_depth_diff = option.max_depth_diff_; opt.min_depth = option.min_depth_; opt.max_depth = option.max_depth_;
    const Eigen::Matrix3d &K = pinhole_camera_intrinsic.intrinsic_matrix_;
    const double k[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    const int method = typeid(jacobian_method) == typeid(RGBDOdometryJacobianFromColorTerm) ? VISMA_ICP_ODOMETRY_COLOR : VISMA_ICP_ODOMETRY_HYBRID;
    double init[16], T[16], info[36];
    detail::to_rowmajor(odo_init, init);
    visma_icp_odometry_result res = {};
    detail::check(ctx, visma_icp_rgbd_odometry_images(ctx, source_color.Handle(), source_depth.Handle(), target_color.Handle(), target_depth.Handle(), k,
                                                      init, method, &opt, T, info, &res), "visma_icp_rgbd_odometry_images");
    if (!res.success) return Out(false, Eigen::Matrix4d::Identity(), Eigen::Matrix6d::Zero());
    Eigen::Matrix4d Tm;
    Eigen::Matrix6d Im;
    for (int i = 0; i < 16; i++) Tm(i / 4, i % 4) = T[i];
    for (int i = 0; i < 36; i++) Im(i / 6, i % 6) = info[i];
    return Out(true, Tm, Im);
}

// The mesh seen through a pinhole camera (visma_icp_render has the rule): the metric depth (0 where nothing is drawn), or
// OpenGL's depth-buffer value (1 where nothing is drawn), as a resident 1 x float image: what cloud_from_depth_image,
// Integrate and ComputeRGBDOdometry of DeviceImages take, so volume -> mesh -> depth -> cloud / volume / odometry runs
// without a host round trip.  index, mask: where given, the visible triangle (1 x int32, -1) and the mask (1 x uint8)
inline DeviceImage RenderDepth(const DeviceTriangleMesh &mesh, const PinholeCameraIntrinsic &intrinsic, const Eigen::Matrix4d &extrinsic,
                               double z_near = 0.05, double z_far = 10.0, bool depth_buffer = false, DeviceImage *index = nullptr,
                               DeviceImage *mask = nullptr)
{
    const Eigen::Matrix3d &K = intrinsic.intrinsic_matrix_;
    const double k[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    double E[16];
    detail::to_rowmajor(extrinsic, E);
    visma_icp_ctx *ctx = mesh.context();
    visma_icp_image *d = nullptr, *i = nullptr, *m = nullptr;
    const int rc = visma_icp_render(ctx, mesh.handle(), intrinsic.width_, intrinsic.height_, k, E, z_near, z_far,
                                    depth_buffer ? VISMA_ICP_RENDER_DEPTH_BUFFER : VISMA_ICP_RENDER_METRIC, &d, index ? &i : nullptr,
                                    mask ? &m : nullptr);
    if (rc == VISMA_ICP_ERR_INVALID) throw std::invalid_argument(std::string("[RenderDepth] ") + visma_icp_last_error(ctx));
    detail::check(ctx, rc, "visma_icp_render");
    if (index) *index = DeviceImage(ctx, i);
    if (mask) *mask = DeviceImage(ctx, m);
    return DeviceImage(ctx, d);
}

// the depth-edge image (edge_detection.frag's rule) of a resident metric depth
inline DeviceImage RenderEdges(const DeviceImage &depth)
{
    visma_icp_image *e = nullptr;
    const int rc = visma_icp_render_edges(depth.Context(), depth.Handle(), &e);
    if (rc == VISMA_ICP_ERR_INVALID) throw std::invalid_argument(std::string("[RenderEdges] ") + visma_icp_last_error(depth.Context()));
    detail::check(depth.Context(), rc, "visma_icp_render_edges");
    return DeviceImage(depth.Context(), e);
}

}  // namespace cicp

inline void TSDFVolume::Integrate(const cicp::DeviceImage &depth, const cicp::DeviceImage *color, const PinholeCameraIntrinsic &intrinsic,
                                  const Eigen::Matrix4d &extrinsic)
{
    const Eigen::Matrix3d &K = intrinsic.intrinsic_matrix_;
    const double k[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    double E[16];
    cicp::detail::to_rowmajor(extrinsic, E);
    const int rc = visma_icp_tsdf_integrate_images(Context(), Handle(), depth.Handle(), color ? color->Handle() : nullptr, k, intrinsic.width_,
                                                   intrinsic.height_, E);
    if (rc == VISMA_ICP_ERR_INVALID) throw std::invalid_argument(std::string("[TSDFVolume::Integrate] ") + visma_icp_last_error(Context()));
    cicp::detail::check(Context(), rc, "visma_icp_tsdf_integrate_images");
}

// the stock names: one upload, the operation, one download, on this thread's context
inline std::shared_ptr<Image> CreateDepthToCameraDistanceMultiplierFloatImage(const PinholeCameraIntrinsic &intrinsic)
{
    visma_icp_ctx *ctx = cicp::detail::ThreadContext::instance().get();
    const Eigen::Matrix3d &K = intrinsic.intrinsic_matrix_;
    const double k[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    visma_icp_image *o = nullptr;
    cicp::detail::check(ctx, visma_icp_image_distance_multiplier(ctx, k, intrinsic.width_, intrinsic.height_, &o), "visma_icp_image_distance_multiplier");
    return cicp::DeviceImage(ctx, o).Download();
}
template <typename T>
std::shared_ptr<Image> CreateImageFromFloatImage(const Image &input)
{
    static_assert(sizeof(T) == 1 || sizeof(T) == 2, "uint8_t or uint16_t");
    return cicp::DeviceImage(input).FromFloat((int)sizeof(T)).Download();
}
inline std::shared_ptr<Image> FlipImage(const Image &input) { return cicp::DeviceImage(input).Flip().Download(); }
inline std::shared_ptr<Image> FilterImage(const Image &input, Image::FilterType type) { return cicp::DeviceImage(input).Filter(type).Download(); }
inline std::shared_ptr<Image> FilterImage(const Image &input, const std::vector<double> &dx, const std::vector<double> &dy)
{
    return cicp::DeviceImage(input).Filter(dx, dy).Download();
}
inline std::shared_ptr<Image> FilterHorizontalImage(const Image &input, const std::vector<double> &kernel)
{
    return cicp::DeviceImage(input).FilterHorizontal(kernel).Download();
}
inline std::shared_ptr<Image> DownsampleImage(const Image &input) { return cicp::DeviceImage(input).Downsample().Download(); }
inline std::shared_ptr<Image> DilateImage(const Image &input, int half_kernel_size) { return cicp::DeviceImage(input).Dilate(half_kernel_size).Download(); }
inline void LinearTransformImage(Image &input, double scale, double offset) { input = *cicp::DeviceImage(input).LinearTransform(scale, offset).Download(); }
inline void ClipIntensityImage(Image &input, double min, double max) { input = *cicp::DeviceImage(input).ClipIntensity(min, max).Download(); }
inline ImagePyramid FilterImagePyramid(const ImagePyramid &input, Image::FilterType type)
{
    ImagePyramid out;
    for (const auto &level : input) out.push_back(FilterImage(*level, type));
    return out;
}
inline ImagePyramid CreateImagePyramid(const Image &image, size_t num_of_levels, bool with_gaussian_filter)
{
    ImagePyramid out;
    for (const cicp::DeviceImage &level : cicp::DeviceImage(image).Pyramid(num_of_levels, with_gaussian_filter)) out.push_back(level.Download());
    return out;
}
namespace cicp {
namespace detail {
inline std::shared_ptr<RGBDImage> rgbd_format(const Image &color, const Image &depth, int format, bool convert_rgb_to_intensity)
{
    auto out = std::make_shared<RGBDImage>();
    if (color.height_ != depth.height_ || color.width_ != depth.width_) return out;
    DeviceImage c(color), d(depth);
    std::pair<DeviceImage, DeviceImage> p = DeviceImage::RGBD(c, d, format, 0.0, 0.0, convert_rgb_to_intensity);
    out->color_ = *p.first.Download();
    out->depth_ = *p.second.Download();
    return out;
}
}  // namespace detail
}  // namespace cicp
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromRedwoodFormat(const Image &color, const Image &depth, bool convert_rgb_to_intensity)
{
    return cicp::detail::rgbd_format(color, depth, VISMA_ICP_RGBD_REDWOOD, convert_rgb_to_intensity);
}
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromTUMFormat(const Image &color, const Image &depth, bool convert_rgb_to_intensity)
{
    return cicp::detail::rgbd_format(color, depth, VISMA_ICP_RGBD_TUM, convert_rgb_to_intensity);
}
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromSUNFormat(const Image &color, const Image &depth, bool convert_rgb_to_intensity)
{
    return cicp::detail::rgbd_format(color, depth, VISMA_ICP_RGBD_SUN, convert_rgb_to_intensity);
}
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromNYUFormat(const Image &color, const Image &depth, bool convert_rgb_to_intensity)
{
    return cicp::detail::rgbd_format(color, depth, VISMA_ICP_RGBD_NYU, convert_rgb_to_intensity);
}
inline RGBDImagePyramid FilterRGBDImagePyramid(const RGBDImagePyramid &rgbd_image_pyramid, Image::FilterType type)
{
    RGBDImagePyramid out;
    for (const auto &level : rgbd_image_pyramid)
        out.push_back(std::make_shared<RGBDImage>(*FilterImage(level->color_, type), *FilterImage(level->depth_, type)));
    return out;
}
// (like the reference, this needs both images to be 1 x float: an image without levels has none to pair)
inline RGBDImagePyramid CreateRGBDImagePyramid(const RGBDImage &rgbd_image, size_t num_of_levels, bool with_gaussian_filter_for_color,
                                               bool with_gaussian_filter_for_depth)
{
    const ImagePyramid color = CreateImagePyramid(rgbd_image.color_, num_of_levels, with_gaussian_filter_for_color);
    const ImagePyramid depth = CreateImagePyramid(rgbd_image.depth_, num_of_levels, with_gaussian_filter_for_depth);
    RGBDImagePyramid out;
    for (size_t l = 0; l < num_of_levels && l < color.size() && l < depth.size(); l++) out.push_back(std::make_shared<RGBDImage>(*color[l], *depth[l]));
    return out;
}
#endif

}  // namespace open3d
