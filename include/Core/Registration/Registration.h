// Core/Registration/Registration.h -- criteria / result types and the
// RegistrationICP / RegistrationRANSAC... entry points of the path (shape of
// O3D/Core/Registration/Registration.h:46-129).  In this stand-alone header set
// open3d::RegistrationICP forwards to the MI355X driver
// open3d::cicp::RegistrationICP (visma_icp_open3d.hpp).
#pragma once
#include <Eigen/Core>
#include <functional>
#include <vector>

#include "TransformationEstimation.h"
#include "../Utility/Eigen.h"

namespace open3d {

class ICPConvergenceCriteria {
public:
    ICPConvergenceCriteria(double relative_fitness = 1e-6, double relative_rmse = 1e-6,
                           int max_iteration = 30)
        : relative_fitness_(relative_fitness), relative_rmse_(relative_rmse),
          max_iteration_(max_iteration) {}
    double relative_fitness_;
    double relative_rmse_;
    int max_iteration_;
};

// RANSAC stops after max_iteration_ trials or once max_validation_ of them have been validated (Registration.h:61-78)
class RANSACConvergenceCriteria {
public:
    RANSACConvergenceCriteria(int max_iteration = 1000, int max_validation = 1000)
        : max_iteration_(max_iteration), max_validation_(max_validation) {}
    int max_iteration_;
    int max_validation_;
};

class CorrespondenceChecker;
class Feature;

class RegistrationResult {
public:
    RegistrationResult(const Eigen::Matrix4d &transformation = Eigen::Matrix4d::Identity())
        : transformation_(transformation), inlier_rmse_(0.0), fitness_(0.0) {}
    Eigen::Matrix4d transformation_;
    CorrespondenceSet correspondence_set_;
    double inlier_rmse_;
    double fitness_;
};

inline RegistrationResult EvaluateRegistration(
    const PointCloud &source, const PointCloud &target, double max_correspondence_distance,
    const Eigen::Matrix4d &transformation = Eigen::Matrix4d::Identity());

inline RegistrationResult RegistrationICP(
    const PointCloud &source, const PointCloud &target, double max_correspondence_distance,
    const Eigen::Matrix4d &init = Eigen::Matrix4d::Identity(),
    const TransformationEstimation &estimation = TransformationEstimationPointToPoint(false),
    const ICPConvergenceCriteria &criteria = ICPConvergenceCriteria());

inline RegistrationResult RegistrationRANSACBasedOnCorrespondence(
    const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres, double max_correspondence_distance,
    const TransformationEstimation &estimation = TransformationEstimationPointToPoint(false), int ransac_n = 6,
    const RANSACConvergenceCriteria &criteria = RANSACConvergenceCriteria());

inline RegistrationResult RegistrationRANSACBasedOnFeatureMatching(
    const PointCloud &source, const PointCloud &target, const Feature &source_feature, const Feature &target_feature,
    double max_correspondence_distance, const TransformationEstimation &estimation = TransformationEstimationPointToPoint(false),
    int ransac_n = 4, const std::vector<std::reference_wrapper<const CorrespondenceChecker>> &checkers = {},
    const RANSACConvergenceCriteria &criteria = RANSACConvergenceCriteria());

// The information matrix of a pose-graph edge (Registration.h:132-135): sum G^T G over the pairs of a pass at
// `transformation` -- without the identity terms the reference adds (visma_icp.h states the deviation)
inline Eigen::Matrix6d GetInformationMatrixFromPointClouds(const PointCloud &source, const PointCloud &target,
                                                           double max_correspondence_distance,
                                                           const Eigen::Matrix4d &transformation);

}  // namespace open3d
