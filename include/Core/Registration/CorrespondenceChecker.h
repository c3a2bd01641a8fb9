// Core/Registration/CorrespondenceChecker.h -- the pruning checks of RANSAC global registration (shape of
// O3D/Core/Registration/CorrespondenceChecker.h:40-140, arithmetic of CorrespondenceChecker.cpp:35-89).  The RANSAC
// entry points run the three built-in classes on the GPU from their thresholds (visma_icp_open3d.hpp); Check() is the
// same test on the host for a caller that asks for it.
#pragma once
#include <Eigen/Core>
#include <cmath>

#include "../Geometry/PointCloud.h"
#include "TransformationEstimation.h"

namespace open3d {

class CorrespondenceChecker {
public:
    CorrespondenceChecker(bool require_pointcloud_alignment) : require_pointcloud_alignment_(require_pointcloud_alignment) {}
    virtual ~CorrespondenceChecker() {}
    virtual bool Check(const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres,
                       const Eigen::Matrix4d &transformation) const = 0;
    bool require_pointcloud_alignment_;     // false: checked before the transformation is estimated
};

// the lengths of every edge of the two point sets agree within the ratio similarity_threshold
class CorrespondenceCheckerBasedOnEdgeLength : public CorrespondenceChecker {
public:
    CorrespondenceCheckerBasedOnEdgeLength(double similarity_threshold = 0.9)
        : CorrespondenceChecker(false), similarity_threshold_(similarity_threshold) {}
    bool Check(const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres,
               const Eigen::Matrix4d &) const override
    {
        for (size_t i = 0; i < corres.size(); i++)
            for (size_t j = i + 1; j < corres.size(); j++) {
                const double ds = (source.points_[corres[i](0)] - source.points_[corres[j](0)]).norm();
                const double dt = (target.points_[corres[i](1)] - target.points_[corres[j](1)]).norm();
                if (ds < dt * similarity_threshold_ || dt < ds * similarity_threshold_) return false;
            }
        return true;
    }
    double similarity_threshold_;
};

// every aligned source point lies within distance_threshold of its target point
class CorrespondenceCheckerBasedOnDistance : public CorrespondenceChecker {
public:
    CorrespondenceCheckerBasedOnDistance(double distance_threshold)
        : CorrespondenceChecker(true), distance_threshold_(distance_threshold) {}
    bool Check(const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres,
               const Eigen::Matrix4d &T) const override
    {
        for (const auto &c : corres) {
            const Eigen::Vector3d &p = source.points_[c(0)];
            const Eigen::Vector3d moved = (T * Eigen::Vector4d(p(0), p(1), p(2), 1.0)).block<3, 1>(0, 0);
            if ((target.points_[c(1)] - moved).norm() > distance_threshold_) return false;
        }
        return true;
    }
    double distance_threshold_;
};

// every aligned source normal lies within normal_angle_threshold (radians) of its target normal
class CorrespondenceCheckerBasedOnNormal : public CorrespondenceChecker {
public:
    CorrespondenceCheckerBasedOnNormal(double normal_angle_threshold)
        : CorrespondenceChecker(true), normal_angle_threshold_(normal_angle_threshold) {}
    bool Check(const PointCloud &source, const PointCloud &target, const CorrespondenceSet &corres,
               const Eigen::Matrix4d &T) const override
    {
        if (!source.HasNormals() || !target.HasNormals()) return true;
        const double c0 = std::cos(normal_angle_threshold_);
        for (const auto &c : corres) {
            const Eigen::Vector3d &n = source.normals_[c(0)];
            const Eigen::Vector3d moved = (T * Eigen::Vector4d(n(0), n(1), n(2), 0.0)).block<3, 1>(0, 0);
            if (target.normals_[c(1)].dot(moved) < c0) return false;
        }
        return true;
    }
    double normal_angle_threshold_;
};

}  // namespace open3d
