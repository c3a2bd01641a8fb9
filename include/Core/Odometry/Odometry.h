// Core/Odometry/Odometry.h -- RGB-D odometry between two frames (shape of O3D/Core/Odometry/Odometry.h).  Defined in
// visma_icp_open3d.hpp, on the GPU (visma_icp.h: the steps and the deviations from the reference).
#pragma once

#include <tuple>

#include <Eigen/Core>

#include "../Camera/PinholeCameraIntrinsic.h"
#include "../Geometry/RGBDImage.h"
#include "../Utility/Eigen.h"
#include "OdometryOption.h"
#include "RGBDOdometryJacobian.h"

namespace open3d {

// -> (success, the 4 x 4 pose source camera -> target camera, the 6 x 6 information matrix of that edge); images that are
// not four single-channel float images of one size, or a run without a solution: (false, I, 0)
inline std::tuple<bool, Eigen::Matrix4d, Eigen::Matrix6d> ComputeRGBDOdometry(
        const RGBDImage &source, const RGBDImage &target, const PinholeCameraIntrinsic &pinhole_camera_intrinsic = PinholeCameraIntrinsic(),
        const Eigen::Matrix4d &odo_init = Eigen::Matrix4d::Identity(),
        const RGBDOdometryJacobian &jacobian_method = RGBDOdometryJacobianFromHybridTerm(), const OdometryOption &option = OdometryOption());

}  // namespace open3d
