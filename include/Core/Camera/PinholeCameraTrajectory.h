// Core/Camera/PinholeCameraTrajectory.h -- one intrinsic and a world -> camera extrinsic per frame (shape of
// O3D/Core/Camera/PinholeCameraTrajectory.h, without its JSON conversion).  Stand-alone and header-only.
#pragma once
#include <Eigen/Core>
#include <Eigen/StdVector>
#include <vector>

#include "PinholeCameraIntrinsic.h"

namespace open3d {

class PinholeCameraTrajectory {
public:
    PinholeCameraTrajectory() {}
    virtual ~PinholeCameraTrajectory() {}

    PinholeCameraIntrinsic intrinsic_;
    std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> extrinsic_;
};

}  // namespace open3d
