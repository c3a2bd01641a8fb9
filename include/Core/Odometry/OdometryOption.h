// Core/Odometry/OdometryOption.h -- the options of RGB-D odometry (shape of O3D/Core/Odometry/OdometryOption.h).
#pragma once

#include <vector>

namespace open3d {

class OdometryOption {
public:
    // iterations per pyramid level, COARSEST level first (its length is the number of levels); pairs whose depths differ
    // by more than max_depth_diff are dropped; depth outside [min_depth, max_depth] is no measurement
    OdometryOption(const std::vector<int> &iteration_number_per_pyramid_level = {20, 10, 5}, double max_depth_diff = 0.03,
                   double min_depth = 0.0, double max_depth = 4.0)
        : iteration_number_per_pyramid_level_(iteration_number_per_pyramid_level), max_depth_diff_(max_depth_diff),
          min_depth_(min_depth), max_depth_(max_depth) {}

    std::vector<int> iteration_number_per_pyramid_level_;
    double max_depth_diff_;
    double min_depth_;
    double max_depth_;
};

}  // namespace open3d
