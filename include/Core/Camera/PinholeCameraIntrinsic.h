// Core/Camera/PinholeCameraIntrinsic.h -- image size and the 3 x 3 camera matrix (shape of
// O3D/Core/Camera/PinholeCameraIntrinsic.h, without its JSON conversion).  Stand-alone and header-only.
#pragma once

#include <utility>

#include <Eigen/Core>

namespace open3d {

class PinholeCameraIntrinsic {
public:
    PinholeCameraIntrinsic() : intrinsic_matrix_(Eigen::Matrix3d::Zero()) {}
    PinholeCameraIntrinsic(int width, int height, double fx, double fy, double cx, double cy) { SetIntrinsics(width, height, fx, fy, cx, cy); }

    void SetIntrinsics(int width, int height, double fx, double fy, double cx, double cy)
    {
        width_ = width; height_ = height;
        intrinsic_matrix_.setIdentity();
        intrinsic_matrix_(0, 0) = fx; intrinsic_matrix_(1, 1) = fy;
        intrinsic_matrix_(0, 2) = cx; intrinsic_matrix_(1, 2) = cy;
    }
    std::pair<double, double> GetFocalLength() const { return std::make_pair(intrinsic_matrix_(0, 0), intrinsic_matrix_(1, 1)); }
    std::pair<double, double> GetPrincipalPoint() const { return std::make_pair(intrinsic_matrix_(0, 2), intrinsic_matrix_(1, 2)); }
    double GetSkew() const { return intrinsic_matrix_(0, 1); }
    bool IsValid() const { return width_ > 0 && height_ > 0; }

    int width_ = -1;
    int height_ = -1;
    Eigen::Matrix3d intrinsic_matrix_;
};

}  // namespace open3d
