// Core/Odometry/RGBDOdometryJacobian.h -- which rows an RGB-D odometry step is built from (shape of
// O3D/Core/Odometry/RGBDOdometryJacobian.h).  The rows themselves are computed on the GPU (visma_icp.h); these classes
// are tags: cicp::ComputeRGBDOdometry selects the method by the type it is handed.
#pragma once

namespace open3d {

class RGBDOdometryJacobian {
public:
    virtual ~RGBDOdometryJacobian() {}
};

// the photometric row alone (Steinbruecker, Sturm, Cremers 2011)
class RGBDOdometryJacobianFromColorTerm : public RGBDOdometryJacobian {};

// a photometric and a depth row per pair (Park, Zhou, Koltun 2017)
class RGBDOdometryJacobianFromHybridTerm : public RGBDOdometryJacobian {};

}  // namespace open3d
