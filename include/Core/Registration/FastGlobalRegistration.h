// Core/Registration/FastGlobalRegistration.h -- the options of fast global registration and its entry point
// (shape of O3D/Core/Registration/FastGlobalRegistration.h:41-78).  Unlike the reference's constructor this one
// initialises every member, decrease_mu_ and maximum_correspondence_distance_ included.
#pragma once

#include <Eigen/Core>

namespace open3d {

class PointCloud;
class Feature;
class RegistrationResult;

class FastGlobalRegistrationOption {
public:
    FastGlobalRegistrationOption(double division_factor = 1.4, bool use_absolute_scale = false, bool decrease_mu = true,
                                 double maximum_correspondence_distance = 0.025, int iteration_number = 64,
                                 double tuple_scale = 0.95, int maximum_tuple_count = 1000)
        : division_factor_(division_factor), use_absolute_scale_(use_absolute_scale), decrease_mu_(decrease_mu),
          maximum_correspondence_distance_(maximum_correspondence_distance), iteration_number_(iteration_number),
          tuple_scale_(tuple_scale), maximum_tuple_count_(maximum_tuple_count) {}

    double division_factor_;                    // graduated non-convexity: par /= division_factor_
    bool use_absolute_scale_;                   // distances in the clouds' own units instead of relative to their extent
    bool decrease_mu_;
    double maximum_correspondence_distance_;    // where par stops decreasing
    int iteration_number_;
    double tuple_scale_;                        // edge ratios of a tuple lie inside (tuple_scale_, 1 / tuple_scale_)
    int maximum_tuple_count_;
};

inline RegistrationResult FastGlobalRegistration(const PointCloud &source, const PointCloud &target, const Feature &source_feature,
                                                 const Feature &target_feature,
                                                 const FastGlobalRegistrationOption &option = FastGlobalRegistrationOption());

}  // namespace open3d
