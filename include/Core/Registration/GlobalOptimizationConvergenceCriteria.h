// Core/Registration/GlobalOptimizationConvergenceCriteria.h -- the option and the stopping criteria of the pose-graph
// optimisation (shape and clamping of O3D/Core/Registration/GlobalOptimizationConvergenceCriteria.h:31-117).
#pragma once

namespace open3d {

class GlobalOptimizationOption {
public:
    GlobalOptimizationOption(double max_correspondence_distance = 0.075, double edge_prune_threshold = 0.25,
                             double preference_loop_closure = 1.0, int reference_node = -1)
        : max_correspondence_distance_(max_correspondence_distance < 0.0 ? 0.075 : max_correspondence_distance),
          edge_prune_threshold_(edge_prune_threshold < 0.0 || edge_prune_threshold > 1.0 ? 0.25 : edge_prune_threshold),
          preference_loop_closure_(preference_loop_closure < 0.0 ? 1.0 : preference_loop_closure),
          reference_node_(reference_node) {}

    double max_correspondence_distance_;        // the radius the information matrices were made with: sets the line-process weight
    double edge_prune_threshold_;               // an uncertain edge with confidence <= this is dropped
    double preference_loop_closure_;            // 0.1 for RGBD odometry, 2.0 for fragment registration
    int reference_node_;                        // the pose of this node is unchanged by the optimisation (-1: none)
};

class GlobalOptimizationConvergenceCriteria {
public:
    GlobalOptimizationConvergenceCriteria(int max_iteration = 100, double min_relative_increment = 1e-6,
                                          double min_relative_residual_increment = 1e-6, double min_right_term = 1e-6,
                                          double min_residual = 1e-6, int max_iteration_lm = 20,
                                          double upper_scale_factor = 2. / 3., double lower_scale_factor = 1. / 3.)
        : max_iteration_(max_iteration), min_relative_increment_(min_relative_increment),
          min_relative_residual_increment_(min_relative_residual_increment), min_right_term_(min_right_term),
          min_residual_(min_residual), max_iteration_lm_(max_iteration_lm),
          upper_scale_factor_(upper_scale_factor < 0.0 || upper_scale_factor > 1.0 ? 2. / 3. : upper_scale_factor),
          lower_scale_factor_(lower_scale_factor < 0.0 || lower_scale_factor > 1.0 ? 1. / 3. : lower_scale_factor) {}

    int max_iteration_;
    double min_relative_increment_;
    double min_relative_residual_increment_;
    double min_right_term_;
    double min_residual_;
    int max_iteration_lm_;                      // the inner loop of Levenberg-Marquardt
    double upper_scale_factor_;                 // lambda is scaled by a factor clamped to [lower, upper]
    double lower_scale_factor_;
};

}  // namespace open3d
