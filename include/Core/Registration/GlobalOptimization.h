// Core/Registration/GlobalOptimization.h -- the pose-graph optimisation of multiway registration (shape of
// O3D/Core/Registration/GlobalOptimization.h:29-64; Choi, Zhou, Koltun, CVPR 2015).  Defined in visma_icp_open3d.hpp.
#pragma once

#include <memory>

#include "GlobalOptimizationConvergenceCriteria.h"
#include "GlobalOptimizationMethod.h"
#include "PoseGraph.h"

namespace open3d {

// validation, optimisation, pruning of the uncertain edges below option.edge_prune_threshold_, optimisation, compensation
// of option.reference_node_; an invalid graph (consecutive nodes without an edge, an edge naming no node) is left as it is
inline void GlobalOptimization(PoseGraph &pose_graph,
                               const GlobalOptimizationMethod &method = GlobalOptimizationLevenbergMarquardt(),
                               const GlobalOptimizationConvergenceCriteria &criteria = GlobalOptimizationConvergenceCriteria(),
                               const GlobalOptimizationOption &option = GlobalOptimizationOption());

inline std::shared_ptr<PoseGraph> CreatePoseGraphWithoutInvalidEdges(const PoseGraph &pose_graph,
                                                                     const GlobalOptimizationOption &option);

}  // namespace open3d
