// Core/Registration/GlobalOptimizationMethod.h -- the two methods of the pose-graph optimisation (shape of
// O3D/Core/Registration/GlobalOptimizationMethod.h:31-78).  OptimizePoseGraph is ONE optimisation (no validation, no
// pruning, no compensation): what GlobalOptimization() runs twice.  Defined in visma_icp_open3d.hpp.
#pragma once

namespace open3d {

class PoseGraph;
class GlobalOptimizationOption;
class GlobalOptimizationConvergenceCriteria;

class GlobalOptimizationMethod {
public:
    GlobalOptimizationMethod() {}
    virtual ~GlobalOptimizationMethod() {}
    virtual void OptimizePoseGraph(PoseGraph &pose_graph, const GlobalOptimizationConvergenceCriteria &criteria,
                                   const GlobalOptimizationOption &option) const = 0;
};

class GlobalOptimizationGaussNewton : public GlobalOptimizationMethod {
public:
    GlobalOptimizationGaussNewton() {}
    ~GlobalOptimizationGaussNewton() override {}
    inline void OptimizePoseGraph(PoseGraph &pose_graph, const GlobalOptimizationConvergenceCriteria &criteria,
                                  const GlobalOptimizationOption &option) const override;
};

class GlobalOptimizationLevenbergMarquardt : public GlobalOptimizationMethod {
public:
    GlobalOptimizationLevenbergMarquardt() {}
    ~GlobalOptimizationLevenbergMarquardt() override {}
    inline void OptimizePoseGraph(PoseGraph &pose_graph, const GlobalOptimizationConvergenceCriteria &criteria,
                                  const GlobalOptimizationOption &option) const override;
};

}  // namespace open3d
