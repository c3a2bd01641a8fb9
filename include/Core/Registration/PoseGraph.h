// Core/Registration/PoseGraph.h -- nodes and edges of a pose graph (shape of O3D/Core/Registration/PoseGraph.h:37-101),
// written here: no JSON base class, reading and writing pose-graph JSON is not part of this library.
#pragma once

#include <vector>

#include <Eigen/Core>

#include "../Utility/Eigen.h"

namespace open3d {

class PoseGraphNode {
public:
    PoseGraphNode(const Eigen::Matrix4d &pose = Eigen::Matrix4d::Identity()) : pose_(pose) {}

    Eigen::Matrix4d pose_;                      // node to world
};

class PoseGraphEdge {
public:
    PoseGraphEdge(int source_node_id = -1, int target_node_id = -1,
                  const Eigen::Matrix4d &transformation = Eigen::Matrix4d::Identity(),
                  const Eigen::Matrix6d &information = Eigen::Matrix6d::Identity(), bool uncertain = false,
                  double confidence = 1.0)
        : source_node_id_(source_node_id), target_node_id_(target_node_id), transformation_(transformation),
          information_(information), uncertain_(uncertain), confidence_(confidence) {}

    int source_node_id_;
    int target_node_id_;
    Eigen::Matrix4d transformation_;            // maps the source node's cloud onto the target node's
    Eigen::Matrix6d information_;               // GetInformationMatrixFromPointClouds
    bool uncertain_;                            // odometry edges: false; loop closures: true
    double confidence_;                         // the line-process value in [0, 1] of an uncertain edge
};

class PoseGraph {
public:
    std::vector<PoseGraphNode> nodes_;
    std::vector<PoseGraphEdge> edges_;
};

}  // namespace open3d
