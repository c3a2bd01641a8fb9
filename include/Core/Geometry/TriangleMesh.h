// Core/Geometry/TriangleMesh.h -- the data carrier of a triangle mesh (shape of O3D/Core/Geometry/TriangleMesh.h: AoS f64
// vertices, normals and colours, int triangles).  Minimal: what ExtractTriangleMesh fills and color map optimization reads and writes.  Stand-alone and
// header-only.
#pragma once
#include <Eigen/Core>
#include <vector>

namespace open3d {

class TriangleMesh {
public:
    TriangleMesh() {}
    virtual ~TriangleMesh() {}

    void Clear() { vertices_.clear(); vertex_normals_.clear(); vertex_colors_.clear(); triangles_.clear(); }
    bool IsEmpty() const { return !HasVertices(); }
    bool HasVertices() const { return vertices_.size() > 0; }
    bool HasTriangles() const { return vertices_.size() > 0 && triangles_.size() > 0; }
    bool HasVertexNormals() const { return vertices_.size() > 0 && vertex_normals_.size() == vertices_.size(); }
    bool HasVertexColors() const { return vertices_.size() > 0 && vertex_colors_.size() == vertices_.size(); }

    std::vector<Eigen::Vector3d> vertices_;
    std::vector<Eigen::Vector3d> vertex_normals_;
    std::vector<Eigen::Vector3d> vertex_colors_;
    std::vector<Eigen::Vector3i> triangles_;
};

}  // namespace open3d
