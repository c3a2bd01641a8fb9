// Core/Geometry/TriangleMesh.h -- a triangle mesh (shape of O3D/Core/Geometry/TriangleMesh.h: AoS f64 vertices, normals and
// colours, int triangles, f64 triangle normals).  What ExtractTriangleMesh fills, color map optimization reads and writes, and
// what ComputeVertexNormals, Purge, SelectDownSample and CropTriangleMesh work on.  Stand-alone and header-only.
//
// The members that only move or compare data (HasX, PaintUniformColor, GetMinBound / GetMaxBound, operator+=) are defined
// here and run on the host.  The members that compute -- NormalizeNormals, Transform, ComputeTriangleNormals,
// ComputeVertexNormals, Purge -- and the free functions SelectDownSample and CropTriangleMesh run on the GPU, on this
// thread's context (or, through open3d::cicp::, on a context of the caller's): they are defined in visma_icp_open3d.hpp and
// give the reference's results bit for bit (visma_icp.h, "TriangleMesh": the rules and the one deviation -- a triangle or
// selected index outside [0, vertices_.size()) throws, where the reference reads out of bounds).
#pragma once
#include <Eigen/Core>
#include <algorithm>
#include <memory>
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
    bool HasTriangleNormals() const { return HasTriangles() && triangles_.size() == triangle_normals_.size(); }

    // (0, 0, 0) for a mesh without vertices; a NaN coordinate is never smaller or larger than another (the first vertex's
    // stays where it is one)
    Eigen::Vector3d GetMinBound() const { return Bound(false); }
    Eigen::Vector3d GetMaxBound() const { return Bound(true); }

    void PaintUniformColor(const Eigen::Vector3d &color) { vertex_colors_.assign(vertices_.size(), color); }

    // the other mesh's rows behind this one's, its triangles shifted; an attribute survives only where both meshes have it
    // (or this one is empty)
    TriangleMesh &operator+=(const TriangleMesh &mesh)
    {
        if (mesh.IsEmpty()) return *this;
        const size_t nv = vertices_.size(), nt = triangles_.size();
        const bool keep_vn = (!HasVertices() || HasVertexNormals()) && mesh.HasVertexNormals();
        const bool keep_vc = (!HasVertices() || HasVertexColors()) && mesh.HasVertexColors();
        const bool keep_tn = (nt == 0 || triangle_normals_.size() == nt) && mesh.HasTriangleNormals();   // (asked once the vertices are in)
        Append(vertex_normals_, mesh.vertex_normals_, nv, keep_vn);
        Append(vertex_colors_, mesh.vertex_colors_, nv, keep_vc);
        Append(triangle_normals_, mesh.triangle_normals_, nt, keep_tn);
        vertices_.insert(vertices_.end(), mesh.vertices_.begin(), mesh.vertices_.end());
        const int shift = (int)nv;
        for (const auto &t : mesh.triangles_) triangles_.push_back(Eigen::Vector3i(t(0) + shift, t(1) + shift, t(2) + shift));
        return *this;
    }
    TriangleMesh operator+(const TriangleMesh &mesh) const { return TriangleMesh(*this) += mesh; }

    // on the GPU (visma_icp_open3d.hpp)
    void NormalizeNormals();
    void Transform(const Eigen::Matrix4d &transformation);
    void ComputeTriangleNormals(bool normalized = true);
    void ComputeVertexNormals(bool normalized = true);
    void Purge();

    std::vector<Eigen::Vector3d> vertices_;
    std::vector<Eigen::Vector3d> vertex_normals_;
    std::vector<Eigen::Vector3d> vertex_colors_;
    std::vector<Eigen::Vector3i> triangles_;
    std::vector<Eigen::Vector3d> triangle_normals_;

private:
    Eigen::Vector3d Bound(bool upper) const
    {
        if (!HasVertices()) return Eigen::Vector3d(0.0, 0.0, 0.0);
        Eigen::Vector3d b = vertices_[0];
        for (const auto &p : vertices_)
            for (int k = 0; k < 3; k++)
                if (upper ? b(k) < p(k) : p(k) < b(k)) b(k) = p(k);
        return b;
    }
    static void Append(std::vector<Eigen::Vector3d> &to, const std::vector<Eigen::Vector3d> &from, size_t rows, bool keep)
    {
        if (!keep) { to.clear(); return; }
        to.resize(rows);
        to.insert(to.end(), from.begin(), from.end());
    }
};

// the triangles whose three corners are among `indices`, the vertices they use, purged; on the GPU (visma_icp_open3d.hpp)
std::shared_ptr<TriangleMesh> SelectDownSample(const TriangleMesh &input, const std::vector<size_t> &indices);
// ... over the vertices with min_bound <= p <= max_bound in every component
std::shared_ptr<TriangleMesh> CropTriangleMesh(const TriangleMesh &input, const Eigen::Vector3d &min_bound, const Eigen::Vector3d &max_bound);

}  // namespace open3d
