// Core/Geometry/PointCloud.h -- the data carrier of the path
// (shape of O3D/Core/Geometry/PointCloud.h:42-89: AoS f64 points/normals/colors).
#pragma once
#include <Eigen/Core>
#include <cmath>
#include <memory>
#include <tuple>
#include <vector>

#include "KDTreeSearchParam.h"

namespace open3d {

class PointCloud {
public:
    PointCloud() {}
    virtual ~PointCloud() {}

    void Clear() { points_.clear(); normals_.clear(); colors_.clear(); }
    bool IsEmpty() const { return !HasPoints(); }
    bool HasPoints() const { return points_.size() > 0; }
    bool HasNormals() const { return points_.size() > 0 && normals_.size() == points_.size(); }
    bool HasColors() const { return points_.size() > 0 && colors_.size() == points_.size(); }

    // (0, 0, 0) for a cloud without points; a NaN coordinate is never smaller or larger than another (the first point's
    // stays where it is one); among equal values the first stays (O3D/Core/Geometry/PointCloud.cpp:47-73)
    Eigen::Vector3d GetMinBound() const { return Bound(false); }
    Eigen::Vector3d GetMaxBound() const { return Bound(true); }

    // Eigen 3.3's normalize() per normal, written out (z = squaredNorm(); if (z > 0) n /= sqrt(z)): a zero or NaN normal stays
    void NormalizeNormals()
    {
        for (auto &n : normals_) {
            const double z = (n(0) * n(0) + n(1) * n(1)) + n(2) * n(2);
            if (z > 0.0) {
                const double len = std::sqrt(z);
                n = Eigen::Vector3d(n(0) / len, n(1) / len, n(2) / len);
            }
        }
    }

    void PaintUniformColor(const Eigen::Vector3d &color) { colors_.assign(points_.size(), color); }

    // Rigid/affine motion of points (w = 1) and normals (w = 0); the 4th row of
    // the matrix is ignored, as pinned by the reference's PointCloud.Transform test.
    void Transform(const Eigen::Matrix4d &T)
    {
        for (auto &p : points_) {
            const Eigen::Vector3d q = T.block<3, 3>(0, 0) * p + T.block<3, 1>(0, 3);
            p = q;
        }
        for (auto &n : normals_) {
            const Eigen::Vector3d m = T.block<3, 3>(0, 0) * n;
            n = m;
        }
    }

    PointCloud &operator+=(const PointCloud &o)
    {
        const bool keep_n = (!HasPoints() || HasNormals()) && o.HasNormals();
        const bool keep_c = (!HasPoints() || HasColors()) && o.HasColors();
        if (!keep_n) normals_.clear(); else normals_.insert(normals_.end(), o.normals_.begin(), o.normals_.end());
        if (!keep_c) colors_.clear(); else colors_.insert(colors_.end(), o.colors_.begin(), o.colors_.end());
        points_.insert(points_.end(), o.points_.begin(), o.points_.end());
        return *this;
    }
    PointCloud operator+(const PointCloud &o) const { return PointCloud(*this) += o; }

    std::vector<Eigen::Vector3d> points_;
    std::vector<Eigen::Vector3d> normals_;
    std::vector<Eigen::Vector3d> colors_;

private:
    Eigen::Vector3d Bound(bool upper) const
    {
        if (!HasPoints()) return Eigen::Vector3d(0.0, 0.0, 0.0);
        Eigen::Vector3d b = points_[0];
        for (const auto &p : points_)
            for (int k = 0; k < 3; k++)
                if (upper ? b(k) < p(k) : p(k) < b(k)) b(k) = p(k);
        return b;
    }
};

/// The rows at `indices`, in their order, with normals and colours (shape of O3D/Core/Geometry/PointCloud.h:119-120); on the
/// GPU, in visma_icp_open3d.hpp, as are the four below.  An index outside [0, points_.size()) throws std::runtime_error
/// where the reference reads out of bounds.
inline std::shared_ptr<PointCloud> SelectDownSample(const PointCloud &input, const std::vector<size_t> &indices);
/// The rows 0, k, 2k, ...; an empty cloud for k == 0 (:131-132)
inline std::shared_ptr<PointCloud> UniformDownSample(const PointCloud &input, size_t every_k_points);
/// The points with min_bound <= p <= max_bound in every component, in their order (:137-138)
inline std::shared_ptr<PointCloud> CropPointCloud(const PointCloud &input, const Eigen::Vector3d &min_bound,
                                                  const Eigen::Vector3d &max_bound);
/// (:169-178) The sums run over chunks of 16,384 points: up to that many the reference's result bit for bit, beyond it
/// equal but for the last bits (visma_icp.h, "PointCloud": mean_and_covariance)
inline std::tuple<Eigen::Vector3d, Eigen::Matrix3d> ComputePointCloudMeanAndCovariance(const PointCloud &input);
inline std::vector<double> ComputePointCloudMahalanobisDistance(const PointCloud &input);

/// Down-sample with a voxel grid (shape of O3D/Core/Geometry/PointCloud.h:101-105);
/// implemented on the GPU in visma_icp_open3d.hpp.
inline std::shared_ptr<PointCloud> VoxelDownSample(const PointCloud &input, double voxel_size);

/// Normals from the covariance of each point's neighbours (shape of
/// O3D/Core/Geometry/PointCloud.h:140-146); on the GPU, in visma_icp_open3d.hpp.  Existing normals
/// keep their sign.
inline bool EstimateNormals(PointCloud &cloud, const KDTreeSearchParam &search_param = KDTreeSearchParamKNN());
/// (O3D/Core/Geometry/PointCloud.h:148-158) host loops, in visma_icp_open3d.hpp
inline bool OrientNormalsToAlignWithDirection(PointCloud &cloud,
                                              const Eigen::Vector3d &orientation_reference = Eigen::Vector3d(0.0, 0.0, 1.0));
inline bool OrientNormalsTowardsCameraLocation(PointCloud &cloud,
                                               const Eigen::Vector3d &camera_location = Eigen::Vector3d::Zero());
/// Distance of every source point to the nearest target point, and of every point to the nearest other point of its
/// cloud (shapes of O3D/Core/Geometry/PointCloud.h:161-167 and :180-183); on the GPU, in visma_icp_open3d.hpp.
inline std::vector<double> ComputePointCloudToPointCloudDistance(const PointCloud &source, const PointCloud &target);
inline std::vector<double> ComputePointCloudNearestNeighborDistance(const PointCloud &input);

}  // namespace open3d
