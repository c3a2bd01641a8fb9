// Core/Integration/UniformTSDFVolume.h -- a cube of resolution^3 voxels resident on the GPU (shape of
// O3D/Core/Integration/UniformTSDFVolume.h).  The methods are defined in visma_icp_open3d.hpp (visma_icp.h: the steps and
// the deviations from the reference).  The voxels live on the device: the reference's tsdf_, weight_ and color_ vectors
// are filled by Download() instead of being members that Integrate writes.
#pragma once

#include <vector>

#include "TSDFVolume.h"

struct visma_icp_ctx;
struct visma_icp_tsdf;

namespace open3d {

class UniformTSDFVolume : public TSDFVolume {
public:
    // on this thread's context (which the volume must not outlive) ...
    UniformTSDFVolume(double length, int resolution, double sdf_trunc, TSDFVolumeColorType color_type,
                      const Eigen::Vector3d &origin = Eigen::Vector3d::Zero());
    // ... or on a context of the caller's
    UniformTSDFVolume(visma_icp_ctx *ctx, double length, int resolution, double sdf_trunc, TSDFVolumeColorType color_type,
                      const Eigen::Vector3d &origin = Eigen::Vector3d::Zero());
    ~UniformTSDFVolume() override;
    UniformTSDFVolume(const UniformTSDFVolume &) = delete;
    UniformTSDFVolume &operator=(const UniformTSDFVolume &) = delete;

    void Reset() override;
    void Integrate(const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic, const Eigen::Matrix4d &extrinsic) override;
    using TSDFVolume::Integrate;                         // ... and of cicp::DeviceImages
    std::shared_ptr<PointCloud> ExtractPointCloud() override;
    std::shared_ptr<TriangleMesh> ExtractTriangleMesh() override;
    visma_icp_ctx *Context() const override { return ctx_; }
    visma_icp_tsdf *Handle() const override { return volume_; }
    // every voxel with a weight and a tsdf in [-0.98, 0.98): its centre, coloured (tsdf + 1) / 2
    std::shared_ptr<PointCloud> ExtractVoxelPointCloud();
    // the reference's tsdf_, weight_ (voxel_num_ floats) and color_ (voxel_num_ entries, empty without colour)
    void Download(std::vector<float> &tsdf, std::vector<float> &weight, std::vector<Eigen::Vector3f> &color) const;

    inline int IndexOf(int x, int y, int z) const { return x * resolution_ * resolution_ + y * resolution_ + z; }
    inline int IndexOf(const Eigen::Vector3i &xyz) const { return IndexOf(xyz(0), xyz(1), xyz(2)); }

    Eigen::Vector3d origin_;
    double length_;
    int resolution_;
    int voxel_num_;

private:
    void Create(visma_icp_ctx *ctx);
    visma_icp_ctx *ctx_ = nullptr;
    visma_icp_tsdf *volume_ = nullptr;
};

}  // namespace open3d
