// Core/Integration/ScalableTSDFVolume.h -- volume units of volume_unit_resolution^3 voxels, opened where the frames' surfaces
// are, resident on the GPU (shape of O3D/Core/Integration/ScalableTSDFVolume.h).  The methods
// are defined in visma_icp_open3d.hpp (visma_icp.h: the steps, the unit pool and THE ORDER of the extractions, which is
// this library's definition: units in lexicographic order of their index, the reference's order within a unit).  The
// units live on the device: the reference's volume_units_ map is read through Units() and DownloadUnit().
#pragma once

#include <vector>

#include "TSDFVolume.h"

struct visma_icp_ctx;
struct visma_icp_tsdf;

namespace open3d {

class ScalableTSDFVolume : public TSDFVolume {
public:
    // on this thread's context (the volume must be destroyed on this thread, before the thread ends) ...
    ScalableTSDFVolume(double voxel_length, double sdf_trunc, TSDFVolumeColorType color_type, int volume_unit_resolution = 16,
                       int depth_sampling_stride = 4);
    // ... or on a context of the caller's (destroy the volume before the context); initial_units: the pool's first capacity
    ScalableTSDFVolume(visma_icp_ctx *ctx, double voxel_length, double sdf_trunc, TSDFVolumeColorType color_type,
                       int volume_unit_resolution = 16, int depth_sampling_stride = 4, int initial_units = 0);
    ~ScalableTSDFVolume() override;
    ScalableTSDFVolume(const ScalableTSDFVolume &) = delete;
    ScalableTSDFVolume &operator=(const ScalableTSDFVolume &) = delete;

    void Reset() override;
    void Integrate(const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic, const Eigen::Matrix4d &extrinsic) override;
    using TSDFVolume::Integrate;                         // ... and of cicp::DeviceImages
    std::shared_ptr<PointCloud> ExtractPointCloud() override;
    std::shared_ptr<TriangleMesh> ExtractTriangleMesh() override;
    visma_icp_ctx *Context() const override { return ctx_; }
    visma_icp_tsdf *Handle() const override { return volume_; }
    std::shared_ptr<PointCloud> ExtractVoxelPointCloud();
    // the indices of the open units, in lexicographic order
    std::vector<Eigen::Vector3i> Units() const;
    // the tsdf_, weight_ and color_ of the unit with that index (false: no such unit)
    bool DownloadUnit(const Eigen::Vector3i &index, std::vector<float> &tsdf, std::vector<float> &weight, std::vector<Eigen::Vector3f> &color) const;

    int volume_unit_resolution_;
    double volume_unit_length_;
    int depth_sampling_stride_;

private:
    visma_icp_ctx *ctx_ = nullptr;
    visma_icp_tsdf *volume_ = nullptr;
};

}  // namespace open3d
