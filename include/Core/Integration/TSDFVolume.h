// Core/Integration/TSDFVolume.h -- the interface of a truncated signed distance volume (shape of
// O3D/Core/Integration/TSDFVolume.h).  Stand-alone and header-only.
#pragma once

#include <memory>

#include <Eigen/Core>

#include "../Camera/PinholeCameraIntrinsic.h"
#include "../Geometry/PointCloud.h"
#include "../Geometry/RGBDImage.h"
#include "../Geometry/TriangleMesh.h"

struct visma_icp_ctx;
struct visma_icp_tsdf;

namespace open3d {

enum class TSDFVolumeColorType { None = 0, RGB8 = 1, Gray32 = 2 };

namespace cicp { class DeviceImage; }

class TSDFVolume {
public:
    TSDFVolume(double voxel_length, double sdf_trunc, TSDFVolumeColorType color_type)
        : voxel_length_(voxel_length), sdf_trunc_(sdf_trunc), color_type_(color_type) {}
    virtual ~TSDFVolume() {}

    virtual void Reset() = 0;
    // image: a float depth image (metres) and a colour image by color_type_ (RGB8: 3 x uint8, Gray32: 1 x float), both of
    // the intrinsic's size; extrinsic: world -> camera.  An image that does not fit throws std::invalid_argument (the
    // reference prints a warning and returns).
    virtual void Integrate(const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic, const Eigen::Matrix4d &extrinsic) = 0;
    // ... of images resident on the device (cicp::DeviceImage, visma_icp_open3d.hpp): no host copy; the same voxels.  color
    // may be NULL for a volume without colour
    void Integrate(const cicp::DeviceImage &depth, const cicp::DeviceImage *color, const PinholeCameraIntrinsic &intrinsic,
                   const Eigen::Matrix4d &extrinsic);
    virtual std::shared_ptr<PointCloud> ExtractPointCloud() = 0;
    // marching cubes: vertices_, vertex_colors_ (empty without colour) and triangles_.  The vertices and their colours are the
    // reference's; their order and the triangulation of a cube are this library's (visma_icp.h: THE ORDER, THE CASE RULE)
    virtual std::shared_ptr<TriangleMesh> ExtractTriangleMesh() = 0;
    // the resident volume's context and handle: what cicp::ExtractTriangleMesh(volume, purge, vertex_normals) and
    // cicp::DeviceTriangleMesh::FromVolume take the extracted mesh through WITHOUT a host copy (visma_icp_open3d.hpp)
    virtual visma_icp_ctx *Context() const = 0;
    virtual visma_icp_tsdf *Handle() const = 0;

    double voxel_length_;
    double sdf_trunc_;
    TSDFVolumeColorType color_type_;
};

}  // namespace open3d
