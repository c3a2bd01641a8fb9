// Core/Geometry/RGBDImage.h -- a colour (or intensity) image and the depth image registered to it (shape of
// O3D/Core/Geometry/RGBDImage.h).  Stand-alone and header-only.
#pragma once

#include <memory>
#include <vector>

#include <Eigen/Core>

#include "../Camera/PinholeCameraIntrinsic.h"
#include "Image.h"
#include "PointCloud.h"

namespace open3d {

class RGBDImage {
public:
    RGBDImage() {}
    RGBDImage(const Image &color, const Image &depth) : color_(color), depth_(depth) {}

    Image color_;
    Image depth_;
};

// depth to metres as float (depth_scale units per metre; depth_trunc metres and beyond: no measurement), colour to one
// float intensity unless convert_rgb_to_intensity is false; images of different sizes: an empty RGBDImage
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromColorAndDepth(const Image &color, const Image &depth, double depth_scale = 1000.0,
                                                                   double depth_trunc = 3.0, bool convert_rgb_to_intensity = true)
{
    auto out = std::make_shared<RGBDImage>();
    if (color.height_ != depth.height_ || color.width_ != depth.width_) return out;
    out->depth_ = *ConvertDepthToFloatImage(depth, depth_scale, depth_trunc);
    out->color_ = convert_rgb_to_intensity ? *CreateFloatImageFromImage(color) : color;
    return out;
}

// The dataset factories (Redwood: 1000 units per metre, 4 m; TUM: 5000, 4 m; SUN: each 16-bit depth rotated right by 3 bits,
// then 1000, 7 m; NYU: bytes swapped, 351.3 / (1092.5 - d) m, then 1000, 7 m) and the RGB-D pyramids, on the GPU
// (visma_icp_open3d.hpp).  Unlike the reference, SUN and NYU leave the caller's depth image as it is (visma_icp.h).
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromRedwoodFormat(const Image &color, const Image &depth, bool convert_rgb_to_intensity = true);
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromTUMFormat(const Image &color, const Image &depth, bool convert_rgb_to_intensity = true);
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromSUNFormat(const Image &color, const Image &depth, bool convert_rgb_to_intensity = true);
inline std::shared_ptr<RGBDImage> CreateRGBDImageFromNYUFormat(const Image &color, const Image &depth, bool convert_rgb_to_intensity = true);
typedef std::vector<std::shared_ptr<RGBDImage>> RGBDImagePyramid;
inline RGBDImagePyramid FilterRGBDImagePyramid(const RGBDImagePyramid &rgbd_image_pyramid, Image::FilterType type);
inline RGBDImagePyramid CreateRGBDImagePyramid(const RGBDImage &rgbd_image, size_t num_of_levels, bool with_gaussian_filter_for_color = true,
                                               bool with_gaussian_filter_for_depth = false);

// The points behind a depth image (1 x float in metres, or 1 x uint16 in depth_scale units per metre cut at depth_trunc),
// every stride-th row and column, and behind an RGB-D image (float depth; colour 3 x uint8 or 1 x float) with their colours,
// in world coordinates: extrinsic^-1 ((u - cx) d / fx, (v - cy) d / fy, d), row-major pixel order (shapes of
// O3D/Core/Geometry/PointCloud.h:192-215).  Any other format: an empty cloud, as in the reference.  On the GPU, in
// visma_icp_open3d.hpp.
inline std::shared_ptr<PointCloud> CreatePointCloudFromDepthImage(const Image &depth, const PinholeCameraIntrinsic &intrinsic,
                                                                  const Eigen::Matrix4d &extrinsic = Eigen::Matrix4d::Identity(),
                                                                  double depth_scale = 1000.0, double depth_trunc = 1000.0, int stride = 1);
inline std::shared_ptr<PointCloud> CreatePointCloudFromRGBDImage(const RGBDImage &image, const PinholeCameraIntrinsic &intrinsic,
                                                                 const Eigen::Matrix4d &extrinsic = Eigen::Matrix4d::Identity());

}  // namespace open3d
