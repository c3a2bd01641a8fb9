// Core/Geometry/RGBDImage.h -- a colour (or intensity) image and the depth image registered to it (shape of
// O3D/Core/Geometry/RGBDImage.h).  Stand-alone and header-only.
#pragma once

#include <memory>

#include "Image.h"

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

}  // namespace open3d
