// Core/Geometry/Image.h -- the image type RGB-D odometry takes (shape of O3D/Core/Geometry/Image.h): a width, a height, a
// number of channels, bytes per channel and the pixel bytes, row-major.  Stand-alone and header-only: PrepareImage, PointerAt
// and the two conversions an odometry caller needs (any image -> single-channel float, a depth image -> metres); the
// filters and pyramids of the reference run on the GPU inside cicp::ComputeRGBDOdometry and are not offered as functions.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

namespace open3d {

class Image {
public:
    enum class ColorToIntensityConversionType { Equal, Weighted };

    void Clear() { width_ = height_ = num_of_channels_ = bytes_per_channel_ = 0; data_.clear(); }
    bool HasData() const { return width_ > 0 && height_ > 0 && data_.size() == size_t(height_ * BytesPerLine()); }
    bool IsEmpty() const { return !HasData(); }
    void PrepareImage(int width, int height, int num_of_channels, int bytes_per_channel)
    {
        width_ = width; height_ = height; num_of_channels_ = num_of_channels; bytes_per_channel_ = bytes_per_channel;
        data_.resize((size_t)width_ * height_ * num_of_channels_ * bytes_per_channel_);
    }
    int BytesPerLine() const { return width_ * num_of_channels_ * bytes_per_channel_; }

    int width_ = 0;
    int height_ = 0;
    int num_of_channels_ = 0;
    int bytes_per_channel_ = 0;
    std::vector<uint8_t> data_;
};

// the address of pixel (u, v) of a single-channel image, and of its channel ch
template <typename T>
T *PointerAt(const Image &image, int u, int v)
{
    return (T *)(image.data_.data() + ((size_t)v * image.width_ + u) * sizeof(T));
}
template <typename T>
T *PointerAt(const Image &image, int u, int v, int ch)
{
    return (T *)(image.data_.data() + (((size_t)v * image.width_ + u) * image.num_of_channels_ + ch) * sizeof(T));
}

// a single-channel float image of any 1- or 3-channel image with 1, 2 or 4 bytes per channel: 8-bit values over 255,
// 16-bit (read as uint16_t) and float values as they are; three channels of any of these widths by the mean (Equal) or by
// 0.299 R + 0.587 G + 0.114 B (Weighted).  Any other number of channels gives the all-zero image, as in the reference.
inline std::shared_ptr<Image> CreateFloatImageFromImage(
        const Image &image, Image::ColorToIntensityConversionType type = Image::ColorToIntensityConversionType::Weighted)
{
    auto out = std::make_shared<Image>();
    if (image.IsEmpty()) return out;
    out->PrepareImage(image.width_, image.height_, 1, 4);
    const bool equal = type == Image::ColorToIntensityConversionType::Equal;
    const int b = image.bytes_per_channel_, nc = image.num_of_channels_;
    float *o = (float *)out->data_.data();
    for (size_t i = 0; i < (size_t)image.width_ * image.height_; i++) {
        const uint8_t *p = image.data_.data() + i * nc * b;
        float c[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < nc && k < 3; k++)
            c[k] = b == 1 ? (float)p[k] : b == 2 ? (float)((const uint16_t *)p)[k] : ((const float *)p)[k];
        float v = 0.0f;
        if (nc == 1) v = c[0];
        else if (nc == 3) v = equal ? (c[0] + c[1] + c[2]) / 3.0f : 0.2990f * c[0] + 0.5870f * c[1] + 0.1140f * c[2];
        o[i] = b == 1 ? v / 255.0f : v;
    }
    return out;
}

// depth in sensor units -> metres as float; a depth of depth_trunc or more becomes 0 (no measurement)
inline std::shared_ptr<Image> ConvertDepthToFloatImage(const Image &depth, double depth_scale = 1000.0, double depth_trunc = 3.0)
{
    auto out = CreateFloatImageFromImage(depth);
    float *p = (float *)out->data_.data();
    for (size_t i = 0; i < (size_t)out->width_ * out->height_; i++) {
        p[i] /= (float)depth_scale;
        if (p[i] >= depth_trunc) p[i] = 0.0f;
    }
    return out;
}

}  // namespace open3d
