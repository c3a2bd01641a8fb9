// Core/Geometry/Image.h -- the image type RGB-D odometry takes (shape of O3D/Core/Geometry/Image.h): a width, a height, a
// number of channels, bytes per channel and the pixel bytes, row-major.  Stand-alone and header-only: PrepareImage, PointerAt
// and the two conversions an odometry caller needs (any image -> single-channel float, a depth image -> metres); the
// filters, pyramids and the other functions of the reference's Image.h are declared at the end and run on the GPU
// (visma_icp_open3d.hpp, over the C ABI's resident image, visma_icp.h: visma_icp_image_*): an upload, the operation and a
// download each, on the calling thread's context; cicp::DeviceImage keeps an image there across a chain of them.
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

namespace open3d {

class PinholeCameraIntrinsic;

class Image {
public:
    enum class ColorToIntensityConversionType { Equal, Weighted };
    enum class FilterType { Gaussian3, Gaussian5, Gaussian7, Sobel3Dx, Sobel3Dy };

    void Clear() { width_ = height_ = num_of_channels_ = bytes_per_channel_ = 0; data_.clear(); }
    bool HasData() const { return width_ > 0 && height_ > 0 && data_.size() == size_t(height_ * BytesPerLine()); }
    bool IsEmpty() const { return !HasData(); }
    void PrepareImage(int width, int height, int num_of_channels, int bytes_per_channel)
    {
        width_ = width; height_ = height; num_of_channels_ = num_of_channels; bytes_per_channel_ = bytes_per_channel;
        data_.resize((size_t)width_ * height_ * num_of_channels_ * bytes_per_channel_);
    }
    int BytesPerLine() const { return width_ * num_of_channels_ * bytes_per_channel_; }
    // (u, v) inside the image, at least inner_margin from its border
    bool TestImageBoundary(double u, double v, double inner_margin = 0.0) const
    {
        return u >= inner_margin && u < width_ - inner_margin && v >= inner_margin && v < height_ - inner_margin;
    }
    // the bilinear value of a 1 x float image at (u, v) in [0, width - 1] x [0, height - 1], in f64; (false, 0) outside, on
    // another format, on an image narrower or lower than 2 pixels and for a NaN coordinate (visma_icp.h: the deviation)
    std::pair<bool, double> FloatValueAt(double u, double v) const
    {
        if (num_of_channels_ != 1 || bytes_per_channel_ != 4 || width_ < 2 || height_ < 2 || u != u || v != v || u < 0.0 ||
            u > (double)(width_ - 1) || v < 0.0 || v > (double)(height_ - 1))
            return std::make_pair(false, 0.0);
        const int ui = std::max(std::min((int)u, width_ - 2), 0), vi = std::max(std::min((int)v, height_ - 2), 0);
        const double pu = u - ui, pv = v - vi;
        const float *p = (const float *)data_.data() + (size_t)vi * width_ + ui;
        const double a = p[0], b = p[width_], c = p[1], d = p[width_ + 1];
        return std::make_pair(true, (a * (1 - pv) + b * pv) * (1 - pu) + (c * (1 - pv) + d * pv) * pu);
    }

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

typedef std::vector<std::shared_ptr<Image>> ImagePyramid;

// The rest of the reference's Image.h, on the GPU (visma_icp_open3d.hpp; the rules and the stated deviations: visma_icp.h,
// "Image").  An input a function does not take gives the empty Image, as in the reference.
inline std::shared_ptr<Image> CreateDepthToCameraDistanceMultiplierFloatImage(const PinholeCameraIntrinsic &intrinsic);
template <typename T>
std::shared_ptr<Image> CreateImageFromFloatImage(const Image &input);             // T: uint8_t or uint16_t; saturating
inline std::shared_ptr<Image> FlipImage(const Image &input);                     // a transpose
inline std::shared_ptr<Image> FilterImage(const Image &input, Image::FilterType type);
inline std::shared_ptr<Image> FilterImage(const Image &input, const std::vector<double> &dx, const std::vector<double> &dy);
inline std::shared_ptr<Image> FilterHorizontalImage(const Image &input, const std::vector<double> &kernel);
inline std::shared_ptr<Image> DownsampleImage(const Image &input);
inline std::shared_ptr<Image> DilateImage(const Image &input, int half_kernel_size = 1);
inline void LinearTransformImage(Image &input, double scale, double offset = 0.0);
inline void ClipIntensityImage(Image &input, double min = 0.0, double max = 1.0);
inline ImagePyramid FilterImagePyramid(const ImagePyramid &input, Image::FilterType type);
inline ImagePyramid CreateImagePyramid(const Image &image, size_t num_of_levels, bool with_gaussian_filter = true);

}  // namespace open3d
