// image.hip -- open3d::Image on the device (visma_icp_image_*): w x h pixels of 1 to 4 channels (the reference's functions
// know 1 and 3; any other count converts to the all-zero image) of 1, 2 or 4 bytes, row-major,
// resident between the steps of the reference's front end (Core/Geometry/Image.cpp, ImageFactory.cpp, RGBDImageFactory.cpp):
// CreateFloatImageFromImage, ConvertDepthToFloatImage, CreateImageFromFloatImage<T>, FilterHorizontalImage, FilterImage,
// FlipImage, DownsampleImage, DilateImage, LinearTransformImage, ClipIntensityImage, Image::FloatValueAt and the depth
// decoding of the SUN and NYU formats.  The arithmetic is the reference's operation for operation (the build's
// -ffp-contract=off: one rounding per operation, fp32 where it computes in fp32, f64 where it widens), fp32 denormals are
// kept (the build does not flush them).  One thread per output pixel, neighbouring lanes on neighbouring pixels of a row; no
// atomics; one writer per output pixel.
//   im_to_float        the nine channel x width combinations, Equal and Weighted, all fp32
//   im_depth           p /= (float)depth_scale in fp32, then (double)p >= depth_trunc -> 0
//   im_from_float      (T)(p * 255.0f) for one byte, (T)p for two: truncation toward zero where that is representable;
//                      outside it SATURATES (NaN and negatives 0, beyond the maximum the maximum): visma_icp.h's deviation
//   img_filter, img_downsample, img_linear   image_kernels.h, shared with the odometry pyramid
//   im_transpose       FlipImage, which is a transpose: a 64 x 64 tile through LDS, rows padded to 65 dwords.  A wave
//                      writes one tile row (64 consecutive dwords: ds_write_b32 is served in lane groups of 32 over 32
//                      banks, 32 distinct banks per group) and reads one tile column (stride 65 = 1 mod 32: distinct banks
//                      again); the global loads and stores are both runs of 64 consecutive floats
//   im_dilate_pass     DilateImage's OR over a (2k + 1)^2 window of in-bounds == 255 tests, which is exactly separable:
//                      rows into a 0 / 255 image, then columns of that; O(k) per pixel
//   im_clip            p > max -> (float)max, then p < min -> (float)min, both compares in f64; a NaN stays
//   im_value_at        FloatValueAt for n coordinates, f64 as the reference evaluates it
//   im_sun, im_nyu     the 16-bit depth decodings
#include "dev_mem.h"
#include "image_kernels.h"
#include "kernels.h"

#include <math.h>

#include <memory>
#include <vector>

namespace visma {

namespace {

#define IM_PIXEL(i, n)                                                             \
    const long long i = (long long)blockIdx.x * kImgThreads + threadIdx.x;       \
    if (i >= (n)) return;

template <class T, int CH, bool BYTE>
__global__ __launch_bounds__(kImgThreads) void im_to_float(const T *__restrict__ in, float *__restrict__ out, long long n, int weighted)
{
    IM_PIXEL(i, n);
    float p;
    if (CH == 1) {
        p = BYTE ? (float)in[i] / 255.0f : (float)in[i];
    } else {
        const float a = (float)in[3 * i], b = (float)in[3 * i + 1], c = (float)in[3 * i + 2];
        if (weighted) {
            p = 0.2990f * a + 0.5870f * b + 0.1140f * c;
            if (BYTE) p = p / 255.0f;
        } else {
            p = (a + b + c) / 3.0f;
            if (BYTE) p = p / 255.0f;
        }
    }
    out[i] = p;
}

__global__ __launch_bounds__(kImgThreads) void im_depth(float *img, long long n, float scale, double trunc)
{
    IM_PIXEL(i, n);
    float p = img[i];
    p /= scale;
    if ((double)p >= trunc) p = 0.0f;
    img[i] = p;
}

template <class T>
__global__ __launch_bounds__(kImgThreads) void im_from_float(const float *__restrict__ in, T *__restrict__ out, long long n)
{
    IM_PIXEL(i, n);
    const float v = sizeof(T) == 1 ? in[i] * 255.0f : in[i];
    const float top = sizeof(T) == 1 ? 255.0f : 65535.0f;
    T r = 0;                                                 // NaN, negatives and (-1, 0]
    if (v >= top) r = (T)top;
    else if (v > 0.0f) r = (T)(int)v;
    out[i] = r;
}

constexpr int kTile = 64, kTileRows = kImgThreads / kTile;

// out (h x w as width x height: out[x * h + y]) = in[y * w + x]
__global__ __launch_bounds__(kImgThreads) void im_transpose(const float *__restrict__ in, float *__restrict__ out, int w, int h)
{
    __shared__ float tile[kTile][kTile + 1];
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const int tiles_x = (w + kTile - 1) / kTile;            // a 1-D grid of tiles: no limit of a grid's y dimension applies
    const int x0 = (int)(blockIdx.x % tiles_x) * kTile, y0 = (int)(blockIdx.x / tiles_x) * kTile;
    for (int r = ty; r < kTile; r += kTileRows) {
        const int x = x0 + tx, y = y0 + r;
        if (x < w && y < h) tile[r][tx] = in[(long long)y * w + x];
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += kTileRows) {
        const int y = y0 + tx, x = x0 + r;                   // the output row x, its column y
        if (x < w && y < h) out[(long long)x * h + y] = tile[tx][r];
    }
}

// out = 255 where a pixel == 255 lies within `k` of the pixel along the row (VERTICAL: the column), inside the image; else 0
template <bool VERTICAL>
__global__ __launch_bounds__(kImgThreads) void im_dilate_pass(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int w, int h, int k)
{
    IM_PIXEL(i, (long long)w * h);
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    const int pos = VERTICAL ? y : x, last = (VERTICAL ? h : w) - 1;
    const long long step = VERTICAL ? w : 1, base = i - (long long)pos * step;
    const int lo = pos - k < 0 ? 0 : pos - k, hi = pos + k > last ? last : pos + k;    // (k <= max(w, h): the caller clamps it)
    uint8_t r = 0;
    for (int q = lo; q <= hi; q++)
        if (in[base + q * step] == 255) { r = 255; break; }
    out[i] = r;
}

__global__ __launch_bounds__(kImgThreads) void im_clip(float *img, long long n, double lo, double hi)
{
    IM_PIXEL(i, n);
    float p = img[i];
    if ((double)p > hi) p = (float)hi;
    if ((double)p < lo) p = (float)lo;
    img[i] = p;
}

// Image.cpp:73-93.  w >= 2 and h >= 2 (the caller answers (false, 0) otherwise); a NaN coordinate: (false, 0)
__global__ __launch_bounds__(kImgThreads) void im_value_at(const float *__restrict__ img, int w, int h, const double *__restrict__ uv,
                                                           long long n, uint8_t *__restrict__ ok, double *__restrict__ value)
{
    IM_PIXEL(i, n);
    const double u = uv[2 * i], v = uv[2 * i + 1];
    uint8_t good = 0;
    double r = 0.0;
    if (!(isnan(u) || isnan(v)) && !(u < 0.0 || u > (double)(w - 1) || v < 0.0 || v > (double)(h - 1))) {
        int ui = (int)u, vi = (int)v;
        ui = ui < w - 2 ? ui : w - 2; ui = ui > 0 ? ui : 0;
        vi = vi < h - 2 ? vi : h - 2; vi = vi > 0 ? vi : 0;
        const double pu = u - (double)ui, pv = v - (double)vi;
        const double v0 = (double)img[(long long)vi * w + ui], v1 = (double)img[(long long)(vi + 1) * w + ui];
        const double v2 = (double)img[(long long)vi * w + ui + 1], v3 = (double)img[(long long)(vi + 1) * w + ui + 1];
        r = (v0 * (1.0 - pv) + v1 * pv) * (1.0 - pu) + (v2 * (1.0 - pv) + v3 * pv) * pu;
        good = 1;
    }
    ok[i] = good;
    value[i] = r;
}

// RGBDImageFactory.cpp:79-84: each 16-bit depth rotated right by three bits
__global__ __launch_bounds__(kImgThreads) void im_sun(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, long long n)
{
    IM_PIXEL(i, n);
    const unsigned d = in[i];
    out[i] = (uint16_t)((d >> 3) | (d << 13));
}

// RGBDImageFactory.cpp:100-114: bytes swapped, 351.3 / (1092.5 - d) metres, to millimetres.  The reference's cast is
// undefined beyond 65535 (swapped values 1088 .. 1092): saturated here
__global__ __launch_bounds__(kImgThreads) void im_nyu(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, long long n)
{
    IM_PIXEL(i, n);
    const unsigned raw = in[i];
    const unsigned d = ((raw >> 8) | (raw << 8)) & 0xffffu;
    const double xx = 351.3 / (1092.5 - (double)d);
    uint16_t r = 0;
    if (!(xx <= 0.0)) {
        const double mm = floor(xx * 1000.0 + 0.5);
        r = mm >= 65535.0 ? (uint16_t)65535 : (uint16_t)(int)mm;
    }
    out[i] = r;
}

}  // namespace

struct ImageDevice {
    int w = 0, h = 0, ch = 0, bpc = 0;                      // an image without pixels keeps its format (PrepareImage(0, 0, 1, 4))
    bool integer = false;                                    // 1 x 4 bytes holding int32 (the renderer's index image), not float
    DeviceBuf<uint8_t> px;
    size_t pixels() const { return (size_t)w * (size_t)h; }
    size_t bytes() const { return pixels() * (size_t)ch * (size_t)bpc; }
    bool is_float() const { return ch == 1 && bpc == 4 && !integer; }
    float *f() const { return reinterpret_cast<float *>(px.get()); }
};

// what a call works in, one per context, grow-only: a filter's long weights, the image between the two passes of a separable
// filter or of dilate.  Every call returns with the stream idle, so the next call finds it free
struct ImageScratch {
    DeviceBuf<float> taps, tmp;
    DeviceBuf<uint8_t> tmp8;
};

ImageScratch *image_scratch_create() { return new ImageScratch; }
void image_scratch_destroy(ImageScratch *W) { delete W; }

namespace {

// a new image of that format with its (uninitialised) pixels; w * h may be 0
hipError_t make_image(int w, int h, int ch, int bpc, std::unique_ptr<ImageDevice> &O)
{
    O.reset(new ImageDevice);
    O->w = w; O->h = h; O->ch = ch; O->bpc = bpc;
    if (O->bytes() > 0) DEV_RESET(O->px, O->bytes());
    return hipSuccess;
}

hipError_t finish(std::unique_ptr<ImageDevice> &O, hipStream_t stream, ImageDevice **out)
{
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = O.release();
    return hipSuccess;
}

// the reference's empty Image
hipError_t empty_image(ImageDevice **out)
{
    *out = new ImageDevice;
    return hipSuccess;
}

// (float)kernel[k] for every tap; beyond kImgArgTaps also into the scratch's device buffer
hipError_t stage_taps(ImageScratch *S, const double *kernel, int n, std::vector<float> &host, const float **dev, hipStream_t stream)
{
    host.resize((size_t)n);
    for (int k = 0; k < n; k++) host[(size_t)k] = (float)kernel[k];
    *dev = nullptr;
    if (n > kImgArgTaps) {
        DEV_RESERVE(S->taps, (size_t)n);
        VISMA_TRY(hipMemcpyAsync(S->taps.get(), host.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, stream));
        VISMA_TRY(hipStreamSynchronize(stream));           // (`host` is pageable memory and is written again)
        *dev = S->taps.get();
    }
    return hipSuccess;
}

}  // namespace

void image_device_destroy(ImageDevice *I) { delete I; }

void image_device_info(const ImageDevice *I, int *w, int *h, int *ch, int *bpc) { *w = I->w; *h = I->h; *ch = I->ch; *bpc = I->bpc; }

const void *image_device_pixels(const ImageDevice *I) { return I->px.get(); }
void *image_device_pixels_rw(ImageDevice *I) { return I->px.get(); }
bool image_device_is_integer(const ImageDevice *I) { return I->integer; }

hipError_t image_device_alloc(int w, int h, int ch, int bpc, bool integer, ImageDevice **out)
{
    *out = nullptr;
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(w, h, ch, bpc, O));
    O->integer = integer;
    *out = O.release();
    return hipSuccess;
}

hipError_t image_device_create(int w, int h, int ch, int bpc, const void *data, bool on_device, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(w, h, ch, bpc, O));
    if (O->bytes() > 0)
        VISMA_TRY(hipMemcpyAsync(O->px.get(), data, O->bytes(), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    return finish(O, stream, out);
}

hipError_t image_device_get(const ImageDevice *I, void *bytes, hipStream_t stream)
{
    if (I->bytes() > 0) VISMA_TRY(hipMemcpyAsync(bytes, I->px.get(), I->bytes(), hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t image_device_copy(const ImageDevice *S, hipStream_t stream, ImageDevice **out)
{
    VISMA_TRY(image_device_create(S->w, S->h, S->ch, S->bpc, S->px.get(), true, stream, out));
    (*out)->integer = S->integer;
    return hipSuccess;
}

// ImageFactory.cpp:64-120
hipError_t image_device_to_float(const ImageDevice *S, int weighted, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    if (S->bytes() == 0) return empty_image(out);            // IsEmpty()
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(S->w, S->h, 1, 4, O));
    const long long n = (long long)S->pixels();
    const dim3 grid(img_blocks(n)), block(kImgThreads);
    const void *p = S->px.get();
    float *o = O->f();
    if (S->ch == 1 && S->bpc == 1) hipLaunchKernelGGL((im_to_float<uint8_t, 1, true>), grid, block, 0, stream, (const uint8_t *)p, o, n, weighted);
    else if (S->ch == 1 && S->bpc == 2) hipLaunchKernelGGL((im_to_float<uint16_t, 1, false>), grid, block, 0, stream, (const uint16_t *)p, o, n, weighted);
    else if (S->ch == 1 && S->bpc == 4) hipLaunchKernelGGL((im_to_float<float, 1, false>), grid, block, 0, stream, (const float *)p, o, n, weighted);
    else if (S->ch == 3 && S->bpc == 1) hipLaunchKernelGGL((im_to_float<uint8_t, 3, true>), grid, block, 0, stream, (const uint8_t *)p, o, n, weighted);
    else if (S->ch == 3 && S->bpc == 2) hipLaunchKernelGGL((im_to_float<uint16_t, 3, false>), grid, block, 0, stream, (const uint16_t *)p, o, n, weighted);
    else if (S->ch == 3 && S->bpc == 4) hipLaunchKernelGGL((im_to_float<float, 3, false>), grid, block, 0, stream, (const float *)p, o, n, weighted);
    else VISMA_TRY(hipMemsetAsync(o, 0, O->bytes(), stream));   // any other channel count: PrepareImage's zeros
    return finish(O, stream, out);
}

// Image.cpp:118-133 (the conversion with its default type, Weighted)
hipError_t image_device_depth_to_float(const ImageDevice *S, double depth_scale, double depth_trunc, hipStream_t stream, ImageDevice **out)
{
    ImageDevice *F = nullptr;
    VISMA_TRY(image_device_to_float(S, 1, stream, &F));
    std::unique_ptr<ImageDevice> O(F);
    const long long n = (long long)O->pixels();
    if (n > 0) hipLaunchKernelGGL(im_depth, dim3(img_blocks(n)), dim3(kImgThreads), 0, stream, O->f(), n, (float)depth_scale, depth_trunc);
    return finish(O, stream, out);
}

// ImageFactory.cpp:122-143
hipError_t image_device_from_float(const ImageDevice *S, int bytes, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    if (!S->is_float()) return empty_image(out);
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(S->w, S->h, 1, bytes, O));
    const long long n = (long long)S->pixels();
    if (n > 0) {
        const dim3 grid(img_blocks(n)), block(kImgThreads);
        if (bytes == 1) hipLaunchKernelGGL(im_from_float<uint8_t>, grid, block, 0, stream, S->f(), O->px.get(), n);
        else hipLaunchKernelGGL(im_from_float<uint16_t>, grid, block, 0, stream, S->f(), reinterpret_cast<uint16_t *>(O->px.get()), n);
    }
    return finish(O, stream, out);
}

// Image.cpp:194-226
hipError_t image_device_filter_horizontal(const ImageDevice *S, ImageScratch *W, const double *kernel, int n, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    if (!S->is_float() || n % 2 != 1) return empty_image(out);
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(S->w, S->h, 1, 4, O));
    std::vector<float> host;
    const float *dev = nullptr;
    VISMA_TRY(stage_taps(W, kernel, n, host, &dev, stream));
    VISMA_TRY(img_launch_filter<false>(S->f(), O->f(), S->w, S->h, host.data(), n, dev, stream));
    return finish(O, stream, out);                           // (returns with the stream idle: `host` was read)
}

// Image.cpp:270-284: horizontal(dx), transpose, horizontal(dy), transpose -- the second pass walks the columns instead
hipError_t image_device_filter_separable(const ImageDevice *S, ImageScratch *W, const double *dx, int n_dx, const double *dy, int n_dy, hipStream_t stream,
                                         ImageDevice **out)
{
    *out = nullptr;
    if (!S->is_float() || n_dx % 2 != 1 || n_dy % 2 != 1) return empty_image(out);
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(S->w, S->h, 1, 4, O));
    if (S->pixels() > 0) {
        DEV_RESERVE(W->tmp, S->pixels());
        std::vector<float> host;
        const float *dev = nullptr;
        VISMA_TRY(stage_taps(W, dx, n_dx, host, &dev, stream));
        VISMA_TRY(img_launch_filter<false>(S->f(), W->tmp.get(), S->w, S->h, host.data(), n_dx, dev, stream));
        if (dev) VISMA_TRY(hipStreamSynchronize(stream));    // the weight buffer is staged again
        VISMA_TRY(stage_taps(W, dy, n_dy, host, &dev, stream));
        VISMA_TRY(img_launch_filter<true>(W->tmp.get(), O->f(), S->w, S->h, host.data(), n_dy, dev, stream));
    }
    return finish(O, stream, out);
}

// Image.cpp:286-306
hipError_t image_device_flip(const ImageDevice *S, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    if (!S->is_float()) return empty_image(out);
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(S->h, S->w, 1, 4, O));
    if (S->pixels() > 0) {
        const dim3 grid((unsigned)((S->w + kTile - 1) / kTile) * (unsigned)((S->h + kTile - 1) / kTile));   // at most 2^30 / 64 tiles
        hipLaunchKernelGGL(im_transpose, grid, dim3(kImgThreads), 0, stream, S->f(), O->f(), S->w, S->h);
    }
    return finish(O, stream, out);
}

// Image.cpp:167-192
hipError_t image_device_downsample(const ImageDevice *S, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    if (!S->is_float()) return empty_image(out);
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(S->w / 2, S->h / 2, 1, 4, O));
    VISMA_TRY(img_launch_downsample(S->f(), S->w, S->h, O->f(), stream));
    return finish(O, stream, out);
}

// Image.cpp:308-339
hipError_t image_device_dilate(const ImageDevice *S, ImageScratch *W, int half_kernel_size, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    if (S->ch != 1 || S->bpc != 1) return empty_image(out);
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(S->w, S->h, 1, 1, O));
    const long long n = (long long)S->pixels();
    if (n > 0) {
        if (half_kernel_size < 0) {
            VISMA_TRY(hipMemsetAsync(O->px.get(), 0, (size_t)n, stream));
        } else {
            const int k = half_kernel_size < (S->w > S->h ? S->w : S->h) ? half_kernel_size : (S->w > S->h ? S->w : S->h);
            DEV_RESERVE(W->tmp8, (size_t)n);
            const dim3 grid(img_blocks(n)), block(kImgThreads);
            hipLaunchKernelGGL(im_dilate_pass<false>, grid, block, 0, stream, S->px.get(), W->tmp8.get(), S->w, S->h, k);
            hipLaunchKernelGGL(im_dilate_pass<true>, grid, block, 0, stream, W->tmp8.get(), O->px.get(), S->w, S->h, k);
        }
    }
    return finish(O, stream, out);
}

// Image.cpp:153-165; an unsupported format is left as it is
hipError_t image_device_linear_transform(ImageDevice *I, double scale, double offset, hipStream_t stream)
{
    if (I->is_float()) VISMA_TRY(img_launch_linear(I->f(), (int64_t)I->pixels(), scale, offset, stream));
    return hipStreamSynchronize(stream);
}

// Image.cpp:135-151
hipError_t image_device_clip_intensity(ImageDevice *I, double lo, double hi, hipStream_t stream)
{
    const long long n = (long long)I->pixels();
    if (I->is_float() && n > 0) {
        hipLaunchKernelGGL(im_clip, dim3(img_blocks(n)), dim3(kImgThreads), 0, stream, I->f(), n, lo, hi);
        VISMA_TRY(hipGetLastError());
    }
    return hipStreamSynchronize(stream);
}

hipError_t image_device_distance_multiplier(int w, int h, const double intrinsic[4], hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(w, h, 1, 4, O));
    VISMA_TRY(launch_tsdf_multiplier(O->f(), w, h, intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3], stream));
    return finish(O, stream, out);
}

hipError_t image_device_float_value_at(const ImageDevice *I, const double *uv, int64_t n, uint8_t *ok, double *value, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (!I->is_float() || I->w < 2 || I->h < 2) {
        for (int64_t i = 0; i < n; i++) { ok[i] = 0; value[i] = 0.0; }
        return hipSuccess;
    }
    DeviceBuf<double> d_uv, d_value;
    DeviceBuf<uint8_t> d_ok;
    DEV_RESET(d_uv, 2 * (size_t)n);
    DEV_RESET(d_value, (size_t)n);
    DEV_RESET(d_ok, (size_t)n);
    VISMA_TRY(hipMemcpyAsync(d_uv.get(), uv, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(im_value_at, dim3(img_blocks(n)), dim3(kImgThreads), 0, stream, I->f(), I->w, I->h, d_uv.get(), (long long)n,
                       d_ok.get(), d_value.get());
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(hipMemcpyAsync(ok, d_ok.get(), (size_t)n, hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipMemcpyAsync(value, d_value.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

// the SUN (nyu == false) or NYU decoding of a 1 x uint16 depth image into a new one
hipError_t image_device_decode_depth(const ImageDevice *S, bool nyu, hipStream_t stream, ImageDevice **out)
{
    *out = nullptr;
    std::unique_ptr<ImageDevice> O;
    VISMA_TRY(make_image(S->w, S->h, 1, 2, O));
    const long long n = (long long)S->pixels();
    if (n > 0) {
        const uint16_t *in = reinterpret_cast<const uint16_t *>(S->px.get());
        uint16_t *o = reinterpret_cast<uint16_t *>(O->px.get());
        if (nyu) hipLaunchKernelGGL(im_nyu, dim3(img_blocks(n)), dim3(kImgThreads), 0, stream, in, o, n);
        else hipLaunchKernelGGL(im_sun, dim3(img_blocks(n)), dim3(kImgThreads), 0, stream, in, o, n);
    }
    return finish(O, stream, out);
}

}  // namespace visma
