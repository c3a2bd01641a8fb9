// image_kernels.h -- the kernels over single-channel fp32 images that the odometry pyramid (odometry_image.hip) and the
// resident Image (image.hip) share: one pass of a separable filter of any odd length, the 2 x 2 down-sampler and the linear
// transform.  One copy of the text; each including file gets its own compiled copy (unnamed namespace), as with
// row_kernels.h.  One thread per OUTPUT pixel, neighbouring lanes on neighbouring pixels of a row.
//
//  img_filter   FilterHorizontalImage (Image.cpp) along the rows, or the same arithmetic down the columns (the reference
//               transposes, filters the rows and transposes back): per tap the fp32 product pixel * (float)weight, widened
//               and added into an f64 sum in tap order -half .. +half, one cast to fp32; indices clamped at both borders.
//               The 3-tap weights in use (.25, .5; 0, +-1, 2) make every product exact; Gaussian5's .375 and Gaussian7's
//               .109375, .21875, .28125 have three mantissa bits and a caller's weights any number: those products ROUND,
//               once, in fp32, as the reference's do (-ffp-contract=off keeps product and sum apart).  A NaN propagates
//               as it does there, 0 * NaN included.  Up to kImgArgTaps weights travel as kernel arguments and the loop is
//               unrolled over them; a longer kernel's lie in a device buffer.
//  img_downsample   (p1 + p2 + p3 + p4) / 4.0f in fp32, in that order; floor(w / 2) x floor(h / 2)
//  img_linear   LinearTransformImage: p = (float)(scale * (double)p + offset), in f64
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace visma {

namespace {

constexpr int kImgThreads = 256;
constexpr int kImgArgTaps = 9;                           // the longest kernel whose weights are kernel arguments
inline unsigned img_blocks(int64_t n) { return (unsigned)((n + kImgThreads - 1) / kImgThreads); }

struct ImgTaps { float k[kImgArgTaps]; };

// HALF >= 0: 2 HALF + 1 weights in `arg`, unrolled.  HALF < 0: 2 half + 1 weights at `taps` on the device.
template <bool VERTICAL, int HALF>
__global__ __launch_bounds__(kImgThreads) void img_filter_kernel(const float *__restrict__ in, float *__restrict__ out, int w, int h,
                                                                 ImgTaps arg, const float *__restrict__ taps, int half)
{
    const long long i = (long long)blockIdx.x * kImgThreads + threadIdx.x;
    if (i >= (long long)w * h) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    const int pos = VERTICAL ? y : x, last = (VERTICAL ? h : w) - 1;
    const long long step = VERTICAL ? w : 1, base = i - (long long)pos * step;
    double t = 0.0;
    if (HALF >= 0) {
#pragma unroll
        for (int k = -HALF; k <= HALF; k++) {
            int q = pos + k;
            q = q < 0 ? 0 : q;
            q = q > last ? last : q;
            t += (double)(in[base + (long long)q * step] * arg.k[k + HALF]);
        }
    } else {
        for (long long k = -(long long)half; k <= half; k++) {
            long long q = pos + k;
            q = q < 0 ? 0 : q;
            q = q > last ? last : q;
            t += (double)(in[base + q * step] * taps[k + half]);
        }
    }
    out[i] = (float)t;
}

__global__ __launch_bounds__(kImgThreads) void img_downsample_kernel(const float *__restrict__ in, int w, float *__restrict__ out, int ow, int oh)
{
    const long long i = (long long)blockIdx.x * kImgThreads + threadIdx.x;
    if (i >= (long long)ow * oh) return;
    const int y = (int)(i / ow), x = (int)(i - (long long)y * ow);
    const float *r0 = in + (long long)(2 * y) * w + 2 * x, *r1 = r0 + w;   // 2x + 1 < w and 2y + 1 < h by ow = w / 2, oh = h / 2
    out[i] = (r0[0] + r0[1] + r1[0] + r1[1]) / 4.0f;
}

__global__ __launch_bounds__(kImgThreads) void img_linear_kernel(float *img, long long n, double scale, double offset)
{
    const long long i = (long long)blockIdx.x * kImgThreads + threadIdx.x;
    if (i >= n) return;
    img[i] = (float)(scale * (double)img[i] + offset);
}

// One pass over w x h pixels with n = 2 half + 1 weights (n odd).  n <= kImgArgTaps: `weights` is read on the host;
// else `dev_taps` holds them on the device.  `in` and `out` are different images.
template <bool VERTICAL>
inline hipError_t img_launch_filter(const float *in, float *out, int w, int h, const float *weights, int n, const float *dev_taps,
                                    hipStream_t stream)
{
    if (w <= 0 || h <= 0) return hipSuccess;
    const dim3 grid(img_blocks((int64_t)w * h)), block(kImgThreads);
    const int half = n / 2;
    ImgTaps arg = {};
    if (n <= kImgArgTaps) for (int k = 0; k < n; k++) arg.k[k] = weights[k];
    switch (n <= kImgArgTaps ? half : -1) {
    case 0: hipLaunchKernelGGL((img_filter_kernel<VERTICAL, 0>), grid, block, 0, stream, in, out, w, h, arg, nullptr, half); break;
    case 1: hipLaunchKernelGGL((img_filter_kernel<VERTICAL, 1>), grid, block, 0, stream, in, out, w, h, arg, nullptr, half); break;
    case 2: hipLaunchKernelGGL((img_filter_kernel<VERTICAL, 2>), grid, block, 0, stream, in, out, w, h, arg, nullptr, half); break;
    case 3: hipLaunchKernelGGL((img_filter_kernel<VERTICAL, 3>), grid, block, 0, stream, in, out, w, h, arg, nullptr, half); break;
    case 4: hipLaunchKernelGGL((img_filter_kernel<VERTICAL, 4>), grid, block, 0, stream, in, out, w, h, arg, nullptr, half); break;
    default: hipLaunchKernelGGL((img_filter_kernel<VERTICAL, -1>), grid, block, 0, stream, in, out, w, h, arg, dev_taps, half); break;
    }
    return hipGetLastError();
}

inline hipError_t img_launch_downsample(const float *in, int w, int h, float *out, hipStream_t stream)
{
    const int ow = w / 2, oh = h / 2;
    if (ow <= 0 || oh <= 0) return hipSuccess;
    hipLaunchKernelGGL(img_downsample_kernel, dim3(img_blocks((int64_t)ow * oh)), dim3(kImgThreads), 0, stream, in, w, out, ow, oh);
    return hipGetLastError();
}

inline hipError_t img_launch_linear(float *img, int64_t n, double scale, double offset, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(img_linear_kernel, dim3(img_blocks(n)), dim3(kImgThreads), 0, stream, img, (long long)n, scale, offset);
    return hipGetLastError();
}

}  // namespace

}  // namespace visma
