// odometry_image.hip -- the image side of RGB-D odometry (Open3D's InitializeRGBDOdometry, CreateRGBDImagePyramid,
// FilterRGBDImagePyramid, ConvertDepthImageToXYZImage and ComputeCorrespondence; Odometry.cpp, Image.cpp, ImageFactory.cpp,
// RGBDImage.cpp) on gfx950.  Single-channel fp32 images, row-major; one thread per OUTPUT pixel, neighbouring lanes on
// neighbouring pixels of a row.  A frame is 0.3 M pixels (1.2 MB): every kernel here streams it once and is bound by its
// launch, not by the memory system, so none of them stages anything in LDS.
//
//  preprocess_depth   d < min_depth || d > max_depth || d <= 0 -> quiet NaN
//  filter3, downsample, scale   image_kernels.h, shared with the resident Image (image.hip): the separable filter's pass at
//                     three taps (rows, then the same arithmetic down the columns), (p1 + p2 + p3 + p4) / 4.0f, and
//                     NormalizeIntensity's p = (float)(scale * p + 0.0).  Every 3-tap weight in use (.25, .5; 0, +-1, 2) makes
//                     the fp32 product exact: the images are the reference's bit for bit.
//  xyz                (float)((x - ox) * z * inv_fx) evaluated in f64; float4 per pixel so that the information pass reads it
//                     as its target cloud
//  correspondences    one thread per SOURCE pixel, f64: uv = d_s * (K R K^-1) (u, v, 1) + K t, u_t = (int)(uv.x / uv.z + 0.5)
//                     (truncation toward zero, as the reference's cast), bounds, !isnan(d_t), |uv.z - d_t| <= max_depth_diff.
//                     The reference's depth buffer is keyed by the source pixel, which is visited once: nothing to
//                     arbitrate, no atomics.  Deviation (visma_icp.h): uv.z <= 0 or a projection that is not finite or
//                     beyond the int range has no pair -- the reference's cast is undefined there.
// (Reasoning: DESIGN.md 4.4c10.)
#include "image_kernels.h"
#include "kernels.h"

#include <cmath>

namespace visma {

namespace {

__global__ __launch_bounds__(kImgThreads) void preprocess_depth_kernel(const float *in, float *out, long long n,
                                                                       double min_depth, double max_depth)
{
    const long long i = (long long)blockIdx.x * kImgThreads + threadIdx.x;
    if (i >= n) return;
    const float p = in[i];
    const bool bad = (double)p < min_depth || (double)p > max_depth || p <= 0.0f;
    out[i] = bad ? __builtin_nanf("") : p;
}

__global__ __launch_bounds__(kImgThreads) void xyz_kernel(const float *__restrict__ depth, int w, int h, double ox, double oy,
                                                          double inv_fx, double inv_fy, float4 *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kImgThreads + threadIdx.x;
    if (i >= (long long)w * h) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    const float z = depth[i];
    float4 p;
    p.x = (float)(((double)x - ox) * (double)z * inv_fx);
    p.y = (float)(((double)y - oy) * (double)z * inv_fy);
    p.z = z;
    p.w = 0.0f;
    out[i] = p;
}

__global__ __launch_bounds__(kImgThreads) void correspondences_kernel(const float *__restrict__ depth_s, const float *__restrict__ depth_t,
                                                                      int w, int h, OdoProjection P, double max_depth_diff,
                                                                      int32_t *__restrict__ idx)
{
    const long long i = (long long)blockIdx.x * kImgThreads + threadIdx.x;
    if (i >= (long long)w * h) return;
    const int v_s = (int)(i / w), u_s = (int)(i - (long long)v_s * w);
    const double d = (double)depth_s[i];
    int32_t found = -1;
    if (!isnan(d)) {
        const double u = (double)u_s, v = (double)v_s;
        const double x = d * (P.m[0] * u + P.m[1] * v + P.m[2]) + P.kt[0];
        const double y = d * (P.m[3] * u + P.m[4] * v + P.m[5]) + P.kt[1];
        const double z = d * (P.m[6] * u + P.m[7] * v + P.m[8]) + P.kt[2];
        const double qu = x / z + 0.5, qv = y / z + 0.5;
        // (NaN fails every comparison: a projection that is not finite has no pair)
        if (z > 0.0 && fabs(qu) < 1073741824.0 && fabs(qv) < 1073741824.0) {
            const int u_t = (int)qu, v_t = (int)qv;          // toward zero: -0.7 is pixel 0, as in the reference
            if (u_t >= 0 && u_t < w && v_t >= 0 && v_t < h) {
                const double d_t = (double)depth_t[(long long)v_t * w + u_t];
                if (!isnan(d_t) && fabs(z - d_t) <= max_depth_diff) found = v_t * w + u_t;
            }
        }
    }
    idx[i] = found;
}

}  // namespace

hipError_t launch_odo_preprocess_depth(const float *in, float *out, int64_t n, double min_depth, double max_depth, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(preprocess_depth_kernel, dim3(img_blocks(n)), dim3(kImgThreads), 0, stream, in, out, (long long)n, min_depth, max_depth);
    return hipGetLastError();
}

hipError_t launch_odo_filter3(const float *in, float *out, int w, int h, float k0, float k1, float k2, int vertical, hipStream_t stream)
{
    const float k[3] = {k0, k1, k2};
    return vertical ? img_launch_filter<true>(in, out, w, h, k, 3, nullptr, stream) : img_launch_filter<false>(in, out, w, h, k, 3, nullptr, stream);
}

hipError_t launch_odo_downsample(const float *in, int w, int h, float *out, hipStream_t stream)
{
    return img_launch_downsample(in, w, h, out, stream);
}

hipError_t launch_odo_scale(float *img, int64_t n, double scale, hipStream_t stream)
{
    return img_launch_linear(img, n, scale, 0.0, stream);
}

hipError_t launch_odo_xyz(const float *depth, int w, int h, double ox, double oy, double inv_fx, double inv_fy, float4 *out,
                          hipStream_t stream)
{
    if (w <= 0 || h <= 0) return hipSuccess;
    hipLaunchKernelGGL(xyz_kernel, dim3(img_blocks((int64_t)w * h)), dim3(kImgThreads), 0, stream, depth, w, h, ox, oy, inv_fx, inv_fy, out);
    return hipGetLastError();
}

hipError_t launch_odo_correspondences(const float *depth_s, const float *depth_t, int w, int h, const OdoProjection &P,
                                      double max_depth_diff, int32_t *idx, hipStream_t stream)
{
    if (w <= 0 || h <= 0) return hipSuccess;
    hipLaunchKernelGGL(correspondences_kernel, dim3(img_blocks((int64_t)w * h)), dim3(kImgThreads), 0, stream, depth_s, depth_t, w, h, P,
                       max_depth_diff, idx);
    return hipGetLastError();
}

}  // namespace visma
