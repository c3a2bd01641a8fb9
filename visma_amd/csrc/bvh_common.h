// bvh_common.h -- the Morton-ordered implicit BVH that mesh.hip (point -> triangle mesh) and cloud_distance.hip
// (point -> point cloud) both search: the 30-bit Morton code over a bounding box, its stable radix sort, the levels
// of the heap-ordered tree above the leaves, the box lower bound of the walk, and the final sqrt.
//
// Included by exactly those two files; the kernels and host helpers are `static`, so each file carries its own
// copy (no relocatable device code is needed) under the same kernel name.
#pragma once

#include "device_common.h"
#include "dev_mem.h"

#include <hipcub/hipcub.hpp>

#include <math.h>

namespace visma {

struct MortonParams {
    double lo[3], inv[3];            // code = min(1023, (c - lo) * inv)
};

__device__ __forceinline__ unsigned spread10(unsigned v)
{
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 10 bits per axis, clamped to the box (a NaN coordinate lands in cell 0)
__device__ __forceinline__ unsigned morton_code(const double c[3], const MortonParams &mp)
{
    unsigned code = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double q = (c[a] - mp.lo[a]) * mp.inv[a];
        q = q >= 0.0 ? q : 0.0;                       // also catches NaN
        const unsigned qi = q < 1023.0 ? (unsigned)q : 1023u;
        code |= spread10(qi) << (2 - a);
    }
    return code;
}

static __global__ __launch_bounds__(256) void point_code_kernel(const double *__restrict__ Pq, long long np,
                                                                MortonParams mp, unsigned *__restrict__ key,
                                                                unsigned *__restrict__ val)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const double c[3] = {Pq[3 * i], Pq[3 * i + 1], Pq[3 * i + 2]};
    key[i] = morton_code(c, mp);
    val[i] = (unsigned)i;
}

// Morton parameters of the box [lo, hi]: 1024 cells per axis, a flat axis all in cell 0
static inline MortonParams morton_params(const double lo[3], const double hi[3])
{
    MortonParams mp;
    for (int a = 0; a < 3; a++) {
        const double e = hi[a] - lo[a];
        mp.lo[a] = lo[a];
        mp.inv[a] = e > 0.0 ? 1024.0 / e : 0.0;
    }
    return mp;
}

// Stable LSD radix sort of n (< 2^31) 30-bit codes with their u32 payload: (key, val) -> (key_out, val_out).  `tmp`
// receives hipcub's scratch and must outlive the sort's kernels on `stream`.
static inline hipError_t morton_sort(unsigned *key, unsigned *key_out, unsigned *val, unsigned *val_out, int64_t n,
                                     DevBuf<char> &tmp, hipStream_t stream)
{
    size_t tmp_bytes = 0;
    VISMA_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, key, key_out, val, val_out, (int)n, 0, 30, stream));
    DEV_RESET(tmp, tmp_bytes);
    return hipcub::DeviceRadixSort::SortPairs(tmp.get(), tmp_bytes, key, key_out, val, val_out, (int)n, 0, 30, stream);
}

// node n = union of its children 2n, 2n+1 (boxes as lo[3], hi[3]); one launch per level, leaves first
static __global__ __launch_bounds__(256) void bvh_level_kernel(long long first, long long count,
                                                               double *__restrict__ nodes)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const long long n = first + i;
    const double *l = nodes + 6 * (2 * n), *r = l + 6;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        nodes[6 * n + a] = fmin(l[a], r[a]);
        nodes[6 * n + 3 + a] = fmax(l[3 + a], r[3 + a]);
    }
}

// the levels above the leaf level [P, 2P) of `nodes`
static inline hipError_t build_bvh_levels(double *nodes, int64_t P, hipStream_t stream)
{
    for (int64_t first = P >> 1; first >= 1; first >>= 1)
        hipLaunchKernelGGL(bvh_level_kernel, dim3((unsigned)((first + 255) / 256)), dim3(256), 0, stream,
                           (long long)first, (long long)first, nodes);
    return hipGetLastError();
}

__device__ __forceinline__ double box_lower_bound(const double *__restrict__ n, const double p[3])
{
    double s = 0.0;
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double below = n[a] - p[a], above = p[a] - n[3 + a];
        t[a] = fmax(0.0, fmax(below, above));        // +inf for an empty (inverted) box
    }
    s = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
    return s;
}

__device__ __forceinline__ float round_down_f32(double x)
{
    float f = (float)x;
    if ((double)f > x) f = nextafterf(f, -INFINITY);
    return f;
}

static __global__ __launch_bounds__(256) void sqrt_kernel(double *__restrict__ d, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) d[i] = sqrt(d[i]);                     // correctly rounded, as std::sqrt / Eigen cwiseSqrt
}

}  // namespace visma
