// feature_match.hip -- exact nearest neighbour among feature vectors on gfx950: for every row of fb the row of fa with the
// smallest squared distance.  What fast global registration's AdvancedMatching asks a KD-tree over 33-dimensional FPFH
// columns for (O3D/Core/Registration/FastGlobalRegistration.cpp:63-83, KDTreeFlann::SearchKNN(., 1, ...)); a grid cannot
// do it in 33 dimensions, a KD-tree degenerates there, brute force is exact and regular.
//
// d2 is flann's L2<double> (flann/algorithms/dist.h:150-177) to the bit: f64, plain differences, ascending j, whole
// groups of four added as result += ((s0 + s1) + s2) + s3 with s = diff * diff, the last dim % 4 one by one.  No
// |a|^2 + |b|^2 - 2 a.b rewrite: the argmin is the one a scan of fa in ascending index with a strict `<` finds -- exact
// ties go to the lowest index, a distance that is NaN or +inf never wins (-1 and +inf where nothing else exists).
//
// One query (a row of fb) per thread, its values in registers, padded with zeros to DP (a zero difference adds +0.0:
// no bit changes); fa streamed through LDS in tiles of kMatchRows rows that every thread of the workgroup reads at the
// same address (a broadcast, no bank conflict).  Rows are counted in 64 bits: up to 2^31 - 1 each.
#include "device_common.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace visma {

namespace {

constexpr int kMatchThreads = 256;
constexpr int kMatchRows = 64;       // rows of fa per LDS tile: 64 x 64 doubles = 32 KiB at the widest

template <int DP>
__global__ __launch_bounds__(kMatchThreads) void match_features_kernel(const double *__restrict__ fa, long long na,
                                                                       const double *__restrict__ fb, long long nb, int dim,
                                                                       int *__restrict__ nn, double *__restrict__ d2_out)
{
    __shared__ double tile[kMatchRows * DP];
    const int tid = threadIdx.x;
    const long long t = (long long)blockIdx.x * kMatchThreads + tid;
    const bool live = t < nb;                                     // (no early return: every thread fills the tiles)
    double q[DP];
#pragma unroll
    for (int j = 0; j < DP; j++) q[j] = (live && j < dim) ? fb[t * dim + j] : 0.0;
    const int groups = dim >> 2;                                  // whole groups of four (dist.h:158-166)
    double best = INFINITY;
    long long best_i = -1;
    for (long long r0 = 0; r0 < na; r0 += kMatchRows) {
        const int rows = (int)min((long long)kMatchRows, na - r0);
        __syncthreads();
        for (int e = tid; e < rows * DP; e += kMatchThreads) {
            const int r = e / DP, j = e - r * DP;
            tile[e] = j < dim ? fa[(r0 + r) * dim + j] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < rows; r++) {
            const double *a = tile + r * DP;
            double d = 0.0;
#pragma unroll
            for (int g = 0; g < DP / 4; g++) {
                const double e0 = q[4 * g] - a[4 * g], e1 = q[4 * g + 1] - a[4 * g + 1];
                const double e2 = q[4 * g + 2] - a[4 * g + 2], e3 = q[4 * g + 3] - a[4 * g + 3];
                if (g < groups) {
                    d += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
                } else {                                          // the last dim % 4 (the padding adds +0.0)
                    d += e0 * e0;
                    d += e1 * e1;
                    d += e2 * e2;
                    d += e3 * e3;
                }
            }
            if (d < best) { best = d; best_i = r0 + r; }
        }
    }
    if (live) {
        nn[t] = (int)best_i;
        if (d2_out) d2_out[t] = best;
    }
}

}  // namespace

// h_nn: nb indices into fa (-1: none); h_d2 (may be NULL): nb squared distances; kernel_ms (may be NULL): device time
hipError_t match_features_device(const double *h_fa, int64_t na, const double *h_fb, int64_t nb, int dim, int32_t *h_nn,
                                 double *h_d2, double *kernel_ms, hipStream_t stream)
{
    if (kernel_ms) *kernel_ms = 0.0;
    if (dim < 1 || dim > 64 || na < 0 || nb < 0 || na > 0x7fffffff || nb > 0x7fffffff) return hipErrorInvalidValue;
    if (nb == 0) return hipSuccess;
    if (na == 0) {
        for (int64_t i = 0; i < nb; i++) {
            h_nn[i] = -1;
            if (h_d2) h_d2[i] = INFINITY;
        }
        return hipSuccess;
    }
    DevBufs B;
    DevEvents<2> ev;
    double *d_fa = nullptr, *d_fb = nullptr, *d_d2 = nullptr;
    int *d_nn = nullptr;
    VISMA_TRY(B.alloc(&d_fa, (size_t)na * dim));
    VISMA_TRY(B.alloc(&d_fb, (size_t)nb * dim));
    VISMA_TRY(B.alloc(&d_nn, (size_t)nb));
    VISMA_TRY(B.alloc(&d_d2, (size_t)nb));
    VISMA_TRY(ev.create());
    VISMA_TRY(hipMemcpyAsync(d_fa, h_fa, sizeof(double) * (size_t)na * dim, hipMemcpyHostToDevice, stream));
    VISMA_TRY(hipMemcpyAsync(d_fb, h_fb, sizeof(double) * (size_t)nb * dim, hipMemcpyHostToDevice, stream));
    const dim3 grid((unsigned)((nb + kMatchThreads - 1) / kMatchThreads)), block(kMatchThreads);
    VISMA_TRY(hipEventRecord(ev[0], stream));
    if (dim <= 4) hipLaunchKernelGGL(match_features_kernel<4>, grid, block, 0, stream, d_fa, (long long)na, d_fb, (long long)nb, dim, d_nn, d_d2);
    else if (dim <= 16) hipLaunchKernelGGL(match_features_kernel<16>, grid, block, 0, stream, d_fa, (long long)na, d_fb, (long long)nb, dim, d_nn, d_d2);
    else if (dim <= 36) hipLaunchKernelGGL(match_features_kernel<36>, grid, block, 0, stream, d_fa, (long long)na, d_fb, (long long)nb, dim, d_nn, d_d2);
    else hipLaunchKernelGGL(match_features_kernel<64>, grid, block, 0, stream, d_fa, (long long)na, d_fb, (long long)nb, dim, d_nn, d_d2);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(hipEventRecord(ev[1], stream));
    VISMA_TRY(hipMemcpyAsync(h_nn, d_nn, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, stream));
    if (h_d2) VISMA_TRY(hipMemcpyAsync(h_d2, d_d2, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    if (kernel_ms) {
        float t = 0.f;
        VISMA_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        *kernel_ms = (double)t;
    }
    return hipSuccess;
}

}  // namespace visma
