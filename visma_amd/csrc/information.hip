// information.hip -- the information matrix of a registered pair of clouds (Open3D's GetInformationMatrixFromPointClouds,
// Registration.cpp:352-413; Choi, Zhou, Koltun: "Robust Reconstruction of Indoor Scenes", CVPR 2015) on gfx950: the
// weight a pose-graph edge enters the global optimisation with.  Per pair of the last nn_pass, with q the TARGET point
// in the caller's frame, G = [-hat(q) | I] (3 x 6) and the result is sum G^T G -- WITHOUT the identity terms the
// reference adds (visma_icp.h states the deviation).
//
//  information_reduce_kernel<T64>   per pair: q = t_j + off as gicp.hip forms it, then the ten sums the 6 x 6 consists of:
//                                   K, sum x, y, z, sum xx, yy, zz, xy, xz, yz.  Then the pair-pass tail the trimmed, the
//                                   robust and the generalized reduction end in (device_common.h: block_reduce_store,
//                                   pair_pass_fold, publish_tagged_stats) with rows of kInfoRow doubles: the last
//                                   workgroup has the column totals and publishes them; information_from_sums
//                                   (host_math.hpp) lays them out as the matrix.
//  ... one launch per edge: the batched entry point (visma_icp_information_matrices) is a host loop over edges that
//  uploads a shared target once, so an edge's sums never depend on what else the call computed.  A second entry that
//  reduces many edges in one launch was deliberately not built: it needs every edge's winners on the device at once,
//  which the per-edge search does not leave.
// The source's coordinates are not read: only which source positions have a pair.  A target point is never an index or
// an address: a non-finite one reaches the sums only.
// No floating-point atomics: a run is bit-identical to itself.  (Reasoning and numbers: DESIGN.md 4.4c9.)
#include "device_common.h"

namespace visma {

namespace {

constexpr int kInfoThreads = 256;
static_assert(kInfoAcc <= kInfoRow && kInfoRow <= 32, "a partial row holds every accumulator; the fold has 32 columns");
static_assert(kInfoRow <= kRobustRow && kInfoAcc <= kRobustPublished, "the pair passes share one scratch, sized for the robust pass");

}  // namespace

template <bool T64>
__global__ __launch_bounds__(kInfoThreads) void information_reduce_kernel(InformationArgs a)
{
    __shared__ double f_tot[32];
    const int tid = threadIdx.x;
    double acc[kInfoAcc];
#pragma unroll
    for (int k = 0; k < kInfoAcc; k++) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * kInfoThreads + tid; i < a.ns; i += (long long)gridDim.x * kInfoThreads) {
        const int j = a.idx[i];
        if (j < 0) continue;
        double q[3];
        if (T64) { const Pt64 t = a.tgt64[j]; q[0] = t.x; q[1] = t.y; q[2] = t.z; }
        else { const float4 t = a.tgt[j]; q[0] = (double)t.x; q[1] = (double)t.y; q[2] = (double)t.z; }
        // into the frame of `off`: the caller's
        const double x = q[0] + a.off.v[0], y = q[1] + a.off.v[1], z = q[2] + a.off.v[2];
        acc[0] += 1.0;
        acc[1] += x; acc[2] += y; acc[3] += z;
        acc[4] += x * x; acc[5] += y * y; acc[6] += z * z;
        acc[7] += x * y; acc[8] += x * z; acc[9] += y * z;
    }
    block_reduce_store<kInfoAcc, kInfoThreads / 64, false, kInfoRow>(acc, a.partials, true);
    if (!pair_pass_fold<kInfoAcc, kInfoRow>(a.partials, a.ticket, f_tot)) return;
    publish_tagged_stats<kInfoAcc>(f_tot, a.host_out, a.seq);
}

hipError_t launch_information_reduce(const InformationArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)robust_reduce_blocks(a.ns)), block(kInfoThreads);
    if (a.tgt64) hipLaunchKernelGGL(information_reduce_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(information_reduce_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace visma
