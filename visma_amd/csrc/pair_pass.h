// pair_pass.h -- the frame of every reduction over the pairs of the last nn_pass (trim.hip, robust.hip, gicp.hip,
// colored.hip, information.hip), once: the grid-stride loop over the source positions, the workgroup's partial row, the
// ticket hand-off to the last workgroup, its fold of the rows and the publication to the host.  A pass file holds its
// arithmetic only, as a small struct:
//
//   struct Pass {
//       using Args = ...;                          // derived from PairPassArgs (kernels.h): the kernel's one argument
//       static constexpr int kAcc = ...;           // f64 accumulators per thread = columns of a partial row that are used
//       static constexpr int kPublished = ...;     // granules to the host
//       static constexpr bool kPublishTotals;      // true: the column totals are what is published, there is no finish()
//       __device__ explicit Pass(const Args &a);   // per-launch state, read once before the loop
//       template <bool S64> __device__ void visit(const Args &a, long long i, int j, double *acc);
//                                                  // EVERY source position i, j = a.idx[i] (< 0: no pair -- the passes with
//                                                  // an output per position write it there, too)
//       __device__ void finish(const double *tot, double *stats) const;
//                                                  // thread 0 of the last workgroup: tot[0 .. kAcc) -> stats[0 .. kPublished)
//   };
//
// The hand-off is the agent-scope recipe of device_common.h (block_reduce_store with write-through stores,
// pair_pass_fold, publish_tagged_stats): rows of kPairRow doubles of which the first kAcc are stored and read, at most
// kPairMaxBlocks of them, the ticket a.ticket re-armed by the last workgroup.  The order of every addition is fixed by
// (grid, kAcc) alone: a run is bit-identical to itself.  No floating-point atomics.
#pragma once

#include "device_common.h"

namespace visma {

// v = the point at position i: its f64 copy where the pass reads those (S64) and the copy exists (a normal has one or
// not on its own), else the fp32 one
template <bool S64>
__device__ __forceinline__ void pair_load3(const float4 *a32, const Pt64 *a64, long long i, double v[3])
{
    if (S64 && a64) { const Pt64 t = a64[i]; v[0] = t.x; v[1] = t.y; v[2] = t.z; }
    else { const float4 t = a32[i]; v[0] = (double)t.x; v[1] = (double)t.y; v[2] = (double)t.z; }
}

// t = T64 * s: the expression of accumulate_pair_d (the statistics do not depend on which entry point formed it)
__device__ __forceinline__ void pair_transform(const Xform64 &T64, const double s[3], double t[3])
{
    t[0] = T64.m[0] * s[0] + T64.m[1] * s[1] + T64.m[2] * s[2] + T64.m[3];
    t[1] = T64.m[4] * s[0] + T64.m[5] * s[1] + T64.m[6] * s[2] + T64.m[7];
    t[2] = T64.m[8] * s[0] + T64.m[9] * s[1] + T64.m[10] * s[2] + T64.m[11];
}

// S64: the launcher saw the f64 copies of the points (the host sets both or neither)
template <bool S64>
__device__ __forceinline__ void pair_assume_views(const PairPassArgs &a)
{
    if constexpr (S64) __builtin_assume(a.src64 != nullptr && a.tgt64 != nullptr);
}

template <class Pass, bool S64>
__global__ __launch_bounds__(kPairThreads) void pair_reduce_kernel(typename Pass::Args a)
{
    static_assert(Pass::kAcc <= kPairRow && kPairRow <= 32, "a partial row holds every accumulator; the fold has 32 columns");
    static_assert(Pass::kPublished <= kPairMaxPublished, "the pair passes share one scratch");
    __shared__ double f_tot[32];
    const int tid = threadIdx.x;
    pair_assume_views<S64>(a);
    Pass pass(a);
    double acc[Pass::kAcc];
#pragma unroll
    for (int k = 0; k < Pass::kAcc; k++) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * kPairThreads + tid; i < a.ns; i += (long long)gridDim.x * kPairThreads)
        pass.template visit<S64>(a, i, a.idx[i], acc);
    block_reduce_store<Pass::kAcc, kPairThreads / 64, false, kPairRow>(acc, a.partials, true);
    if (!pair_pass_fold<Pass::kAcc, kPairRow>(a.partials, a.ticket, f_tot)) return;
    if constexpr (Pass::kPublishTotals) {
        publish_tagged_stats<Pass::kPublished>(f_tot, a.host_out, a.seq);
    } else {
        __shared__ double f_stats[Pass::kPublished];
        if (tid == 0) pass.finish(f_tot, f_stats);
        publish_tagged_stats<Pass::kPublished>(f_stats, a.host_out, a.seq);
    }
}

// s64: which instantiation -- the one that reads the f64 copies of the points
template <class Pass>
hipError_t launch_pair_reduce(const typename Pass::Args &a, bool s64, hipStream_t stream)
{
    const dim3 grid((unsigned)pair_reduce_blocks(a.ns)), block(kPairThreads);
    if (s64) hipLaunchKernelGGL((pair_reduce_kernel<Pass, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((pair_reduce_kernel<Pass, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace visma
