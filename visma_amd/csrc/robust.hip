// robust.hip -- robust ICP (M-estimators, iteratively re-weighted least squares) on gfx950: every pair of a pass enters
// the statistics with a weight w(r) of its own residual r (Huber 1964; Beaton & Tukey 1974; Cauchy: Fitzgibbon 2003;
// tuning constants of Holland & Welsch 1977), the scale c either the caller's or tune * 1.4826 * the median residual.
//
//  robust_residual_kernel<S64>     point-to-plane with the automatic scale only: (float)(r_i^2) per source position, the
//                                  ranking value of the median select (trim_select_kernel of trim.hip, unchanged; the
//                                  point-to-point select runs over the pass's own fp32 d2).
//  robust_reduce_kernel<PLANE,S64> per pair: p, q (and n) as the plain reduction forms them, the residual, the weight,
//                                  and w times the pair's contribution to every accumulator of Acc<PLANE>; w per source
//                                  position goes to memory.  Automatic scale: the median's bit pattern is read from the
//                                  select's state word and c is formed here in f64 -- no host round trip between select
//                                  and reduction.  Then the pair-pass tail trim_reduce_kernel ends in (device_common.h:
//                                  block_reduce_store, pair_pass_fold, publish_tagged_stats) with rows of kRobustRow
//                                  doubles: the last workgroup has the column totals, expands the moments and
//                                  publishes 38 statistics, c, v, the pairs with w == 0 and sum w r^2.
// No floating-point atomics: a run is bit-identical to itself.  (Reasoning and numbers: DESIGN.md 4.4c4.)
#include "device_common.h"

namespace visma {

namespace {

constexpr int kRobustThreads = 256;
constexpr int kRobustExtra = 2;                        // behind the accumulators of Acc<PLANE>: pairs with w == 0, sum w r^2
static_assert(Acc<true>::N + kRobustExtra <= kRobustRow && kRobustRow <= 32, "a partial row holds every accumulator; the fold has 32 columns");

// the weight of a residual r >= 0 at scale c (visma_icp.h); c == 0 (or not positive): 1 for r == 0, else 0 -- never NaN
__device__ __forceinline__ double robust_weight(int kernel, double r, double c)
{
    if (!(c > 0.0)) return r == 0.0 ? 1.0 : 0.0;
    const double u = r / c;
    if (kernel == kRobustHuber) return r <= c ? 1.0 : c / r;
    if (kernel == kRobustTukey) {
        if (!(r < c)) return 0.0;
        const double t = 1.0 - u * u;
        return t * t;
    }
    return 1.0 / (1.0 + u * u);                        // Cauchy
}

// One pair as the plain reduction sees it: t = T64 * s (the expression of accumulate_pair_d), q, n; returns the
// residual in the frame of `off` (|p - q|, or |(p - q) . n| with PLANE)
template <bool PLANE, bool S64>
__device__ __forceinline__ double load_pair(const RobustArgs &a, long long i, int j, double t[3], double q[3], double n[3])
{
    double sx, sy, sz;
    if constexpr (S64) {
        const Pt64 s8 = a.src64[i], q8 = a.tgt64[j];
        sx = s8.x; sy = s8.y; sz = s8.z;
        q[0] = q8.x; q[1] = q8.y; q[2] = q8.z;
    } else {
        const float4 s4 = a.src[i], q4 = a.tgt[j];
        sx = (double)s4.x; sy = (double)s4.y; sz = (double)s4.z;
        q[0] = (double)q4.x; q[1] = (double)q4.y; q[2] = (double)q4.z;
    }
    n[0] = n[1] = n[2] = 0.0;
    if constexpr (PLANE) {
        if (S64 && a.nrm64) { const Pt64 n8 = a.nrm64[j]; n[0] = n8.x; n[1] = n8.y; n[2] = n8.z; }
        else { const float4 n4 = a.nrm[j]; n[0] = (double)n4.x; n[1] = (double)n4.y; n[2] = (double)n4.z; }
    }
    t[0] = a.T64.m[0] * sx + a.T64.m[1] * sy + a.T64.m[2] * sz + a.T64.m[3];
    t[1] = a.T64.m[4] * sx + a.T64.m[5] * sy + a.T64.m[6] * sz + a.T64.m[7];
    t[2] = a.T64.m[8] * sx + a.T64.m[9] * sy + a.T64.m[10] * sz + a.T64.m[11];
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = (t[k] + a.off.v[k]) - (q[k] + a.off.v[k]);
    if constexpr (PLANE) return fabs(d[0] * n[0] + d[1] * n[1] + d[2] * n[2]);
    else return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

}  // namespace

template <bool S64>
__global__ __launch_bounds__(kRobustThreads) void robust_residual_kernel(RobustArgs a)
{
    for (long long i = (long long)blockIdx.x * kRobustThreads + threadIdx.x; i < a.ns; i += (long long)gridDim.x * kRobustThreads) {
        const int j = a.idx[i];
        float v = 0.f;
        if (j >= 0) {
            double t[3], q[3], n[3];
            const double r = load_pair<true, S64>(a, i, j, t, q, n);
            v = (float)(r * r);
        }
        a.r2_out[i] = v;
    }
}

template <bool PLANE, bool S64>
__global__ __launch_bounds__(kRobustThreads) void robust_reduce_kernel(RobustArgs a)
{
    constexpr int NACC = Acc<PLANE>::N;
    constexpr int NROW = NACC + kRobustExtra;
    __shared__ double f_tot[32];
    __shared__ double f_stats[kRobustPublished];
    const int tid = threadIdx.x;
    // the scale: the caller's, or from the median the select left in its state word
    double c = a.scale, v = 0.0;
    if (a.auto_scale) {
        const unsigned vbits = ld_agent_u32(a.select_work + kTrimHistWords + 4);
        v = (double)__uint_as_float(vbits);
        const double cm = a.tune_k * sqrt(v);            // tune_k = tune * 1.4826, formed on the host
        c = cm > a.min_scale ? cm : a.min_scale;
    }
    double acc[NROW];
#pragma unroll
    for (int k = 0; k < NROW; k++) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * kRobustThreads + tid; i < a.ns; i += (long long)gridDim.x * kRobustThreads) {
        const int j = a.idx[i];
        double w = 0.0;
        if (j >= 0) {
            double t[3], q[3], n[3];
            const double r = load_pair<PLANE, S64>(a, i, j, t, q, n);
            w = robust_weight(a.kernel, r, c);
            // the pair's own contribution by the plain pass's arithmetic, then scaled: the plain and trimmed passes keep theirs
            double one[NACC];
#pragma unroll
            for (int k = 0; k < NACC; k++) one[k] = 0.0;
            accumulate_pq_d<PLANE>(one, t[0], t[1], t[2], q[0], q[1], q[2], n[0], n[1], n[2], a.off);
#pragma unroll
            for (int k = 0; k < NACC; k++) acc[k] += w * one[k];
            acc[NACC] += w == 0.0 ? 1.0 : 0.0;
            acc[NACC + 1] += w * (r * r);
        }
        a.w_out[i] = w;
    }
    block_reduce_store<NROW, kRobustThreads / 64, false, kRobustRow>(acc, a.partials, true);
    if (!pair_pass_fold<NROW, kRobustRow>(a.partials, a.ticket, f_tot)) return;
    if (tid == 0) {
        expand_moments<PLANE>(f_tot, f_stats);
        f_stats[kNStats] = c;
        f_stats[kNStats + 1] = v;                            // the median's square as the select ranked it (0: fixed scale)
        f_stats[kNStats + 2] = f_tot[NACC];                  // pairs with w == 0
        f_stats[kNStats + 3] = f_tot[NACC + 1];              // sum w r^2
    }
    publish_tagged_stats<kRobustPublished>(f_stats, a.host_out, a.seq);
}

int robust_reduce_blocks(int64_t ns) { return trim_reduce_blocks(ns); }

hipError_t launch_robust_residual(const RobustArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)robust_reduce_blocks(a.ns)), block(kRobustThreads);
    if (a.src64) hipLaunchKernelGGL(robust_residual_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(robust_residual_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_robust_reduce(const RobustArgs &a, int plane, hipStream_t stream)
{
    const dim3 grid((unsigned)robust_reduce_blocks(a.ns)), block(kRobustThreads);
    if (plane) {
        if (a.src64) hipLaunchKernelGGL((robust_reduce_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((robust_reduce_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (a.src64) hipLaunchKernelGGL((robust_reduce_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((robust_reduce_kernel<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace visma
