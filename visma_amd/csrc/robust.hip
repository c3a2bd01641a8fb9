// robust.hip -- robust ICP (M-estimators, iteratively re-weighted least squares) on gfx950: every pair of a pass enters
// the statistics with a weight w(r) of its own residual r (Huber 1964; Beaton & Tukey 1974; Cauchy: Fitzgibbon 2003;
// tuning constants of Holland & Welsch 1977), the scale c either the caller's or tune * 1.4826 * the median residual.
//
//  robust_residual_kernel<S64>     point-to-plane with the automatic scale only: (float)(r_i^2) per source position, the
//                                  ranking value of the median select (trim_select_kernel of trim.hip, unchanged; the
//                                  point-to-point select runs over the pass's own fp32 d2).
//  RobustReduce<PLANE>             per pair: p, q (and n) as the plain reduction forms them, the residual, the weight,
//                                  and w times the pair's contribution to every accumulator of Acc<PLANE>; w per source
//                                  position goes to memory.  Automatic scale: the median's bit pattern is read from the
//                                  select's state word and c is formed here in f64 -- no host round trip between select
//                                  and reduction.  In the frame of pair_pass.h; the last workgroup expands the moments
//                                  and publishes 38 statistics, c, v, the pairs with w == 0 and sum w r^2.
// No floating-point atomics: a run is bit-identical to itself.  (Reasoning and numbers: DESIGN.md 4.4c4.)
#include "pair_pass.h"

namespace visma {

namespace {

constexpr int kRobustExtra = 2;                        // behind the accumulators of Acc<PLANE>: pairs with w == 0, sum w r^2

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

// One pair as the plain reduction sees it: t = T64 * s, q, n; returns the residual in the frame of `off` (|p - q|, or
// |(p - q) . n| with PLANE)
template <bool PLANE, bool S64>
__device__ __forceinline__ double pair_residual(const RobustArgs &a, long long i, int j, double t[3], double q[3], double n[3])
{
    double s[3];
    pair_load3<S64>(a.src, a.src64, i, s);
    pair_load3<S64>(a.tgt, a.tgt64, j, q);
    n[0] = n[1] = n[2] = 0.0;
    if constexpr (PLANE) pair_load3<S64>(a.nrm, a.nrm64, j, n);
    pair_transform(a.T64, s, t);
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = (t[k] + a.off.v[k]) - (q[k] + a.off.v[k]);
    if constexpr (PLANE) return fabs(d[0] * n[0] + d[1] * n[1] + d[2] * n[2]);
    else return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

}  // namespace

template <bool S64>
__global__ __launch_bounds__(kPairThreads) void robust_residual_kernel(RobustArgs a)
{
    pair_assume_views<S64>(a);
    for (long long i = (long long)blockIdx.x * kPairThreads + threadIdx.x; i < a.ns; i += (long long)gridDim.x * kPairThreads) {
        const int j = a.idx[i];
        float v = 0.f;
        if (j >= 0) {
            double t[3], q[3], n[3];
            const double r = pair_residual<true, S64>(a, i, j, t, q, n);
            v = (float)(r * r);
        }
        a.r2_out[i] = v;
    }
}

template <bool PLANE>
struct RobustReduce {
    using Args = RobustArgs;
    static constexpr int NACC = Acc<PLANE>::N;
    static constexpr int kAcc = NACC + kRobustExtra;
    static constexpr int kPublished = kRobustPublished;
    static constexpr bool kPublishTotals = false;
    double c, v;

    // the scale: the caller's, or from the median the select left in its state word
    __device__ explicit RobustReduce(const Args &a)
    {
        c = a.scale; v = 0.0;
        if (a.auto_scale) {
            const unsigned vbits = ld_agent_u32(a.select_work + kSelectStateWord);
            v = (double)__uint_as_float(vbits);
            const double cm = a.tune_k * sqrt(v);            // tune_k = tune * 1.4826, formed on the host
            c = cm > a.min_scale ? cm : a.min_scale;
        }
    }
    template <bool S64>
    __device__ __forceinline__ void visit(const Args &a, long long i, int j, double *acc)
    {
        double w = 0.0;
        if (j >= 0) {
            double t[3], q[3], n[3];
            const double r = pair_residual<PLANE, S64>(a, i, j, t, q, n);
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
    __device__ void finish(const double *tot, double *stats) const
    {
        expand_moments<PLANE>(tot, stats);
        stats[kNStats] = c;
        stats[kNStats + 1] = v;                              // the median's square as the select ranked it (0: fixed scale)
        stats[kNStats + 2] = tot[NACC];                      // pairs with w == 0
        stats[kNStats + 3] = tot[NACC + 1];                  // sum w r^2
    }
};

hipError_t launch_robust_residual(const RobustArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)pair_reduce_blocks(a.ns)), block(kPairThreads);
    if (a.src64) hipLaunchKernelGGL(robust_residual_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(robust_residual_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_robust_reduce(const RobustArgs &a, int plane, hipStream_t stream)
{
    return plane ? launch_pair_reduce<RobustReduce<true>>(a, a.src64 != nullptr, stream) : launch_pair_reduce<RobustReduce<false>>(a, a.src64 != nullptr, stream);
}

}  // namespace visma
