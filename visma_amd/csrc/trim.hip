// trim.hip -- trimmed ICP (Chetverikov et al., ICPR 2002) on gfx950: of the K pairs of a pass only the m with the
// smallest key (d2, source index) enter the statistics.
//
//  trim_select_kernel<ROUND>  exact m-th smallest fp32 squared distance among the pairs of the last pass (idx >= 0):
//                             a most-significant-digit radix select over the IEEE bit pattern (d2 >= 0: the bits order
//                             like the value), 11 + 11 + 10 bits.  Every workgroup builds the histogram of ITS queries in
//                             LDS and adds the non-empty bins to the launch's histogram (one atomicAdd per bin); the last
//                             workgroup to arrive (one ticket) picks the digit that holds rank `need` and leaves
//                             {prefix, need, ties} for the next round.  Integer counts only: the result does not depend on
//                             arrival order.  Round 2 ends with the cut distance v, the number of pairs AT v (ties) and how
//                             many of them are kept (need).  need < ties -- a tie straddles the cut -- is decided by the
//                             caller's source index: the same select over the 32 index bits of the tied pairs, run by
//                             that last workgroup alone (rare; the price is three scans of the queries by 256 threads).
//  TrimReduce                 the reduction's arithmetic (accumulate_pq_d, device_common.h) over the pairs with key
//                             (d2 bits << 32 | source index) <= cut key, and the kept mask, in the frame of pair_pass.h;
//                             the last workgroup expands the moments and publishes statistics, cut distance and kept count.
// No sort, no copy of the distances to the host.  Four launches per pass (reasoning and numbers: DESIGN.md).
#include "pair_pass.h"

namespace visma {

namespace {

constexpr int kTrimThreads = kPairThreads;

// All 256 threads: the bin of h[0 .. NB) that holds rank `need` (1-based, need <= sum of h) and the count of the bins
// before it.  Results in res[0] (bin), res[1] (before); h is left as it was.
template <int NB>
__device__ __forceinline__ void find_bin(const unsigned *h, unsigned need, unsigned *scan, unsigned *res)
{
    constexpr int PER = NB / kTrimThreads;
    const int tid = threadIdx.x;
    unsigned own = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) own += h[tid * PER + k];
    scan[tid] = own;
    __syncthreads();
    // inclusive scan over the 256 chunk sums (Hillis-Steele, 8 steps)
    for (int o = 1; o < kTrimThreads; o <<= 1) {
        const unsigned add = tid >= o ? scan[tid - o] : 0u;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const unsigned incl = scan[tid], excl = incl - own;
    if (excl < need && need <= incl) {
        unsigned cum = excl;
        int b = tid * PER;
        for (int k = 0; k < PER; k++, b++) {
            const unsigned c = h[b];
            if (cum + c >= need) break;
            cum += c;
        }
        res[0] = (unsigned)b;
        res[1] = cum;
    }
    __syncthreads();
}

}  // namespace

// work: kTrimHistWords histogram words (3 rounds x 2048), then 4 tickets, then the state {prefix, need, ties, cut index}
template <int ROUND>
__global__ __launch_bounds__(kTrimThreads) void trim_select_kernel(const float *__restrict__ d2, const int *__restrict__ idx,
                                                                  const int *__restrict__ order, int ns, unsigned m,
                                                                  unsigned *__restrict__ work)
{
    constexpr int BITS = ROUND == 2 ? 10 : 11;
    constexpr int NB = 1 << BITS;
    constexpr int SHIFT = ROUND == 0 ? 21 : (ROUND == 1 ? 10 : 0);
    __shared__ unsigned h[2048];
    __shared__ unsigned scan[kTrimThreads];
    __shared__ unsigned res[2];
    __shared__ int last;
    const int tid = threadIdx.x;
    unsigned *hist = work + ROUND * 2048;
    unsigned *tickets = work + kTrimHistWords;
    unsigned *state = tickets + 4;
    unsigned prefix = 0u, need = m;
    if (ROUND > 0) { prefix = ld_agent_u32(state); need = ld_agent_u32(state + 1); }
    for (int b = tid; b < NB; b += kTrimThreads) h[b] = 0u;
    __syncthreads();
    const long long stride = (long long)gridDim.x * kTrimThreads;
    for (long long i0 = (long long)blockIdx.x * kTrimThreads + tid; i0 < ns; i0 += 4 * stride) {
        unsigned bits[4];
        int j[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {                      // four independent loads in flight
            const long long i = i0 + u * stride;
            j[u] = -1;
            bits[u] = 0u;
            if (i < ns) { j[u] = idx[i]; bits[u] = __float_as_uint(d2[i]); }
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (j[u] >= 0 && (ROUND == 0 || (bits[u] >> (SHIFT + BITS)) == prefix)) atomicAdd(&h[(bits[u] >> SHIFT) & (NB - 1)], 1u);
    }
    __syncthreads();
    for (int b = tid; b < NB; b += kTrimThreads) {
        const unsigned c = h[b];
        if (c) __hip_atomic_fetch_add(hist + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(tickets + ROUND, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1u ? 1 : 0;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            st_agent_u32(tickets + ROUND, 0u);               // re-armed for the next pass
        }
    }
    __syncthreads();
    if (!last) return;
    for (int b = tid; b < NB; b += kTrimThreads) {
        h[b] = ld_agent_u32(hist + b);
        st_agent_u32(hist + b, 0u);                          // ... and so is the histogram
    }
    __syncthreads();
    find_bin<NB>(h, need, scan, res);
    prefix = (prefix << BITS) | res[0];
    need -= res[1];
    const unsigned ties = h[res[0]];
    unsigned cut = 0xFFFFFFFFu;
    if (ROUND == 2 && need < ties) {
        // pairs AT the cut distance on both sides of the cut: the `need` lowest source indices stay
        unsigned ipre = 0u;
        for (int r = 0; r < 3; r++) {
            const int bits_r = r == 2 ? 10 : 11, shift_r = r == 0 ? 21 : (r == 1 ? 10 : 0);
            __syncthreads();
            for (int b = tid; b < 2048; b += kTrimThreads) h[b] = 0u;
            __syncthreads();
            for (int i = tid; i < ns; i += kTrimThreads) {
                if (idx[i] < 0 || __float_as_uint(d2[i]) != prefix) continue;
                const unsigned o = order ? (unsigned)order[i] : (unsigned)i;
                if (r == 0 || (o >> (shift_r + bits_r)) == ipre) atomicAdd(&h[(o >> shift_r) & ((1u << bits_r) - 1u)], 1u);
            }
            __syncthreads();
            find_bin<2048>(h, need, scan, res);              // (round 2: the upper 1024 bins are empty)
            ipre = (ipre << bits_r) | res[0];
            need -= res[1];
        }
        cut = ipre;
    }
    if (tid == 0) {
        st_agent_u32(state, prefix);
        st_agent_u32(state + 1, need);
        st_agent_u32(state + 2, ties);
        st_agent_u32(state + 3, cut);
    }
}

struct TrimReduce {
    using Args = TrimReduceArgs;
    static constexpr int kAcc = Acc<false>::N;
    static constexpr int kPublished = kTrimPublished;
    static constexpr bool kPublishTotals = false;
    unsigned vbits;
    unsigned long long cut_key;

    __device__ explicit TrimReduce(const Args &a)
    {
        const unsigned *state = a.work + kSelectStateWord;
        vbits = ld_agent_u32(state);
        const unsigned cut_idx = ld_agent_u32(state + 3);
        cut_key = ((unsigned long long)vbits << 32) | cut_idx;
    }
    template <bool S64>
    __device__ __forceinline__ void visit(const Args &a, long long i, int j, double *acc)
    {
        const unsigned o = a.order ? (unsigned)a.order[i] : (unsigned)i;
        const unsigned long long key = ((unsigned long long)__float_as_uint(a.d2[i]) << 32) | o;
        const bool kept = j >= 0 && key <= cut_key;
        a.mask[i] = kept ? 1 : 0;
        if (kept) {
            double s[3], q[3], t[3];
            pair_load3<S64>(a.src, a.src64, i, s);
            pair_load3<S64>(a.tgt, a.tgt64, j, q);
            pair_transform(a.T64, s, t);
            accumulate_pq_d<false>(acc, t[0], t[1], t[2], q[0], q[1], q[2], 0.0, 0.0, 0.0, a.off);
        }
    }
    __device__ void finish(const double *tot, double *stats) const
    {
        expand_moments<false>(tot, stats);
        stats[kNStats] = (double)__uint_as_float(vbits);       // the cut: the largest kept d2
        stats[kNStats + 1] = tot[0];                           // kept pairs (= stats[0])
    }
};

int trim_select_blocks(int64_t ns)
{
    // few workgroups with many queries each: what costs is one atomicAdd per non-empty bin per workgroup
    const int64_t want = (ns + 4095) / 4096;
    return (int)(want < 1 ? 1 : (want > 128 ? 128 : want));
}

hipError_t launch_trim_select(const float *d2, const int32_t *idx, const int32_t *order, int64_t ns, unsigned m, unsigned *work,
                              hipStream_t stream)
{
    const dim3 grid((unsigned)trim_select_blocks(ns)), block(kTrimThreads);
    hipLaunchKernelGGL(trim_select_kernel<0>, grid, block, 0, stream, d2, idx, order, (int)ns, m, work);
    hipLaunchKernelGGL(trim_select_kernel<1>, grid, block, 0, stream, d2, idx, order, (int)ns, m, work);
    hipLaunchKernelGGL(trim_select_kernel<2>, grid, block, 0, stream, d2, idx, order, (int)ns, m, work);
    return hipGetLastError();
}

hipError_t launch_trim_reduce(const TrimReduceArgs &a, hipStream_t stream) { return launch_pair_reduce<TrimReduce>(a, a.src64 != nullptr, stream); }

}  // namespace visma
