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
//  trim_reduce_kernel<S64>    the reduction's arithmetic (accumulate_pair / accumulate_pair_d, device_common.h) over
//                             the pairs with key (d2 bits << 32 | source index) <= cut key, the kept mask, then the
//                             pair-pass tail (device_common.h: block_reduce_store, pair_pass_fold,
//                             publish_tagged_stats): the last workgroup has the column totals, expands the moments and
//                             publishes statistics, cut distance and kept count.  No floating-point atomics: a run is
//                             bit-identical to itself.
// No sort, no copy of the distances to the host.  Four launches per pass (reasoning and numbers: DESIGN.md).
#include "device_common.h"

namespace visma {

namespace {

constexpr int kTrimThreads = 256;

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

template <bool S64>
__global__ __launch_bounds__(kTrimThreads) void trim_reduce_kernel(TrimReduceArgs a)
{
    constexpr int NACC = Acc<false>::N;
    __shared__ double f_tot[32];
    __shared__ double f_stats[kTrimPublished];
    const int tid = threadIdx.x;
    unsigned *tickets = a.work + kTrimHistWords;
    const unsigned *state = tickets + 4;
    const unsigned vbits = ld_agent_u32(state), cut_idx = ld_agent_u32(state + 3);
    const unsigned long long cut_key = ((unsigned long long)vbits << 32) | cut_idx;
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; k++) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * kTrimThreads + tid; i < a.ns; i += (long long)gridDim.x * kTrimThreads) {
        const int j = a.idx[i];
        const unsigned o = a.order ? (unsigned)a.order[i] : (unsigned)i;
        const unsigned long long key = ((unsigned long long)__float_as_uint(a.d2[i]) << 32) | o;
        const bool kept = j >= 0 && key <= cut_key;
        a.mask[i] = kept ? 1 : 0;
        if (kept) {
            if constexpr (S64) {
                const Pt64 s8 = a.src64[i], q8 = a.tgt64[j];
                accumulate_pair_d<false>(acc, s8.x, s8.y, s8.z, q8.x, q8.y, q8.z, 0.0, 0.0, 0.0, a.T64, a.off);
            } else {
                accumulate_pair<false>(acc, a.src[i], a.tgt[j], make_float4(0.f, 0.f, 0.f, 0.f), a.T64, a.off);
            }
        }
    }
    block_reduce_store<NACC>(acc, a.partials, true);
    if (!pair_pass_fold<NACC, kReduceAcc>(a.partials, tickets + 3, f_tot)) return;
    if (tid == 0) {
        expand_moments<false>(f_tot, f_stats);
        f_stats[kNStats] = (double)__uint_as_float(vbits);    // the cut: the largest kept d2
        f_stats[kNStats + 1] = f_tot[0];                       // kept pairs (= stats[0])
    }
    publish_tagged_stats<kTrimPublished>(f_stats, a.host_out, a.seq);
}

int trim_select_blocks(int64_t ns)
{
    // few workgroups with many queries each: what costs is one atomicAdd per non-empty bin per workgroup
    const int64_t want = (ns + 4095) / 4096;
    return (int)(want < 1 ? 1 : (want > 128 ? 128 : want));
}

int trim_reduce_blocks(int64_t ns)
{
    const int64_t want = (ns + kTrimThreads - 1) / kTrimThreads;
    return (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
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

hipError_t launch_trim_reduce(const TrimReduceArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)trim_reduce_blocks(a.ns)), block(kTrimThreads);
    if (a.src64) hipLaunchKernelGGL(trim_reduce_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(trim_reduce_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace visma
