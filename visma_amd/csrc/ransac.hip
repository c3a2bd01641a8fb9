// ransac.hip -- the trial loop of RANSAC global registration on gfx950 (open3d::RegistrationRANSACBasedOnFeatureMatching /
// ...BasedOnCorrespondence, O3D/Core/Registration/Registration.cpp:188-353): one lane per trial over a chunk of trials,
// both clouds, the normals and the pair table resident for the call.  The arithmetic of a trial is ransac.hpp's, the
// same functions visma_icp_ransac_hypotheses_host runs.
//
// ransac_trial_kernel runs the whole trial per lane; lanes the edge-length checker rejects return early.  (A version in two
// stages -- edge test over all trials, ordered compaction, solve over the survivors only -- was built and measured: 0.91 ms
// against 0.57 ms at 4,000,000 trials; the faster one is kept.)  Every trial leaves a verdict byte and,
// where it was solved, its T in the slot of its own trial; the trials that passed are then compacted IN TRIAL ORDER: a flag
// per trial, one workgroup that counts its 1,024 contiguous segments, scans the counts in LDS and writes the indices -- no
// atomic anywhere, so the list, and with it which trials get validated, does not depend on how the launch was scheduled.
//
// ransac_score_kernel: EvaluateRANSACBasedOnCorrespondence (:98-123), one workgroup per trial over the K pairs; every
// thread sums its pairs c = tid, tid + 256, ... in that order, the 256 partial sums are folded by a fixed tree: the
// same bits every run.
#include "device_common.h"
#include "ransac.hpp"

#include <algorithm>
#include <vector>

namespace visma {

namespace {

constexpr int kRansacThreads = 256;
constexpr int kCompactThreads = 1024;

template <int N>
__global__ __launch_bounds__(kRansacThreads) void ransac_trial_kernel(RansacView v, long long t0, int n,
                                                                      signed char *__restrict__ verdict, double *__restrict__ T_slot)
{
    const int i = blockIdx.x * kRansacThreads + threadIdx.x;
    if (i >= n) return;
    double T[12];
    const int r = ransac_trial<N>(v, t0 + i, T);
    verdict[i] = (signed char)r;
    if (r == kRansacBefore) return;
#pragma unroll
    for (int k = 0; k < 12; k++) T_slot[(size_t)i * 12 + k] = T[k];
}

// idx[0 .. *count) = the i in [0, n) with flag[i] == want, ascending.  One workgroup; every thread owns a contiguous
// segment whose length is a multiple of 16 and reads it 16 flags at a time (flag is a hipMalloc'd array: 16-byte aligned).
__global__ __launch_bounds__(kCompactThreads) void ransac_compact_kernel(const signed char *__restrict__ flag, int n, int want,
                                                                         int *__restrict__ idx, int *__restrict__ count)
{
    __shared__ int s[kCompactThreads];
    const int tid = threadIdx.x;
    const int per = (((n + kCompactThreads - 1) / kCompactThreads) + 15) & ~15;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    const unsigned w = (unsigned)(want & 0xff);
    auto hits = [&](const unsigned x) {                           // bytes of x equal to want
        return (int)(((x & 0xffu) == w) + (((x >> 8) & 0xffu) == w) + (((x >> 16) & 0xffu) == w) + ((x >> 24) == w));
    };
    int c = 0;
    int i = lo;
    for (; i + 16 <= hi; i += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(flag + i);
        c += hits(v.x) + hits(v.y) + hits(v.z) + hits(v.w);
    }
    for (; i < hi; i++) c += flag[i] == want;
    s[tid] = c;
    __syncthreads();
    for (int d = 1; d < kCompactThreads; d <<= 1) {              // inclusive scan
        const int add = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    int o = s[tid] - c;
    if (c > 0) {
        i = lo;
        for (; i + 16 <= hi; i += 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(flag + i);
            if (hits(v.x) + hits(v.y) + hits(v.z) + hits(v.w) == 0) continue;
            for (int k = i; k < i + 16; k++)
                if (flag[k] == want) idx[o++] = k;
        }
        for (; i < hi; i++)
            if (flag[i] == want) idx[o++] = i;
    }
    if (tid == kCompactThreads - 1) *count = s[tid];
}

// T_out[k] = T_slot[idx[k]] for k < *count
__global__ __launch_bounds__(kRansacThreads) void ransac_gather_kernel(const int *__restrict__ idx, const int *__restrict__ count, int n,
                                                                       const double *__restrict__ T_slot, double *__restrict__ T_out)
{
    const int m = min(*count, n);
    for (int e = blockIdx.x * kRansacThreads + threadIdx.x; e < m * 12; e += gridDim.x * kRansacThreads) {
        const int k = e / 12, c = e - k * 12;
        T_out[e] = T_slot[(size_t)idx[k] * 12 + c];
    }
}

__global__ __launch_bounds__(kRansacThreads) void ransac_score_kernel(const double *__restrict__ src, const double *__restrict__ tgt,
                                                                      const int *__restrict__ ps, const int *__restrict__ pt,
                                                                      long long K, const double *__restrict__ Ts, double max_dis2,
                                                                      long long *__restrict__ good_out, double *__restrict__ err2_out)
{
    __shared__ double s_e[kRansacThreads];
    __shared__ int s_g[kRansacThreads];
    const int tid = threadIdx.x;
    double T[12];
#pragma unroll
    for (int c = 0; c < 12; c++) T[c] = Ts[(size_t)blockIdx.x * 12 + c];
    double e = 0.0;
    int g = 0;
    for (long long c = tid; c < K; c += kRansacThreads) {
        const double d2 = ransac_pair_dis2(src, tgt, ps[c], pt[c], T);
        if (d2 < max_dis2) { g++; e += d2; }
    }
    s_e[tid] = e;
    s_g[tid] = g;
    __syncthreads();
    for (int d = kRansacThreads / 2; d > 0; d >>= 1) {
        if (tid < d) { s_e[tid] += s_e[tid + d]; s_g[tid] += s_g[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) { good_out[blockIdx.x] = s_g[0]; err2_out[blockIdx.x] = s_e[0]; }
}

}  // namespace

struct RansacDevice : DevBufs {
    DevEvents<2> ev;
    hipStream_t stream = nullptr;
    RansacView v;                       // device pointers
    int n = 0;                          // ransac_n
    int64_t cap = 0;                    // trials per chunk at most
    int64_t n_draw_trials = -1;         // trials the draws cover (-1: seeded)
    signed char *verdict = nullptr;
    double *T_slot = nullptr, *T_out = nullptr;
    int *idx = nullptr, *cnt = nullptr;                      // *cnt: trials of the chunk that passed
    template <class T>
    hipError_t upload(const T **out, const T *h, size_t count)
    {
        T *d = nullptr;
        hipError_t e = alloc(&d, count);
        if (e != hipSuccess) return e;
        *out = d;
        return count ? hipMemcpyAsync(d, h, sizeof(T) * count, hipMemcpyHostToDevice, stream) : hipSuccess;
    }
};

#define RANSAC_FOR_N(n, CALL)                                     \
    switch (n) {                                                  \
    case 3: CALL(3); break;                                       \
    case 4: CALL(4); break;                                       \
    case 5: CALL(5); break;                                       \
    case 6: CALL(6); break;                                       \
    case 7: CALL(7); break;                                       \
    default: CALL(8); break;                                      \
    }

static hipError_t ransac_device_create_impl(const RansacProblem &p, int64_t chunk_cap, hipStream_t stream, RansacDevice *D)
{
    if (p.ransac_n < kRansacMinN || p.ransac_n > kRansacMaxN || p.ns <= 0 || p.nt <= 0 || p.n_pairs <= 0 || chunk_cap <= 0 ||
        chunk_cap > (1 << 22) || p.ns > 0x7fffffff || p.nt > 0x7fffffff || p.n_pairs > 0x7fffffff)
        return hipErrorInvalidValue;
    D->stream = stream;
    D->n = p.ransac_n;
    D->cap = chunk_cap;
    D->n_draw_trials = p.draws ? p.n_draw_trials : -1;
    RansacView &v = D->v;
    VISMA_TRY(D->upload(&v.src, p.src, (size_t)p.ns * 3));
    VISMA_TRY(D->upload(&v.tgt, p.tgt, (size_t)p.nt * 3));
    if (p.src_n && p.tgt_n) {
        VISMA_TRY(D->upload(&v.src_n, p.src_n, (size_t)p.ns * 3));
        VISMA_TRY(D->upload(&v.tgt_n, p.tgt_n, (size_t)p.nt * 3));
    }
    if (p.pair_src) VISMA_TRY(D->upload(&v.pair_src, p.pair_src, (size_t)p.n_pairs));
    VISMA_TRY(D->upload(&v.pair_tgt, p.pair_tgt, (size_t)p.n_pairs));
    if (p.draws) VISMA_TRY(D->upload(&v.draws, p.draws, (size_t)p.n_draw_trials * p.ransac_n));
    v.n_pairs = p.n_pairs;
    v.seed = p.seed;
    v.edge = p.edge; v.dist = p.dist; v.cos_normal = p.cos_normal;
    v.use_edge = p.use_edge; v.use_dist = p.use_dist; v.use_normal = p.use_normal;
    VISMA_TRY(D->alloc(&D->verdict, (size_t)chunk_cap));
    VISMA_TRY(D->alloc(&D->T_slot, (size_t)chunk_cap * 12));
    VISMA_TRY(D->alloc(&D->T_out, (size_t)chunk_cap * 12));
    VISMA_TRY(D->alloc(&D->idx, (size_t)chunk_cap));
    VISMA_TRY(D->alloc(&D->cnt, 1));
    VISMA_TRY(D->ev.create());
    return hipStreamSynchronize(stream);
}

hipError_t ransac_device_create(const RansacProblem &p, int64_t chunk_cap, hipStream_t stream, RansacDevice **out)
{
    RansacDevice *D = new RansacDevice;
    const hipError_t e = ransac_device_create_impl(p, chunk_cap, stream, D);
    if (e != hipSuccess) { delete D; D = nullptr; }
    *out = D;
    return e;
}

void ransac_device_destroy(RansacDevice *D) { delete D; }

hipError_t ransac_device_chunk(RansacDevice *D, int64_t t0, int64_t n64, int8_t *h_verdict, double *h_T_all,
                               std::vector<int64_t> *pass_trial, std::vector<double> *pass_T, double *ms)
{
    if (!D || n64 <= 0 || n64 > D->cap || t0 < 0 || !h_verdict) return hipErrorInvalidValue;
    if (D->n_draw_trials >= 0 && t0 + n64 > D->n_draw_trials) return hipErrorInvalidValue;     // (the draws end here)
    const int n = (int)n64;
    hipStream_t st = D->stream;
    const dim3 block(kRansacThreads), grid((unsigned)((n + kRansacThreads - 1) / kRansacThreads));
    VISMA_TRY(hipEventRecord(D->ev[0], st));
#define RANSAC_ONE(N) hipLaunchKernelGGL(ransac_trial_kernel<N>, grid, block, 0, st, D->v, (long long)t0, n, D->verdict, D->T_slot)
    RANSAC_FOR_N(D->n, RANSAC_ONE)
#undef RANSAC_ONE
    VISMA_TRY(hipGetLastError());
    hipLaunchKernelGGL(ransac_compact_kernel, dim3(1), dim3(kCompactThreads), 0, st, D->verdict, n, kRansacPass, D->idx, D->cnt);
    VISMA_TRY(hipGetLastError());
    hipLaunchKernelGGL(ransac_gather_kernel, dim3(std::min<unsigned>(grid.x, 256u)), block, 0, st, D->idx, D->cnt, n, D->T_slot, D->T_out);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(hipEventRecord(D->ev[1], st));
    int h_cnt = 0;
    VISMA_TRY(hipMemcpyAsync(&h_cnt, D->cnt, sizeof(int), hipMemcpyDeviceToHost, st));
    VISMA_TRY(hipMemcpyAsync(h_verdict, D->verdict, (size_t)n, hipMemcpyDeviceToHost, st));
    std::vector<double> t12;
    if (h_T_all) {
        t12.resize((size_t)n * 12);
        VISMA_TRY(hipMemcpyAsync(t12.data(), D->T_slot, sizeof(double) * 12 * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    VISMA_TRY(hipStreamSynchronize(st));
    if (ms) {
        float t = 0.f;
        VISMA_TRY(hipEventElapsedTime(&t, D->ev[0], D->ev[1]));
        *ms += (double)t;
    }
    auto widen = [](const double *t12, double *t16) {
        for (int c = 0; c < 12; c++) t16[c] = t12[c];
        t16[12] = t16[13] = t16[14] = 0.0;
        t16[15] = 1.0;
    };
    if (h_T_all)
        for (int i = 0; i < n; i++) {
            if (h_verdict[i] == kRansacBefore) std::fill(h_T_all + (size_t)i * 16, h_T_all + (size_t)i * 16 + 16, 0.0);
            else widen(&t12[(size_t)i * 12], h_T_all + (size_t)i * 16);
        }
    if (h_cnt < 0 || h_cnt > n) return hipErrorUnknown;
    if (pass_trial && pass_T && h_cnt > 0) {
        std::vector<int> idx((size_t)h_cnt);
        std::vector<double> T((size_t)h_cnt * 12);
        VISMA_TRY(hipMemcpyAsync(idx.data(), D->idx, sizeof(int) * (size_t)h_cnt, hipMemcpyDeviceToHost, st));
        VISMA_TRY(hipMemcpyAsync(T.data(), D->T_out, sizeof(double) * 12 * (size_t)h_cnt, hipMemcpyDeviceToHost, st));
        VISMA_TRY(hipStreamSynchronize(st));
        for (int k = 0; k < h_cnt; k++) {
            pass_trial->push_back(t0 + idx[(size_t)k]);
            pass_T->resize(pass_T->size() + 16);
            widen(&T[(size_t)k * 12], pass_T->data() + pass_T->size() - 16);
        }
    }
    return hipSuccess;
}

// h_T: n x 16 row-major; h_good / h_err2: per trial the pairs with dis2 < max_dist^2 and the sum of their dis2
hipError_t ransac_score_device(RansacDevice *D, const double *h_T, int64_t n, double max_dist, int64_t *h_good, double *h_err2)
{
    if (!D || !D->v.pair_src || n < 0 || !h_T || !h_good || !h_err2) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    hipStream_t st = D->stream;
    std::vector<double> t12((size_t)n * 12);
    for (int64_t i = 0; i < n; i++) std::copy(h_T + 16 * i, h_T + 16 * i + 12, t12.begin() + 12 * i);
    double *d_T = nullptr, *d_e = nullptr;
    long long *d_g = nullptr;
    VISMA_TRY(D->alloc(&d_T, (size_t)n * 12));
    VISMA_TRY(D->alloc(&d_e, (size_t)n));
    VISMA_TRY(D->alloc(&d_g, (size_t)n));
    VISMA_TRY(hipMemcpyAsync(d_T, t12.data(), sizeof(double) * 12 * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ransac_score_kernel, dim3((unsigned)n), dim3(kRansacThreads), 0, st, D->v.src, D->v.tgt, D->v.pair_src,
                       D->v.pair_tgt, D->v.n_pairs, d_T, max_dist * max_dist, d_g, d_e);
    VISMA_TRY(hipGetLastError());
    std::vector<long long> g((size_t)n);
    VISMA_TRY(hipMemcpyAsync(g.data(), d_g, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, st));
    VISMA_TRY(hipMemcpyAsync(h_err2, d_e, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    VISMA_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; i++) h_good[i] = (int64_t)g[(size_t)i];
    return hipSuccess;
}

}  // namespace visma
