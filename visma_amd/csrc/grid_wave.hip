// grid_wave.hip -- round 3's warm-started search kernel, kept for BATCHES (problems with their own clouds, sweeps over
// shared clouds): every wave searches its own 64 queries, no certificate, no workgroup barriers.  Measured against the
// certificate kernel of grid_coop.hip (round 4) on one box: config 3 986 k vs 888 k iterations/s, config 5 2.18 M vs
// 1.93 M, a 24-yaw sweep 0.92 vs 1.00 ms -- hundreds of small problems, 30 iterations each from far-off starts, with more
// waves than the chip holds: the waves of a workgroup in lock step through six barriers hide less latency than sixteen
// independent waves per CU.  Single registrations run grid_coop.hip.  The per-query state is grid_coop.hip's (Pt64: the
// winner's f64 point, index | LB << 32); this kernel reads the point and leaves LB = 0 (nothing certified from it).
//
// The search itself -- warm start, flattening, the exactness argument -- is described in grid_coop.hip and warm_search.h;
// the pieces the two kernels share are in warm_search.h.
#include "warm_search.h"

namespace visma {

namespace {

constexpr int kCoopCap = 512;                 // chunk descriptors per wave and list window (4 KiB)
#ifndef VISMA_WAVE_DEPTH
#define VISMA_WAVE_DEPTH 7
#endif
constexpr int kCoopDepth = VISMA_WAVE_DEPTH;  // chunks per lane octet in flight

}  // namespace


// Everything the launch is given, as ONE by-value argument read from the kernarg segment at the top of EVERY pass
// (warm_search.h: ld_karg; grid_coop.hip's persistent kernel does the same).
struct SweepParams {
    int ns; const float *s12f; const unsigned *start; GridParams g; float r2f; int *idx_out; float *d2_out; double *partials;
    unsigned long long *cand_count; DevIcpState *st; int bpp; long long out_stride; int nprob; const Pt64 *src64;
    const Pt64 *sorted64; FoldArgs fold; Pt64 *prevq_io; SweepArgs sa;
};

template <bool PLANE, bool ONE, bool SWEEP = false>
__device__ __forceinline__ bool wave_body(
    int ns, const float *__restrict__ s12f, const unsigned *__restrict__ start, GridParams g,
    const float4 *__restrict__ nrm, Xform64 T64, Offset64 off, float r2f, int *__restrict__ idx_out,
    float *__restrict__ d2_out, double *__restrict__ partials, unsigned long long *__restrict__ cand_count,
    const DevIcpState *__restrict__ st, int bpp, long long out_stride, const ProbDesc *__restrict__ descs,
    int nprob, const Pt64 *__restrict__ src64, const Pt64 *__restrict__ sorted64,
    const Pt64 *__restrict__ nrm64, const FoldArgs &fold, double *__restrict__ d64_out,
    Pt64 *__restrict__ prevq_io, int warm, int sweep_pass = 0)
{
    constexpr int NACC = Acc<PLANE>::N;
    const P12 *s12 = reinterpret_cast<const P12 *>(s12f);
    const WarmProblem pb = resolve_problem(descs, nprob, warm, ns, bpp, g, out_stride, [&](const ProbDesc &d) {
        src64 += d.src_off;
        s12 += d.sorted_off;
        sorted64 += d.sorted_off;
        if constexpr (PLANE) {
            if (nrm) nrm += d.sorted_off;
            if (nrm64) nrm64 += d.sorted_off;
        }
        start += d.start_off;
        idx_out += d.out_off;
        d2_out += d.out_off;
        prevq_io += d.out_off;
    });
    const int prob = pb.prob, lb = pb.lb;
    const long long row0 = pb.row0;
    ns = pb.ns; bpp = pb.bpp; g = pb.g;
    if (st) st += prob;
    {
        Xform32 T32_unused;
        if (!load_loop_state(st, T32_unused, T64, off, r2f)) return false;
    }
    const double r2d = (double)r2f;                         // (double)(float)(r*r): KDTreeFlann.cpp:184-185
    idx_out += (long long)prob * pb.out_stride;
    d2_out += (long long)prob * pb.out_stride;
    prevq_io += (long long)prob * pb.out_stride;
    double acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; a++) acc[a] = 0.0;
    unsigned ncand = 0, ncand_all = 0;

    // (inside the persistent sweep's loop: opaque, or everything derived from the thread's number is hoisted out and spilled)
    const int tid = thread_number<SWEEP, kBlock>(), lane = tid & 63, wave = tid >> 6;
    const int oct = lane >> 3, l8 = lane & 7;
    // the query -> lane map of nn_grid_reduce_kernel<G = 1> (XCD-aware chunking of the Morton order)
    int vb = lb;
    if ((bpp & 7) == 0) vb = (lb & 7) * (bpp >> 3) + (lb >> 3);
    const int total_groups = bpp * kBlock;
    const int per_group = (ns + total_groups - 1) / total_groups;
    const int gid = vb * kBlock + tid;
    const long long i_begin = (long long)gid * per_group;
    const long long i_end = i_begin + per_group < ns ? i_begin + per_group : ns;

    __shared__ float4 s_qp[kBlock];                         // (px, py, pz, W) of the query of each lane
    __shared__ uint2 s_item[kBlock / 64][kCoopCap + 64];    // chunk descriptors, completed by chunk results (+ 64 null
                                                            // descriptors behind the last one: the list is read unguarded)
    uint2 *items = s_item[wave];

    // one query (or none: the lanes past the end still work on the others' chunks)
    auto query = [&](long long i, bool active) {
        // ---- the query: the reference's transform of a source point (PointCloud.cpp:75-80), in f64
        Pt64 s8 = Pt64{0.0, 0.0, 0.0, 0ull};
        float4 qprev = make_float4(NAN, NAN, NAN, 0.f);     // the previous pass's winner (fp32 view), NaN = none
        if (active) {
            s8 = src64[i];
            if (warm & kWarmRead) {
                // (the state of grid_coop.hip: the previous winner's f64 point; all bits set = NaN = none)
                const Pt64 w8 = prevq_io[i];
                qprev = make_float4((float)w8.x, (float)w8.y, (float)w8.z, 0.f);
            }
        }
        // (se3_act: the restatement of SE3Type's action on a point, core/se3.h:103-106 -- same products, same order)
        double pd[3];
        {
            const double sv[3] = {s8.x, s8.y, s8.z};
            se3_act(T64.m, sv, pd);
        }
        const double pxd = pd[0], pyd = pd[1], pzd = pd[2];
        const float px = (float)pxd, py = (float)pyd, pz = (float)pzd;
        const WarmBand band = warm_band(px, py, pz, r2f);
        s_qp[tid] = make_float4(px, py, pz, band.W);
        // what nothing nearer than can be missed by: the previous winner's distance now, or the radius
        float bound0 = band.L;
        {
            const float dprev = sqdist_f32(qprev, px, py, pz);
            if (dprev < band.L) bound0 = dprev;              // (NaN = no previous winner: the radius)
        }
        // the slot ranges that can hold a candidate at or within bound0 (the lower bound that comes with them is the
        // certificate kernel's business: unused here)
        unsigned xb[9], xe[9], looked;
        float lbgeo2_unused;
        list_rows(start, g, px, py, pz, band.E, bound0, active, xb, xe, lbgeo2_unused, looked);
        if (cand_count) {
            // profiling only (one uniform branch): candidates listed, cell-table rows looked up
#pragma unroll
            for (int k = 0; k < 9; k++) ncand += xe[k] - xb[k];
            ncand_all += looked;
        }
        // the two best chunks (minimum, first slot, flag byte) and the third chunk minimum
        ChunkBest cb(band.L);
        // ---- the rows, chunked and flattened over the wave.  A query's chunks take CONSECUTIVE list entries: the
        // owner reads its results back as one short run (walking the rows again, one LDS round trip per chunk, took
        // 2.5 us of every wave's 17).
        {
            unsigned nq = 0;
#pragma unroll
            for (int k = 0; k < 9; k++) nq += (xe[k] - xb[k] + 7u) >> 3;
            const unsigned incl = wave_scan_incl(nq, lane);
            const unsigned M = (unsigned)__shfl((int)incl, 63, 64);
            const unsigned off_q = incl - nq;
            auto window = [&](const unsigned w0) {
                {
                    // descriptor: (the chunk's first slot, owner's query in LDS | candidates << 16); a query's chunks
                    // take CONSECUTIVE list entries, row after row
                    const unsigned own = (unsigned)tid << 4; // where this lane's query lies in s_qp
                    unsigned j = off_q - w0;                 // (a run that begins before the window wraps: never < cap)
#pragma unroll
                    for (int k = 0; k < 9; k++) {
                        unsigned b = xb[k];
                        while (b < xe[k]) {
                            if (j < (unsigned)kCoopCap) items[j] = make_uint2(b, own | (min(xe[k] - b, 8u) << 16));
                            j++;
                            b += 8u;
                        }
                    }
                }
                const unsigned Mw = min(M - w0, (unsigned)kCoopCap);
                items[Mw + lane] = make_uint2(0u, 0u);       // null descriptors (count 0) for the last, partial trip
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (unsigned t = 0; t < Mw; t += 8u * kCoopDepth) {
                    // kCoopDepth chunks per lane octet in flight: every load of the list is independent
                    P12 c4[kCoopDepth];
                    unsigned meta[kCoopDepth];
#pragma unroll
                    for (int u = 0; u < kCoopDepth; u++) {
                        const uint2 dsc = items[t + u * 8 + oct];
                        meta[u] = dsc.y;
                        // scalar base + 32-bit byte offset (the launcher keeps 12 * slots below 2^32; the array carries
                        // kSortedSlack entries of slack)
                        c4[u] = *reinterpret_cast<const P12 *>(reinterpret_cast<const char *>(s12) + (((dsc.x * 3u) << 2) + (unsigned)l8 * 12u));
                    }
#pragma unroll
                    for (int u = 0; u < kCoopDepth; u++) {
                        const unsigned cnt = meta[u] >> 16;
                        const float4 p = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(s_qp) + (meta[u] & 0xFFF0u));
                        float d = sqdist_f32(make_float4(c4[u].x, c4[u].y, c4[u].z, 0.f), p.x, p.y, p.z);
                        const bool mine = (unsigned)l8 < cnt;            // (lane 0 of the octet: the chunk exists)
                        d = mine ? d : INFINITY;
                        const float m = octet_min(d);
                        // (a lane past the chunk's end holds +inf: never within m + W of a finite minimum; a null
                        //  descriptor's result is not stored)
                        const unsigned long long bal = __builtin_amdgcn_ballot_w64(d <= m + p.w);
                        const unsigned flags = (unsigned)(bal >> (oct * 8)) & 0xFFu;
                        // the result takes the place of the descriptor's second word: the chunk minimum rounded DOWN to
                        // 16 mantissa bits | the flag byte (the first word, the chunk's position, stays)
                        if (l8 == 0 && mine) items[t + u * 8 + oct].y = (__float_as_uint(m) & 0xFFFFFF00u) | flags;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                // the owner's run of results, four reads in flight (a lane past its run inserts +inf: no effect)
                for (unsigned c0 = 0; __builtin_amdgcn_ballot_w64(c0 < nq) != 0ull; c0 += 4u) {
                    uint2 r[4];
                    bool in[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const unsigned j = off_q - w0 + c0 + (unsigned)u;
                        in[u] = c0 + (unsigned)u < nq && j < (unsigned)kCoopCap;
                        r[u] = items[in[u] ? j : 0u];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        chunk_insert(cb, in[u] ? __uint_as_float(r[u].y & 0xFFFFFF00u) : INFINITY, r[u].x, r[u].y & 0xFFu);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            };
            // (one window unless the cloud is very dense)
            for (unsigned w0 = 0; w0 < M; w0 += kCoopCap) window(w0);
        }
        // ---- the f64 decision: flagged candidates of the kept chunks inside g + W
        Best best(r2d);
        bool slow = false;                                   // needs every listed candidate ranked in f64
        // (the kept chunk minima were rounded down by < 2^-15 relative: g_up bounds the fp32 minimum from above, and
        //  the tests below stay on the safe side -- a chunk or candidate more is ranked in f64, never one less)
        const float g_up = cb.h0 * (1.0f + 6.2e-5f);
        if (active && cb.b0 != 0xFFFFFFFFu) {
            const float thr = g_up + band.W;
            unsigned c[4] = {0u, 0u, 0u, 0u};
            int n = 0;
            slow = cb.h2 <= thr;                             // a third chunk reaches into the band
            add_flagged(cb.b0, cb.m0, c, n, slow);
            if (cb.h1 <= thr) add_flagged(cb.b1, cb.m1, c, n, slow);
            rank_flagged(best, sorted64, c, n, pxd, pyd, pzd);
        }
        // ---- the re-scan (rescan_wave), over the slot ranges this lane listed and still holds
        for (unsigned long long rem = __builtin_amdgcn_ballot_w64(slow); rem; rem &= rem - 1ull) {
            const int q = (int)__builtin_ctzll(rem);         // wave-uniform
            const WaveQuery wq = broadcast_query(q, px, py, pz, pxd, pyd, pzd, band.rup, band.E, g_up);
            unsigned qb[9], pre[10];
            broadcast_ranges(q, xb, xe, qb, pre);
            rescan_wave(best, q, lane, qb, pre, wq, r2d, s12, sorted64);
        }
        if (active) {
            idx_out[i] = (best.pos == 0xFFFFFFFFu) ? -1 : (int)best.idx;
            d2_out[i] = (float)best.d;
            // the winner as the candidate array holds it (fp32 rounding of the same f64 value): next pass's bound
            {
                // the state for the next pass: the winner's f64 point and index, LB = 0 (no certificate can follow from it)
                Pt64 o8;
                o8.x = o8.y = o8.z = __longlong_as_double(-1ll);
                o8.w = 0xFFFFFFFFull;
                if (best.pos != 0xFFFFFFFFu) { o8.x = best.q.x; o8.y = best.q.y; o8.z = best.q.z; o8.w = (unsigned long long)best.idx; }
                prevq_io[i] = o8;
            }
            if (d64_out) d64_out[i] = best.d;                    // (target-sharded ranks compare shards in f64)
            if (best.pos != 0xFFFFFFFFu) {
                double nx = 0.0, ny = 0.0, nz = 0.0;
                if (PLANE) {
                    if (nrm64) { const Pt64 n8 = nrm64[(unsigned)best.q.w]; nx = n8.x; ny = n8.y; nz = n8.z; }
                    else { const float4 n4 = nrm[(unsigned)best.q.w]; nx = n4.x; ny = n4.y; nz = n4.z; }
                }
                accumulate_pq_d<PLANE>(acc, pxd, pyd, pzd, best.q.x, best.q.y, best.q.z, nx, ny, nz, off);
            }
        }
    };
    if constexpr (ONE) {
        query(i_begin, i_begin < i_end);
    } else {
        for (int it = 0; it < per_group; it++) query(i_begin + it, i_begin + it < i_end);   // wave-uniform trip count
    }
    block_reduce_store<NACC, kBlock / 64, SWEEP>(acc, partials, SWEEP || fold.tickets != nullptr);   // (rows read by another workgroup: past the L2)
    if (cand_count) {
        unsigned long long c = ncand, ca = ncand_all;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c += __shfl_down(c, o, 64);
            ca += __shfl_down(ca, o, 64);
        }
        if (lane == 0 && ca) {
            unsigned long long *slot = cand_count + 2 * (blockIdx.x & 4095);
            atomicAdd(slot, c);
            atomicAdd(slot + 1, ca);
        }
    }
    bool published = false;
    if constexpr (SWEEP) {
        // (the persistent sweep launch: fold, closed-form update, compose, stop test and the hand-over of the next transform
        //  by the workgroup that completes the problem's fold)
        // (the fold's arguments are read from the kernarg segment HERE, not carried across the search)
        typedef const SweepParams __attribute__((address_space(4))) *KernargPtr;
        KernargPtr kp = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        FoldArgs f{};
        f.tickets = ld_karg(&kp->fold.tickets); f.partials2 = ld_karg(&kp->fold.partials2);
        f.ticket_stride = ld_karg(&kp->fold.ticket_stride); f.stats_out = ld_karg(&kp->fold.stats_out);
        f.stats_stride = ld_karg(&kp->fold.stats_stride);
        f.solve = ld_karg(&kp->st);
        f.sweep_relay = ld_karg(&kp->sa.relay);
        f.sweep_tag = ld_karg(&kp->sa.tag0) + (unsigned)sweep_pass + 1u;
        f.sweep_passes = ld_karg(&kp->sa.passes0) + sweep_pass;
        published = fused_fold<PLANE, kBlock, true, true>(f, ld_karg(&kp->partials), row0, lb, bpp, prob);
    } else {
        if (fold.tickets) published = fused_fold<PLANE, kBlock, false, kSolveInFold>(fold, partials, row0, lb, bpp, prob);
    }
    return published;
}

#define VISMA_WAVE_PARAMS                                                                                         \
    int ns, const float *__restrict__ s12f, const unsigned *__restrict__ start, GridParams g,                    \
        const float4 *__restrict__ nrm, Xform64 T64, Offset64 off, float r2f, int *__restrict__ idx_out,         \
        float *__restrict__ d2_out, double *__restrict__ partials, unsigned long long *__restrict__ cand_count,  \
        const DevIcpState *__restrict__ st, int bpp, long long out_stride, const ProbDesc *__restrict__ descs,   \
        int nprob, const Pt64 *__restrict__ src64, const Pt64 *__restrict__ sorted64,                            \
        const Pt64 *__restrict__ nrm64, const FoldArgs fold, double *__restrict__ d64_out,                       \
        Pt64 *__restrict__ prevq_io, int warm
#define VISMA_WAVE_ARGS                                                                                          \
    ns, s12f, start, g, nrm, T64, off, r2f, idx_out, d2_out, partials, cand_count, st, bpp, out_stride, descs,   \
        nprob, src64, sorted64, nrm64, fold, d64_out, prevq_io, warm
// One query per lane: C4's 262,144 queries are 4096 waves, all resident at once only at 4 waves per SIMD
// (<= 128 VGPRs; the kernel needs 104).  Several queries per lane: the 23 / 29 f64 moments stay live across
// the queries, so the compiler gets the registers it asks for (2 waves per SIMD; such launches have more
// waves than the chip holds anyway).
#ifndef VISMA_WAVE_WAVES
#define VISMA_WAVE_WAVES 4
#endif
template <bool PLANE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(VISMA_WAVE_WAVES, VISMA_WAVE_WAVES))) void nn_wave_kernel_one(VISMA_WAVE_PARAMS)
{
    wave_body<PLANE, true>(VISMA_WAVE_ARGS);
}
template <bool PLANE>
__global__ __launch_bounds__(kBlock) void nn_wave_kernel_many(VISMA_WAVE_PARAMS)
{
    wave_body<PLANE, false>(VISMA_WAVE_ARGS);
}
#undef VISMA_WAVE_PARAMS
#undef VISMA_WAVE_ARGS

// ---- The PERSISTENT SWEEP launch (round 6): the warm passes of nprob registrations over SHARED clouds -- the 24 yaw starts of
// feh::RegisterModelToScene (src/annotation.cpp:35-61), a device-resident loop of one problem -- inside ONE launch.  Until now
// every pass was a search launch plus a one-thread solve launch (5 k -> 20 k, 24 starts: 27 us per pass for 20 us of kernels).
// Here a workgroup runs its problem's passes back to back: search and block reduction as in nn_wave_kernel_one, the ticket
// fold of its problem, and the workgroup that completes the fold advances the problem's state (advance_state: the code of
// solve_state_kernel) and hands the next transform to the problem's other workgroups through 25 self-validating words in
// device memory (kernels.h: FoldArgs::sweep_relay) -- nobody fences, every wait is bounded by the wall clock.  Problems
// advance independently; a problem that stops frees its workgroups.  Same results as one launch per pass, bit for bit (same
// search, same fold order, same solve).  Needs every workgroup resident (the launcher's caller checks the capacity); a wait
// that runs out sets *dead and everybody leaves: the states hold what was completed, the host carries on with launches.
template <bool PLANE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void nn_wave_kernel_sweep(const SweepParams P)
{
    // the transform of the pass that is due: 32-bit halves of its 12 doubles + the command word, in LDS
    __shared__ unsigned s_w[32];
    const int prob = (int)blockIdx.x / P.bpp;
    {
        // pass 0: the state as the launches before this one left it
        const DevIcpState *sp = P.st + prob;
        if (!sp->active) return;
        if (threadIdx.x < 12) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(sp->Tc[threadIdx.x]);
            s_w[2 * threadIdx.x] = (unsigned)b;
            s_w[2 * threadIdx.x + 1] = (unsigned)(b >> 32);
        }
    }
    __syncthreads();
    typedef const SweepParams __attribute__((address_space(4))) *KernargPtr;
    for (int pass = 0;; pass++) {
        KernargPtr kp = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));                         // (nothing read through it is loop-invariant to the compiler)
#define VISMA_KARG(F_) ld_karg(&kp->F_)
        Xform64 T64;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)s_w[2 * k]);
            const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)s_w[2 * k + 1]);
            T64.m[k] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
        DevIcpState *st = VISMA_KARG(st);
        const int bpp = VISMA_KARG(bpp);
        const int pr = (int)blockIdx.x / bpp;
        Offset64 off;
        {
            const DevIcpState *sp = st + pr;                 // (constants of the loop: never written after its start)
#pragma unroll
            for (int a = 0; a < 3; a++) off.v[a] = sp->world_frame ? sp->centre[a] : 0.0;
        }
        const FoldArgs nofold{};                             // (wave_body reads the fold's arguments itself: SWEEP)
        (void)wave_body<PLANE, true, true>(VISMA_KARG(ns), VISMA_KARG(s12f), VISMA_KARG(start), VISMA_KARG(g), nullptr, T64, off,
                                           VISMA_KARG(r2f), VISMA_KARG(idx_out), VISMA_KARG(d2_out), VISMA_KARG(partials),
                                           VISMA_KARG(cand_count), nullptr, bpp, VISMA_KARG(out_stride), nullptr, VISMA_KARG(nprob),
                                           VISMA_KARG(src64), VISMA_KARG(sorted64), nullptr, nofold, nullptr, VISMA_KARG(prevq_io), 1,
                                           pass);
        kp = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const SweepArgs sa = VISMA_KARG(sa);
#undef VISMA_KARG
        if (pass + 1 >= sa.max_passes) break;
        // ---- the problem's next transform: the first wave polls the problem's 25 words for the tag of the pass that is due
        __syncthreads();                                     // (everybody has read s_w)
        if (threadIdx.x < 64) {
            const int lane = (int)threadIdx.x;
            const unsigned tag = sa.tag0 + (unsigned)pass + 1u;
            unsigned long long w = 0ull;
            const long long t0 = (long long)wall_clock64();
            const int pr2 = (int)blockIdx.x / ld_karg(&kp->bpp);
            for (;;) {
                if (lane < kPersistWords) w = __hip_atomic_load(sa.relay + 32ll * pr2 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool ok = lane >= kPersistWords || (unsigned)(w >> 32) == tag;
                if (__builtin_amdgcn_ballot_w64(ok) == ~0ull) break;
                const bool dead = __hip_atomic_load(sa.dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull;
                if (dead || (long long)wall_clock64() - t0 > sa.wait_ticks) {
                    // (somebody's workgroups are not running, or left: no fold of this launch can complete any more)
                    if (lane == 0) __hip_atomic_store(sa.dead, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    w = (unsigned long long)kPersistAbort;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (lane < 32) s_w[lane] = (unsigned)w;
        }
        __syncthreads();
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)s_w[kPersistWords - 1]) != kPersistGo) break;
    }
}

int nn_wave_sweep_capacity()
{
    static int cap[64];
    static bool known[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 0; }
    if (!known[dev]) {
        int per_cu = 0, cus = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, nn_wave_kernel_sweep<false>, kBlock, 0);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) { (void)hipGetLastError(); per_cu = 0; cus = 0; }
        cap[dev] = per_cu * cus;
        known[dev] = true;
    }
    return cap[dev];
}

hipError_t launch_nn_wave_sweep(const SearchArgs &a, const SweepArgs &sa, hipStream_t stream)
{
    const int bpp = search_blocks(a.ns, kCoopLanes, a.max_blocks);
    if (!a.src64 || !a.sorted64 || !a.sorted12 || !a.wst_io || !a.st || !a.fold.tickets || !sa.relay || !sa.dead || sa.max_passes < 1 ||
        a.nprob < 1 || (long long)bpp * kBlock < a.ns || bpp * a.nprob > nn_wave_sweep_capacity())
        return hipErrorInvalidValue;
    SweepParams P{};
    P.ns = (int)a.ns; P.s12f = a.sorted12; P.start = a.start; P.g = a.g; P.r2f = a.r2f; P.idx_out = a.idx_out; P.d2_out = a.d2_out;
    P.partials = a.partials; P.cand_count = a.cand_count; P.st = a.st; P.bpp = bpp; P.out_stride = (long long)a.out_stride;
    P.nprob = a.nprob; P.src64 = a.src64; P.sorted64 = a.sorted64; P.fold = a.fold; P.prevq_io = a.wst_io; P.sa = sa;
    hipLaunchKernelGGL(nn_wave_kernel_sweep<false>, dim3(bpp * a.nprob), dim3(kBlock), 0, stream, P);
    return hipGetLastError();
}

#define VISMA_WAVE_LAUNCH(KERNEL_)                                                                                  \
    hipLaunchKernelGGL(KERNEL_, dim3(geo.total_blocks), dim3(kBlock), 0, stream, (int)a.ns, a.sorted12, a.start, a.g, \
                       a.nrm, a.T64, a.off, a.r2f, a.idx_out, a.d2_out, a.partials, a.cand_count, a.st, geo.bpp,     \
                       (long long)a.out_stride, a.descs, a.nprob, a.src64, a.sorted64, a.nrm64, a.fold, a.d64_out,   \
                       a.wst_io, warm)

// The warm-started, flattened exact search of round 3 (what launch_nn_coop hands batches and sweeps): same arguments,
// no Tprev and no runner-up state; wst_io holds the winners as points of the candidate array.
hipError_t launch_nn_wave(const SearchArgs &a, const SearchGeom &geo, hipStream_t stream)
{
    if (!a.src64 || !a.sorted64 || !a.sorted12 || !a.wst_io) return hipErrorInvalidValue;
    const int warm = a.warm & (kWarmRead | kWarmMap | kWarmNoCert);
    if (a.point_to_plane) {
        if (geo.one) VISMA_WAVE_LAUNCH(nn_wave_kernel_one<true>); else VISMA_WAVE_LAUNCH(nn_wave_kernel_many<true>);
    } else {
        if (geo.one) VISMA_WAVE_LAUNCH(nn_wave_kernel_one<false>); else VISMA_WAVE_LAUNCH(nn_wave_kernel_many<false>);
    }
    return hipGetLastError();
}
#undef VISMA_WAVE_LAUNCH

}  // namespace visma
