// warm_search.h -- what the two warm-pass search kernels share: grid_coop.hip (the certificate kernel: single
// registrations) and grid_wave.hip (the wave-owned kernel: batches and sweeps).  One statement each of the "which problem
// am I" prologue, the rounding band of a query, the listing of its rows' slot ranges, the bookkeeping of its best chunks,
// the f64 ranking and the whole-wave f64 re-scan.  Inlined device functions and small structs only; what differs between
// the kernels (certificate, queue, list windows, chunk work-off loops, the loops around a pass) stays in their files.
//
// Exactness without per-candidate top-2 bookkeeping: the eight lanes of a chunk reduce
// their fp32 d2 to the chunk minimum m (three DPP steps) and flag every candidate with d2 <= m + W, W an
// upper bound of band(m) - m for any m inside the radius (band(m) = (sqrt(m) + 2E)^2, E the rounding
// half-width of exact_band()).  The query keeps its two best CHUNKS (m, first slot, flag byte) and the
// third chunk minimum.  Any candidate within the rounding band of the global fp32 minimum g lies in a
// chunk with m <= g + W and is flagged there (d2 <= band(g) <= band(m) <= m + W), so ranking the flagged
// candidates of the kept chunks with m <= g + W in f64 (reference arithmetic, lowest original index on
// exact ties, strict d2 < (double)(float)r2) returns the reference's correspondence; a third chunk inside
// g + W, or more than four flagged candidates, sends the query to the f64 re-scan of its 27 cells (points
// given several times).
#pragma once

#include "device_common.h"

namespace visma {

// minimum over the 8 lanes of an aligned lane octet: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror.
// (v_min_f32_dpp reads its first source through the permutation; a VALU result needs two wait states
// before a DPP read, which the compiler does not insert inside an asm block.)  A NaN d (a candidate that is not finite) is
// skipped: v_min_f32 returns its other operand; an octet of nothing but NaN gives NaN, which no comparison after it
// accepts (tests/test_core_hostile.py).
__device__ __forceinline__ float octet_min(float d)
{
    float r;
    asm volatile("s_nop 1\n\t"
                 "v_min_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf"
                 : "=&v"(r)
                 : "v"(d));
    return r;
}

// inclusive prefix sum over the 64 lanes: DPP row shifts inside the 16-lane rows (absent lanes read 0), then the
// last lane of row 0 / 2 broadcast into row 1 / 3 and lane 31 into the upper half -- no LDS round trips
__device__ __forceinline__ unsigned wave_scan_incl(unsigned v, int)
{
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}

// a (member of a) kernel argument read through the laundered kernarg pointer, word by word: the persistent kernels read
// their arguments at the top of EVERY pass through a pointer the compiler cannot see through (with ordinary arguments
// the loop around the pass had every invariant of the body hoisted out of it and spilled)
template <class T>
__device__ __forceinline__ T ld_karg(const T __attribute__((address_space(4))) *p)
{
    static_assert(sizeof(T) % 4 == 0, "words");
    constexpr int N = (int)(sizeof(T) / 4);
    union U { T v; unsigned w[N]; __device__ U() {} } u;
    typedef const unsigned __attribute__((address_space(4))) *WordPtr;
    const WordPtr pw = (WordPtr)p;
#pragma unroll
    for (int k = 0; k < N; k++) u.w[k] = pw[k];
    return u.v;
}

// ---- Which problem a workgroup belongs to, and where that problem's arrays begin.  Shared clouds (descs == NULL):
// problem blockIdx.x / bpp, every problem `out_stride` elements further in the out arrays.  A batch of problems with their
// own clouds: the descriptor's shape and grid, out_stride = 0, and `apply_offsets(d)` for the kernel to move ITS pointers
// by the descriptor's element offsets (source: src_off; candidate arrays and normals: sorted_off; cell table: start_off;
// outputs and state: out_off).  (Inside the branch, not as offsets handed back: offsets that are zero on the other path
// stay live as scalar registers beside the pointers, and the one-pass certificate kernels spilled 12 of them.)
struct WarmProblem {
    int prob, lb, bpp, ns;
    long long row0;                                          // the problem's first partial row
    GridParams g;
    long long out_stride;
};
template <class ApplyOffsets>
__device__ __forceinline__ WarmProblem resolve_problem(const ProbDesc *__restrict__ descs, int nprob, int warm, int ns, int bpp,
                                                       const GridParams &g, long long out_stride, ApplyOffsets apply_offsets)
{
    WarmProblem p;
    if (descs) {
        // (largest p with first_block <= blockIdx.x; wave-uniform)
        if (warm & kWarmMap) {
            // (the launcher put a workgroup -> problem map behind the descriptors)
            p.prob = reinterpret_cast<const int *>(descs + nprob)[blockIdx.x];
        } else {
            int lo = 0, hi = nprob - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (descs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
            }
            p.prob = lo;
        }
        const ProbDesc d = descs[p.prob];
        p.lb = (int)blockIdx.x - d.first_block;
        p.bpp = d.nblocks;
        p.ns = d.ns;
        p.row0 = d.first_block;
        p.g = d.g;
        p.out_stride = 0;
        apply_offsets(d);
    } else {
        p.prob = blockIdx.x / bpp;
        p.lb = blockIdx.x - p.prob * bpp;
        p.bpp = bpp;
        p.ns = ns;
        p.row0 = (long long)p.prob * bpp;
        p.g = g;
        p.out_stride = out_stride;
    }
    return p;
}

// ---- The rounding band of the query at (px, py, pz) (exact_band): E bounds |d64 - sqrt(d2_32)|; L = the
// squared fp32 distance at or beyond which a candidate cannot be accepted in f64; W >= band(m) - m for every m < L
struct WarmBand { float rup, E, tlim, L, W; };
__device__ __forceinline__ WarmBand warm_band(float px, float py, float pz, float r2f)
{
    WarmBand b;
    b.rup = band_round_up(sqrtf(r2f));
    b.E = exact_band_at(px, py, pz, b.rup);
    b.tlim = b.rup + 2.0f * b.E;
    b.L = exact_band_square(b.rup, b.E);
    b.W = (4.0f * b.E * b.tlim + 4.0f * b.E * b.E) * (1.0f + 1e-6f) + b.L * 5e-7f;
    return b;
}

// ---- The slot ranges of the query at (px, py, pz) that can hold a candidate at or within the squared fp32 distance
// bound0: xb[k] .. xe[k] of row k = (dy, dz) of the 3 x 3 x 3 cells around it, and lbgeo2, a lower bound (squared) of
// the distance to every target point that lies in NONE of those ranges.  `want`: this lane looks its rows up at all.
// `looked`: cell-table rows looked up (profiling).
__device__ __forceinline__ void list_rows(const unsigned *__restrict__ start, const GridParams &g, const float px, const float py,
                                          const float pz, const float E, const float bound0, const bool want, unsigned (&xb)[9],
                                          unsigned (&xe)[9], float &lbgeo2, unsigned &looked)
{
    const int cx = cell_coord(px, g.mn[0], g.inv_h, g.dim[0]);
    const int cy = cell_coord(py, g.mn[1], g.inv_hs, g.dim[1]);
    const int cz = cell_coord(pz, g.mn[2], g.inv_hs, g.dim[2]);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
    const int span = x1 + 1 - x0;                            // cells of a row that exist: <= 0, 1, 2 or 3
    // ---- starts of the cells x0 .. x0+3 of a row: one 16-byte load (absent row / lane: zeros = empty)
    typedef unsigned u4a __attribute__((ext_vector_type(4), aligned(4)));
    // (cell indices fit 32 bits: kGridMaxCells; which of the three y / z rows exist is tested once per axis)
    const bool yok[3] = {cy - 1 >= 0 && cy - 1 < g.dim[1], cy >= 0 && cy < g.dim[1], cy + 1 >= 0 && cy + 1 < g.dim[1]};
    const bool zok[3] = {cz - 1 >= 0 && cz - 1 < g.dim[2], cz >= 0 && cz < g.dim[2], cz + 1 >= 0 && cz + 1 < g.dim[2]};
    const int row_c = (cz * g.dim[1] + cy) * g.dim[0] + x0, pitch_y = g.dim[0], pitch_z = g.dim[1] * g.dim[0];
    auto load_row = [&](int k, bool wanted) {
        const bool ok = wanted && span > 0 && zok[k / 3] && yok[k % 3];
        u4a v = {0u, 0u, 0u, 0u};
        if (ok) v = *reinterpret_cast<const u4a *>(reinterpret_cast<const char *>(start) + (unsigned)(row_c + (k / 3 - 1) * pitch_z + (k % 3 - 1) * pitch_y) * 4u);
        return v;
    };
    // slab distances (in cells) of the neighbouring rows / cells, margins as in nn_grid_reduce_kernel
    const float fx = (px - g.mn[0]) * g.inv_h - (float)cx;
    const float fy = (py - g.mn[1]) * g.inv_hs - (float)cy;
    const float fz = (pz - g.mn[2]) * g.inv_hs - (float)cz;
    const float mgn = 1e-3f + 4.0f * E * g.inv_hs;
    const float lo_x = fmaxf(fx - mgn, 0.f), hi_x = fmaxf(1.0f - fx - mgn, 0.f);
    const float lo_y = fmaxf(fy - mgn, 0.f), hi_y = fmaxf(1.0f - fy - mgn, 0.f);
    const float lo_z = fmaxf(fz - mgn, 0.f), hi_z = fmaxf(1.0f - fz - mgn, 0.f);
    const float h2 = slab_h2(g.hs);
    // LB, geometric part: what everything outside the 27 cells is at least away (squared): one cell plus the
    // nearest face of the own cell; a query far outside the grid's bounding box (clamped cell coordinate): its
    // distance to the box, in cells (same fp32 binning, same margin).  The cells NOT listed: pruned2 below.
    float out2;
    {
        const float face = fminf(fminf(fminf(lo_x, hi_x), fminf(lo_y, hi_y)), fminf(lo_z, hi_z));
        const float ux = fx + (float)cx, uy = fy + (float)cy, uz = fz + (float)cz;
        const float far = fmaxf(fmaxf(fmaxf(-ux, ux - (float)g.dim[0]), fmaxf(-uy, uy - (float)g.dim[1])),
                                fmaxf(-uz, uz - (float)g.dim[2])) - 2.0f * mgn;
        const float outc = fmaxf(1.0f + face, far);
        out2 = outc * outc * h2;
    }
    float exq[3];                                            // (a cell past the span: +inf -- never listed, bounds nothing)
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int xi = x0 + j;
        const float ex = xi == cx ? 0.f : (xi < cx ? lo_x + (float)(cx - xi - 1) : hi_x + (float)(xi - cx - 1));
        exq[j] = j < span ? ex * ex * h2 : INFINITY;
    }
    const float ey2[3] = {lo_y * lo_y, 0.f, hi_y * hi_y}, ez2[3] = {lo_z * lo_z, 0.f, hi_z * hi_z};
    float rowB[9];                                           // squared slab bound of row k = (dy, dz); a row that does not exist: +inf
#pragma unroll
    for (int k = 0; k < 9; k++) rowB[k] = (zok[k / 3] && yok[k % 3]) ? (ey2[k % 3] + ez2[k / 3]) * h2 : INFINITY;
    // ---- only the rows whose slab can hold a point at or within bound0 are looked up at all (a converged
    // pass needs 1.9 of the 9 per query), all of them in ONE round of gathers: nothing depends on a load
    // from here to the candidates
    u4a cs[9];
    looked = 0u;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const bool w = want && !(rowB[k] > bound0);
        cs[k] = load_row(k, w);
        looked += (w && span > 0) ? 1u : 0u;
    }
    // ---- the slots of each row that can hold a candidate at or within bound0: cells whose slab bound
    // (y, z and x slab distances, squared) does not exceed it.  A skipped cell holds nothing that could
    // win or tie (margins: fp32 binning + rounding band, as in the lane-serial kernel).
    // (B + exq[j] <= bound0 tested as B <= bound0 - exq[j]: the slab bounds carry a relative margin of ~1e-3, a
    //  rounding of the subtraction cannot drop a cell that matters; a cell that does not exist: -inf)
    const float lim0 = bound0 - exq[0];                      // (-inf for a cell past the span)
    const float lim1 = bound0 - exq[1];
    const float lim2 = bound0 - exq[2];
    float pruned2 = INFINITY;                                // smallest slab bound (squared) among the cells NOT listed
    const float thr0 = bound0 * (1.0f - 1e-6f);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const float B = rowB[k];
        const bool n0 = B <= lim0, n1 = B <= lim1, n2 = B <= lim2;
        // (a cell is NOT listed iff B > fl(bound0 - exq[j]), which implies fl(B + exq[j]) > bound0 (1 - 2e-7): every
        //  such cell is in this minimum; a listed cell within 1e-6 of bound0 may be too -- its slab bound holds as well.
        //  Own comparisons, so that the 27 listing masks need not stay live)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float S = B + exq[j];
            pruned2 = fminf(pruned2, S >= thr0 ? S : INFINITY);
        }
        const u4a v = cs[k];                                 // (a row not looked up reads as zeros: empty)
        const unsigned b = n0 ? v.x : (n1 ? v.y : v.z);
        unsigned e = n2 ? v.w : (n1 ? v.z : (n0 ? v.y : b));
        if (!(n0 || n1 || n2)) e = b;
        xb[k] = b;
        xe[k] = e;
    }
    lbgeo2 = fminf(out2, pruned2);
}

// ---- What a query keeps of its chunks: the two best (minimum, first slot, flag byte), the third chunk minimum, and the
// best chunk's side word (the certificate kernel's runner-up builds only)
struct ChunkBest {
    float h0, h1, h2;
    unsigned b0, b1, m0, m1, s0;
    __device__ explicit ChunkBest(float none, unsigned side_none = 0u)
        : h0(none), h1(none), h2(none), b0(0xFFFFFFFFu), b1(0xFFFFFFFFu), m0(0u), m1(0u), s0(side_none) {}
};
__device__ __forceinline__ void chunk_insert(ChunkBest &c, float m, unsigned b, unsigned flags)
{
    const bool c1 = m < c.h0, c2 = m < c.h1;
    c.h2 = __builtin_amdgcn_fmed3f(c.h1, c.h2, m);
    c.h1 = __builtin_amdgcn_fmed3f(c.h0, c.h1, m);
    c.h0 = fminf(c.h0, m);
    c.b1 = c2 ? b : c.b1; c.m1 = c2 ? flags : c.m1;
    c.b1 = c1 ? c.b0 : c.b1; c.m1 = c1 ? c.m0 : c.m1;
    c.b0 = c1 ? b : c.b0; c.m0 = c1 ? flags : c.m0;
}
// (... with the chunk's side word, kept for the best chunk.  An overload, not a defaulted argument: the update of a word
//  nobody reads, removed as dead code, still cost the persistent kernel a spilled scalar register)
__device__ __forceinline__ void chunk_insert(ChunkBest &c, float m, unsigned b, unsigned flags, unsigned side)
{
    const bool c1 = m < c.h0;
    chunk_insert(c, m, b, flags);
    c.s0 = c1 ? side : c.s0;
}

// ---- The f64 decision.  Best: the best candidate so far -- d strictly below r2d once set, its original index, its slot
// in the cell-sorted arrays (~0: none) and its f64 point.
struct Best {
    double d;
    unsigned idx, pos;
    Pt64 q;
    __device__ explicit Best(double r2d) : d(r2d), idx(0xFFFFFFFFu), pos(0xFFFFFFFFu), q(Pt64{0.0, 0.0, 0.0, 0ull}) {}
};
// one candidate against the best so far: the reference's arithmetic, lowest original index on an exact tie
__device__ __forceinline__ void rank_f64(Best &best, const Pt64 &c8, unsigned pos, double pxd, double pyd, double pzd)
{
    // flann L2 (dist.h:159-176): result += diff * diff over x, y, z
    const double dx = c8.x - pxd, dy = c8.y - pyd, dz = c8.z - pzd;
    double d = dx * dx;
    d += dy * dy;
    d += dz * dz;
    const unsigned id = (unsigned)c8.w;
    const bool lt = d < best.d || (d == best.d && id < best.idx && best.idx != 0xFFFFFFFFu);
    best.d = lt ? d : best.d;
    best.idx = lt ? id : best.idx;
    best.pos = lt ? pos : best.pos;
    best.q.x = lt ? c8.x : best.q.x; best.q.y = lt ? c8.y : best.q.y; best.q.z = lt ? c8.z : best.q.z; best.q.w = lt ? c8.w : best.q.w;
}
// the flagged candidates of the chunk that begins at slot b: up to four slots in c[], n counts them all; a fifth sets slow
__device__ __forceinline__ void add_flagged(unsigned b, unsigned flags, unsigned (&c)[4], int &n, bool &slow)
{
    while (flags) {
        const unsigned pos = b + (unsigned)__builtin_ctz(flags);
        flags &= flags - 1u;
        if (n == 0) c[0] = pos; else if (n == 1) c[1] = pos; else if (n == 2) c[2] = pos; else if (n == 3) c[3] = pos;
        else slow = true;
        n++;
    }
}
// ... ranked in f64 (a second flagged candidate: one query in a thousand; a third: duplicated points)
__device__ __forceinline__ void rank_flagged(Best &best, const Pt64 *__restrict__ sorted64, const unsigned (&c)[4], int n, double pxd,
                                             double pyd, double pzd)
{
    Pt64 c8a = Pt64{0.0, 0.0, 0.0, 0ull}, c8b = c8a;
    if (n > 0) c8a = sorted64[c[0]];
    if (n > 1) c8b = sorted64[c[1]];
    if (n > 0) rank_f64(best, c8a, c[0], pxd, pyd, pzd);
    if (n > 1) rank_f64(best, c8b, c[1], pxd, pyd, pzd);
    if (n > 2) rank_f64(best, sorted64[c[2]], c[2], pxd, pyd, pzd);
    if (n > 3) rank_f64(best, sorted64[c[3]], c[3], pxd, pyd, pzd);
}

// ---- The re-scan of a query that the chunk bookkeeping cannot decide (a third chunk inside the band, more than four
// flagged candidates: points given several times), by the WHOLE WAVE for one such query at a time (a few per launch at
// C4, and the launch lasts as long as its slowest wave: one lane walking its 27 cells alone -- ~90 dependent loads -- put
// 6 us on the tail of every launch).  The query's listed slot ranges (everything that can win or tie lies in them, see
// list_rows) are flattened over the lanes: one fp32 filter load, one f64 load, a butterfly over (d2, original index), the
// winner's coordinates handed to the owner lane.
// the value lane q holds (q wave-uniform)
__device__ __forceinline__ unsigned bcast_u(unsigned v, int q) { return (unsigned)__builtin_amdgcn_readlane((int)v, q); }
__device__ __forceinline__ float bcast_f(float v, int q) { return __uint_as_float(bcast_u(__float_as_uint(v), q)); }
__device__ __forceinline__ unsigned long long bcast_u64(unsigned long long u, int q)
{
    return ((unsigned long long)bcast_u((unsigned)(u >> 32), q) << 32) | bcast_u((unsigned)u, q);
}
__device__ __forceinline__ double bcast_d(double v, int q)
{
    return __longlong_as_double((long long)bcast_u64((unsigned long long)__double_as_longlong(v), q));
}
// the query of lane q on every lane: its fp32 and f64 point, and Ls, the squared fp32 distance beyond which nothing can
// win or tie in f64 against its fp32 minimum (g_up bounds that minimum from above)
struct WaveQuery {
    float x, y, z, Ls;
    double xd, yd, zd;
};
__device__ __forceinline__ WaveQuery broadcast_query(int q, float px, float py, float pz, double pxd, double pyd, double pzd, float rup,
                                                     float E, float g_up)
{
    WaveQuery w;
    w.x = bcast_f(px, q); w.y = bcast_f(py, q); w.z = bcast_f(pz, q);
    w.xd = bcast_d(pxd, q); w.yd = bcast_d(pyd, q); w.zd = bcast_d(pzd, q);
    w.Ls = exact_band_limit_from(bcast_f(E, q), rup, bcast_f(g_up, q));
    return w;
}
// lane q's nine slot ranges on every lane: where each begins, and the running count of their slots
__device__ __forceinline__ void broadcast_ranges(int q, const unsigned (&xb)[9], const unsigned (&xe)[9], unsigned (&qb)[9],
                                                 unsigned (&pre)[10])
{
    pre[0] = 0u;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        qb[k] = bcast_u(xb[k], q);
        pre[k + 1] = pre[k] + (bcast_u(xe[k], q) - qb[k]);
    }
}
// every slot of the nine ranges ranked in f64 by the wave; lane q's `best` takes the winner if it beats what the lane has
__device__ __forceinline__ void rescan_wave(Best &best, int q, int lane, const unsigned (&qb)[9], const unsigned (&pre)[10],
                                            const WaveQuery &w, double r2d, const P12 *__restrict__ s12,
                                            const Pt64 *__restrict__ sorted64)
{
    double ld = r2d;
    unsigned lid = 0xFFFFFFFFu, lpos = 0xFFFFFFFFu;
    Pt64 lq = Pt64{0.0, 0.0, 0.0, 0ull};
    for (unsigned f0 = 0; f0 < pre[9]; f0 += 128u) {          // (one trip unless the rows are very dense)
        unsigned j[2];
        bool in[2];
        P12 t[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const unsigned f = f0 + (unsigned)u * 64u + (unsigned)lane;
            in[u] = f < pre[9];
            unsigned jj = 0u;
#pragma unroll
            for (int k = 0; k < 9; k++)
                if (f >= pre[k] && f < pre[k + 1]) jj = qb[k] + (f - pre[k]);
            j[u] = jj;
            t[u] = P12{0.f, 0.f, 0.f};
            if (in[u]) t[u] = s12[jj];
        }
        Pt64 c8[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            in[u] = in[u] && sqdist_f32(make_float4(t[u].x, t[u].y, t[u].z, 0.f), w.x, w.y, w.z) <= w.Ls;
            c8[u] = Pt64{0.0, 0.0, 0.0, 0ull};
            if (in[u]) c8[u] = sorted64[j[u]];
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
            if (in[u]) {
                // flann L2 (dist.h:159-176), as rank_f64
                const double dx = c8[u].x - w.xd, dy = c8[u].y - w.yd, dz = c8[u].z - w.zd;
                double d = dx * dx;
                d += dy * dy;
                d += dz * dz;
                const unsigned id = (unsigned)c8[u].w;
                const bool lt = d < ld || (d == ld && id < lid && lid != 0xFFFFFFFFu);
                if (lt) { ld = d; lid = id; lpos = j[u]; lq = c8[u]; }
            }
    }
    // minimum over the lanes by (d2, original index); lanes without a candidate hold (r2d, none)
    double rd = ld;
    unsigned rid = lid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(rd, o, 64);
        const unsigned oid = (unsigned)__shfl_xor((int)rid, o, 64);
        const bool lt = oid != 0xFFFFFFFFu && (od < rd || (od == rd && oid < rid));
        rd = lt ? od : rd;
        rid = lt ? oid : rid;
    }
    if (rid != 0xFFFFFFFFu) {                                // (wave-uniform)
        const unsigned long long holders = __builtin_amdgcn_ballot_w64(lid == rid && ld == rd);
        const int wl = (int)__builtin_ctzll(holders);
        Pt64 w8;
        w8.x = bcast_d(lq.x, wl);
        w8.y = bcast_d(lq.y, wl);
        w8.z = bcast_d(lq.z, wl);
        w8.w = bcast_u64(lq.w, wl);
        const unsigned wpos = bcast_u(lpos, wl);
        if (lane == q) {
            const bool lt = rd < best.d || (rd == best.d && rid < best.idx && best.idx != 0xFFFFFFFFu);
            if (lt) { best.d = rd; best.idx = rid; best.pos = wpos; best.q = w8; }
        }
    }
}

}  // namespace visma
