// fpfh.hip -- open3d::ComputeFPFHFeature on gfx950 (O3D/Core/Registration/Feature.cpp:38-157; Rusu, Blodow, Beetz: "Fast
// Point Feature Histograms (FPFH) for 3D Registration", ICRA 2009): the 33-bin descriptor per point that fast global
// registration matches when there is no initial pose.
//
// Two passes over one neighbour list per point -- KNN(knn) or Hybrid(radius, max_nn); the grid and the tuning of its cells
// are nn_grid.hip's, the search and the list nn_list.h's, shared with normals.hip and color_gradient.hip:
//   SPFH (:72-108)   entry 0 of the list is skipped whatever index it holds, every other entry gives the four pair
//                    features of ComputePairFeatures (:38-70), three of which are binned into 11 bins each with the
//                    weight 100 / (len - 1); a list of length <= 1 leaves the column zero.
//   FPFH (:126-154)  over the same list, entry 0 and entries at distance 0 skipped: the neighbours' SPFH / d2 summed per
//                    bin and per histogram in list order, each histogram rescaled to 100 where its sum is not 0, the
//                    point's own SPFH added.
// All f64, statement by statement; the build keeps -ffp-contract=off.  A bin argument that is not finite, or that (int)
// cannot hold, goes to bin 0: what (int) of such a double followed by the clamp gives on the reference's platform.  A
// non-finite normal or coordinate reaches sums only, never an index or an address.
//
// One thread per point, in cell order; lists of up to kNormalsMaxList entries in LDS, nn_list_threads(cap) threads per
// workgroup by nn_launch (cap = 100: 64 threads on 75 KiB, two workgroups per CU by LDS).  The second pass needs the lists again: the first pass either
// KEEPS them in global memory ([cap][n], 12 bytes per entry, read back coalesced) or the second pass REBUILDS them by the
// same search.  Kept where they fit the budget below (measured: DESIGN.md 4.4c7, profiles/fpfh_fgr_probe.txt).
#include "nn_list.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace visma {

namespace {

constexpr int kFpfhDim = 33;

struct FpfhArgs {
    NnGridView view;
    const double *nrm;           // n x 3, original order
    double *spfh;                // n x 33, original order
    double *out;                 // n x 33, original order
    int n;
    int cap;                     // list capacity: min(knn, n)
    double r2d;                  // (double)(float)(r * r); unused for KNN
    double *keep_d2;             // kept lists: [cap][n] by query in cell order, or NULL
    int *keep_id;
    int *keep_cnt;               // n
};

// (int)floor(v) clamped to [0, 10] as Feature.cpp:92-94 gives it on x86-64: the conversion of a NaN, an infinity or a value
// int cannot hold is INT_MIN there, which the clamp turns into 0
__device__ __forceinline__ int fpfh_bin(double v)
{
    v = floor(v);
    if (!(v > -2147483649.0 && v < 2147483648.0)) return 0;
    if (v < 0.0) return 0;
    if (v >= 11.0) return 10;
    return (int)v;
}

// Feature.cpp:38-70, f[0..2] only (f[3], the distance, is never binned).  Eigen's dot, cross and norm written out.
__device__ __forceinline__ void pair_features(const Pt64 &p1, const double *n1, const Pt64 &p2, const double *n2, double f[3])
{
    double d[3] = {p2.x - p1.x, p2.y - p1.y, p2.z - p1.z};
    const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    f[0] = 0.0; f[1] = 0.0; f[2] = 0.0;
    if (len == 0.0) return;
    double a[3] = {n1[0], n1[1], n1[2]}, b[3] = {n2[0], n2[1], n2[2]};
    const double angle1 = (a[0] * d[0] + a[1] * d[1] + a[2] * d[2]) / len;
    const double angle2 = (b[0] * d[0] + b[1] * d[1] + b[2] * d[2]) / len;
    double f2;
    if (acos(fabs(angle1)) > acos(fabs(angle2))) {
        for (int k = 0; k < 3; k++) { a[k] = n2[k]; b[k] = n1[k]; d[k] *= -1.0; }
        f2 = -angle2;
    } else {
        f2 = angle1;
    }
    double v[3] = {d[1] * a[2] - d[2] * a[1], d[2] * a[0] - d[0] * a[2], d[0] * a[1] - d[1] * a[0]};
    const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (vn == 0.0) return;
    v[0] /= vn; v[1] /= vn; v[2] /= vn;
    const double w[3] = {a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]};
    f[2] = f2;
    f[1] = v[0] * b[0] + v[1] * b[1] + v[2] * b[2];
    f[0] = atan2(w[0] * b[0] + w[1] * b[1] + w[2] * b[2], a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}

// The FPFH column of one point from its list (Feature.cpp:130-154): len entries, entry j at d2[j * stride], id[j * stride]
__device__ __forceinline__ void fpfh_column(const FpfhArgs &a, int me, int len, const double *d2, const int *id, size_t stride)
{
    double f[kFpfhDim];
#pragma unroll
    for (int j = 0; j < kFpfhDim; j++) f[j] = 0.0;
    if (len > 1) {
        double sum[3] = {0.0, 0.0, 0.0};
        for (int k = 1; k < len; k++) {
            const double dist = d2[(size_t)k * stride];
            if (dist == 0.0) continue;
            const double *s = a.spfh + (size_t)id[(size_t)k * stride] * kFpfhDim;
#pragma unroll
            for (int j = 0; j < kFpfhDim; j++) {
                const double val = s[j] / dist;
                sum[j / 11] += val;
                f[j] += val;
            }
        }
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (sum[j] != 0.0) sum[j] = 100.0 / sum[j];
        const double *own = a.spfh + (size_t)me * kFpfhDim;
#pragma unroll
        for (int j = 0; j < kFpfhDim; j++) {
            f[j] *= sum[j / 11];
            f[j] += own[j];
        }
    }
    double *o = a.out + (size_t)me * kFpfhDim;
#pragma unroll
    for (int j = 0; j < kFpfhDim; j++) o[j] = f[j];
}

// TYPE: 0 KNN, 2 Hybrid.  PASS 0: SPFH (and the lists to global memory where a.keep_d2 is set); PASS 1: the list rebuilt,
// then FPFH.
template <int TYPE, int NTH, int PASS>
__global__ __launch_bounds__(NTH) void fpfh_search_kernel(FpfhArgs a)
{
    extern __shared__ double lds_raw[];
    const long long t = (long long)blockIdx.x * NTH + threadIdx.x;
    // (the list's addresses before the bounds test: the kernel argument loads then merge as they did before the search moved
    // to nn_list.h, and the search loop keeps its place in the instruction cache lines -- 4 bytes off cost 1.7 % of a pass,
    // profiles/nn_search_ab.txt)
    NnList L = nn_list_lds(lds_raw, threadIdx.x, NTH, a.cap);
    if (t >= a.n) return;
    const NnQuery query = nn_query(a.view, t);                    // queries in cell order
    // nn_list.h's rule (Hybrid: flann's radiusSearch, strict; a neighbour at a NaN distance is never listed)
    nn_search<TYPE == 0>(a.view, query, L, nn_accept<TYPE == 0>(a.r2d));
    const Pt64 q = query.p;
    const int me = query.me;
    if (PASS == 1) {
        fpfh_column(a, me, L.cnt, L.d2, L.id, L.stride);
        return;
    }
    if (a.keep_d2) {
        a.keep_cnt[t] = L.cnt;
        for (int j = 0; j < L.cnt; j++) {
            a.keep_d2[(size_t)j * a.n + t] = L.d2[(size_t)j * L.stride];
            a.keep_id[(size_t)j * a.n + t] = L.id[(size_t)j * L.stride];
        }
    }
    double h[kFpfhDim];
    for (int j = 0; j < kFpfhDim; j++) h[j] = 0.0;
    if (L.cnt > 1) {                                              // :85-104
        const double n1[3] = {a.nrm[3ll * me], a.nrm[3ll * me + 1], a.nrm[3ll * me + 2]};
        const double incr = 100.0 / (double)(L.cnt - 1);
        for (int k = 1; k < L.cnt; k++) {
            const int id = L.id[(size_t)k * L.stride];
            const Pt64 p = a.view.pts[id];
            const double n2[3] = {a.nrm[3ll * id], a.nrm[3ll * id + 1], a.nrm[3ll * id + 2]};
            double f[3];
            pair_features(q, n1, p, n2, f);
            h[fpfh_bin(11 * (f[0] + M_PI) / (2.0 * M_PI))] += incr;
            h[fpfh_bin(11 * (f[1] + 1.0) * 0.5) + 11] += incr;
            h[fpfh_bin(11 * (f[2] + 1.0) * 0.5) + 22] += incr;
        }
    }
    double *o = a.spfh + (size_t)me * kFpfhDim;
    for (int j = 0; j < kFpfhDim; j++) o[j] = h[j];
}

// the second pass over kept lists: one thread per point in cell order, the list read back coalesced
__global__ __launch_bounds__(256) void fpfh_from_lists_kernel(FpfhArgs a)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const int me = (int)a.view.sorted64[t].w;
    fpfh_column(a, me, a.keep_cnt[t], a.keep_d2 + t, a.keep_id + t, (size_t)a.n);
}

template <int TYPE, int PASS>
hipError_t launch_fpfh(const FpfhArgs &a, hipStream_t stream)
{
    return nn_launch(a.cap, a.n, a, stream, [](auto nth) { return &fpfh_search_kernel<TYPE, decltype(nth)::value, PASS>; });
}

}  // namespace

// search_type 0 KNN(knn) | 2 Hybrid(radius, max_nn = knn); knn in [2, kNormalsMaxList].  second_pass 0: lists kept where
// they fit, 1: kept, 2: rebuilt.  ms (may be NULL): device time of the grid build, the first and the second pass.
hipError_t compute_fpfh_device(const double *h_xyz, int64_t n, const double *h_nrm, int search_type, int knn, double radius,
                               double *h_out, int second_pass, double ms[3], hipStream_t stream)
{
    if (ms) ms[0] = ms[1] = ms[2] = 0.0;
    if (n <= 0) return hipSuccess;
    if ((search_type != 0 && search_type != 2) || knn < 2 || knn > kNormalsMaxList || n > 0x7fffffff || second_pass < 0 ||
        second_pass > 2)
        return hipErrorInvalidValue;
    const bool use_r = search_type == 2;
    const int cap = (int)std::min<int64_t>(knn, n);
    // no neighbours for any point (KDTreeFlann.cpp:171-176; one point: the list is the point itself): every column zero
    if ((use_r && (!(radius > 0.0) || !std::isfinite(radius))) || cap < 2) {
        std::fill(h_out, h_out + (size_t)n * kFpfhDim, 0.0);
        return hipSuccess;
    }
    NnGrid G;
    DevBufs B;
    DevEvents<4> ev;
    double *d_xyz = nullptr, *d_nrm = nullptr, *d_spfh = nullptr, *d_out = nullptr;
    VISMA_TRY(B.alloc(&d_xyz, 3 * (size_t)n));
    VISMA_TRY(B.alloc(&d_nrm, 3 * (size_t)n));
    VISMA_TRY(B.alloc(&d_spfh, kFpfhDim * (size_t)n));
    VISMA_TRY(B.alloc(&d_out, kFpfhDim * (size_t)n));
    VISMA_TRY(G.alloc(n));
    VISMA_TRY(ev.create());
    VISMA_TRY(hipMemcpyAsync(d_xyz, h_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    VISMA_TRY(hipMemcpyAsync(d_nrm, h_nrm, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    VISMA_TRY(hipEventRecord(ev[0], stream));                     // ms[0]: from here, the uploads queued ...
    ColorGradientInput in;
    in.xyz = d_xyz; in.n = n;
    nn_binning_origin(h_xyz, n, in.origin);
    VISMA_TRY(G.build(in, nullptr, radius, use_r ? 0 : cap, stream));
    FpfhArgs a{};
    a.view = G.view;
    a.nrm = d_nrm; a.spfh = d_spfh; a.out = d_out; a.n = (int)n; a.cap = cap;
    a.r2d = nn_radius2(radius);
    // the lists kept for the second pass: n * cap * 12 bytes, within 1 GiB and half of what the device has free
    bool keep = second_pass != 2;
    const size_t entries = (size_t)n * (size_t)cap;
    if (second_pass == 0) {
        size_t budget = (size_t)1 << 30, free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, free_b / 2);
        keep = entries * kNnListEntryBytes <= budget;
    }
    if (keep) {
        VISMA_TRY(B.alloc(&a.keep_d2, entries));
        VISMA_TRY(B.alloc(&a.keep_id, entries));
        VISMA_TRY(B.alloc(&a.keep_cnt, (size_t)n));
    }
    VISMA_TRY(hipEventRecord(ev[1], stream));
    if (use_r) VISMA_TRY((launch_fpfh<2, 0>(a, stream)));
    else VISMA_TRY((launch_fpfh<0, 0>(a, stream)));
    VISMA_TRY(hipEventRecord(ev[2], stream));
    if (keep) {
        hipLaunchKernelGGL(fpfh_from_lists_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
        VISMA_TRY(hipGetLastError());
    } else if (use_r) {
        VISMA_TRY((launch_fpfh<2, 1>(a, stream)));
    } else {
        VISMA_TRY((launch_fpfh<0, 1>(a, stream)));
    }
    VISMA_TRY(hipEventRecord(ev[3], stream));
    VISMA_TRY(hipMemcpyAsync(h_out, d_out, sizeof(double) * kFpfhDim * (size_t)n, hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    if (ms)
        for (int k = 0; k < 3; k++) {
            float t = 0.f;
            VISMA_TRY(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
            ms[k] = (double)t;
        }
    return hipSuccess;
}

}  // namespace visma
