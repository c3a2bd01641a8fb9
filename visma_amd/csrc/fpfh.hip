// fpfh.hip -- open3d::ComputeFPFHFeature on gfx950 (O3D/Core/Registration/Feature.cpp:38-157; Rusu, Blodow, Beetz: "Fast
// Point Feature Histograms (FPFH) for 3D Registration", ICRA 2009): the 33-bin descriptor per point that fast global
// registration matches when there is no initial pose.
//
// Two passes over one neighbour list per point -- KNN(knn) or Hybrid(radius, max_nn), the list, its order and the walk over
// the cells nn_list.h's, shared with normals.hip and color_gradient.hip:
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
// workgroup (cap = 100: 64 threads on 75 KiB, two workgroups per CU by LDS).  The second pass needs the lists again: the first pass either
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
    const float4 *sorted;        // cell-sorted fp32 copy (cell binning only)
    const Pt64 *sorted64;        // cell-sorted points, w = original index
    const unsigned *start;
    GridParams g;
    const Pt64 *pts;             // original order
    const double *nrm;           // n x 3, original order
    double *spfh;                // n x 33, original order
    double *out;                 // n x 33, original order
    int n;
    int cap;                     // list capacity: min(knn, n)
    double r2d;                  // (double)(float)(r * r); unused for KNN
    double *keep_d2;             // kept lists: [cap][n] by query in cell order, or NULL
    int *keep_id;
    int *keep_cnt;               // n
    unsigned long long *n27;     // (sampling pass) sum of 27-cell populations, queries counted
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
// then FPFH; PASS 2: only count the 27-cell population of every 64th point (KNN cell-size tuning, as normals.hip).
template <int TYPE, int NTH, int PASS>
__global__ __launch_bounds__(NTH) void fpfh_search_kernel(FpfhArgs a)
{
    extern __shared__ double lds_raw[];
    const int tid = threadIdx.x;
    const long long t = (long long)blockIdx.x * NTH + tid;
    if (t >= a.n) return;
    const Pt64 q = a.sorted64[t];                                 // queries in cell order
    const float4 qf = a.sorted[t];
    const GridParams g = a.g;
    const int cx = cell_coord(qf.x, g.mn[0], g.inv_h, g.dim[0]);
    const int cy = cell_coord(qf.y, g.mn[1], g.inv_hs, g.dim[1]);
    const int cz = cell_coord(qf.z, g.mn[2], g.inv_hs, g.dim[2]);
    if (PASS == 2) {
        if ((t & 63) != 0) return;
        unsigned long long tot = 0;
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++) {
                const int z = cz + dz, y = cy + dy;
                if (z < 0 || z >= g.dim[2] || y < 0 || y >= g.dim[1]) continue;
                const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
                if (x0 > x1) continue;
                const long long row = ((long long)z * g.dim[1] + y) * g.dim[0];
                tot += a.start[row + x1 + 1] - a.start[row + x0];
            }
        atomicAdd(a.n27, tot);
        atomicAdd(a.n27 + 1, 1ull);
        return;
    }
    NnList L = nn_list_lds(lds_raw, tid, NTH, a.cap);
    auto consider = [&](const Pt64 &p) {
        const double d = nn_dist2(q, p);
        if (TYPE != 0 && !(d < a.r2d)) return;                    // flann radiusSearch: strict
        if (TYPE == 0 && d != d) return;                          // a NaN distance has no place in an ordered list
        nn_list_insert(L, d, (int)p.w);
    };
    const int rmax = TYPE == 0 ? max(max(g.dim[0], g.dim[1]), g.dim[2]) : 1;
    for (int R = 0; R <= rmax; R++) {
        nn_scan_shell(g, a.start, a.sorted64, cx, cy, cz, R, consider);
        if (TYPE != 0) continue;                                  // cells of edge 1.001 r: the 27 cover the radius
        // KNN: every point nearer than R cell edges has been seen (0.1 % slack for the fp32 binning); normals.hip
        if (L.cnt == a.cap && R >= 1) {
            const double cover = (double)R * (double)g.h * 0.999;
            if (L.d2[(size_t)(a.cap - 1) * L.stride] <= cover * cover) break;
        }
        if (cx - R <= 0 && cy - R <= 0 && cz - R <= 0 && cx + R >= g.dim[0] - 1 && cy + R >= g.dim[1] - 1 &&
            cz + R >= g.dim[2] - 1)
            break;                                                // the whole grid has been scanned
    }
    const int me = (int)q.w;
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
            const Pt64 p = a.pts[id];
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
    const int me = (int)a.sorted64[t].w;
    fpfh_column(a, me, a.keep_cnt[t], a.keep_d2 + t, a.keep_id + t, (size_t)a.n);
}

__global__ void fpfh_pack_kernel(const double *__restrict__ xyz, long long n, double cx, double cy, double cz,
                                 float4 *__restrict__ f4, Pt64 *__restrict__ p8)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    // the fp32 copy is for BINNING only, relative to a point of the cloud (normals.hip: pack_points_kernel)
    f4[i] = make_float4((float)(x - cx), (float)(y - cy), (float)(z - cz), __uint_as_float((unsigned)i));
    p8[i] = Pt64{x, y, z, (unsigned long long)i};
}

struct FpfhBufs {
    std::vector<void *> ptrs;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~FpfhBufs()
    {
        for (void *p : ptrs) (void)hipFree(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    template <class T>
    hipError_t alloc(T **out, size_t count)
    {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, sizeof(T) * std::max<size_t>(count, 1));
        if (e != hipSuccess) return e;
        ptrs.push_back(p);
        *out = (T *)p;
        return hipSuccess;
    }
};

template <int TYPE, int NTH, int PASS>
hipError_t launch_fpfh_nth(const FpfhArgs &a, size_t lds, hipStream_t stream)
{
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)fpfh_search_kernel<TYPE, NTH, PASS>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((fpfh_search_kernel<TYPE, NTH, PASS>), dim3((unsigned)((a.n + NTH - 1) / NTH)), dim3(NTH), lds, stream, a);
    return hipGetLastError();
}

template <int TYPE, int PASS>
hipError_t launch_fpfh(const FpfhArgs &a, hipStream_t stream)
{
    const int lds_cap = PASS == 2 ? 0 : a.cap;
    const int nth = nn_list_threads(lds_cap);
    const size_t lds = nn_list_lds_bytes(lds_cap, nth);
    if (nth == 256) return launch_fpfh_nth<TYPE, 256, PASS>(a, lds, stream);
    if (nth == 128) return launch_fpfh_nth<TYPE, 128, PASS>(a, lds, stream);
    return launch_fpfh_nth<TYPE, 64, PASS>(a, lds, stream);
}

}  // namespace

#define FPFH_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

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
    FpfhBufs B;
    double *d_xyz = nullptr, *d_nrm = nullptr, *d_spfh = nullptr, *d_out = nullptr;
    float4 *d_f4 = nullptr, *d_sorted = nullptr;
    Pt64 *d_p8 = nullptr, *d_sorted64 = nullptr;
    unsigned *d_box = nullptr, *d_cell_of = nullptr;
    unsigned long long *d_n27 = nullptr;
    FPFH_TRY(B.alloc(&d_xyz, 3 * (size_t)n));
    FPFH_TRY(B.alloc(&d_nrm, 3 * (size_t)n));
    FPFH_TRY(B.alloc(&d_spfh, kFpfhDim * (size_t)n));
    FPFH_TRY(B.alloc(&d_out, kFpfhDim * (size_t)n));
    FPFH_TRY(B.alloc(&d_f4, (size_t)n));
    FPFH_TRY(B.alloc(&d_sorted, (size_t)n + kSortedSlack));
    FPFH_TRY(B.alloc(&d_p8, (size_t)n));
    FPFH_TRY(B.alloc(&d_sorted64, (size_t)n));
    FPFH_TRY(B.alloc(&d_box, 8));
    FPFH_TRY(B.alloc(&d_cell_of, 2 * (size_t)n));
    FPFH_TRY(B.alloc(&d_n27, 2));
    for (hipEvent_t &e : B.ev) FPFH_TRY(hipEventCreate(&e));
    FPFH_TRY(hipMemcpyAsync(d_xyz, h_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    FPFH_TRY(hipMemcpyAsync(d_nrm, h_nrm, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    FPFH_TRY(hipEventRecord(B.ev[0], stream));
    {
        double c0[3] = {0.0, 0.0, 0.0};                           // a finite point of the cloud as the binning origin
        for (int64_t i = 0; i < n; i++)
            if (std::isfinite(h_xyz[3 * i]) && std::isfinite(h_xyz[3 * i + 1]) && std::isfinite(h_xyz[3 * i + 2])) {
                c0[0] = h_xyz[3 * i]; c0[1] = h_xyz[3 * i + 1]; c0[2] = h_xyz[3 * i + 2];
                break;
            }
        hipLaunchKernelGGL(fpfh_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_xyz, (long long)n,
                           c0[0], c0[1], c0[2], d_f4, d_p8);
        FPFH_TRY(hipGetLastError());
    }
    FPFH_TRY(launch_grid_bbox(d_f4, n, d_box, stream));
    unsigned box[6];
    FPFH_TRY(hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, stream));
    FPFH_TRY(hipStreamSynchronize(stream));
    float mn[3], mx[3];
    grid_decode_bbox(box, mn, mx);
    double diag = 0.0;
    for (int k = 0; k < 3; k++) diag += ((double)mx[k] - mn[k]) * ((double)mx[k] - mn[k]);
    diag = std::sqrt(diag);
    // KNN: a first guess of the distance to the knn-th neighbour on a surface, refined from the measured population of
    // the 27 cells (normals.hip); any cell size is exact, rings of cells are added until the knn-th distance is covered
    double cell = use_r ? radius : 0.6 * diag * std::sqrt((double)cap / (double)n);
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = 1.0;
    FpfhArgs a{};
    unsigned *d_count = nullptr, *d_start = nullptr, *d_bsum = nullptr;
    int64_t cell_cap = 0;
    for (int attempt = 0;; attempt++) {
        const int64_t max_cells = std::min<int64_t>(kGridMaxCells, std::max<int64_t>(4096, 8 * n));
        const GridParams g = grid_plan(mn, mx, cell, max_cells);
        if (g.ncell + 1 > cell_cap) {
            FPFH_TRY(B.alloc(&d_count, (size_t)g.ncell + 1));
            FPFH_TRY(B.alloc(&d_start, (size_t)g.ncell + 9));
            FPFH_TRY(B.alloc(&d_bsum, (size_t)grid_scan_blocks(g.ncell) + 1));
            cell_cap = g.ncell + 1;
        }
        FPFH_TRY(launch_grid_build(d_f4, n, g, d_cell_of, d_count, d_bsum, d_start, d_sorted, stream, d_p8, d_sorted64));
        a.sorted = d_sorted; a.sorted64 = d_sorted64; a.start = d_start; a.g = g; a.pts = d_p8; a.nrm = d_nrm;
        a.spfh = d_spfh; a.out = d_out; a.n = (int)n; a.cap = cap; a.n27 = d_n27;
        const float r2f = (float)(radius * radius);
        a.r2d = (double)r2f;
        if (use_r || attempt >= 3) break;
        FPFH_TRY(hipMemsetAsync(d_n27, 0, 2 * sizeof(unsigned long long), stream));
        FPFH_TRY((launch_fpfh<0, 2>(a, stream)));
        unsigned long long h27[2];
        FPFH_TRY(hipMemcpyAsync(h27, d_n27, sizeof(h27), hipMemcpyDeviceToHost, stream));
        FPFH_TRY(hipStreamSynchronize(stream));
        const double mean27 = h27[1] ? (double)h27[0] / h27[1] : 0.0, want = 2.5 * cap;
        if (mean27 >= 0.6 * want && mean27 <= 2.5 * want) break;
        const double f = mean27 > 0.0 ? std::sqrt(want / mean27) : 2.0;
        const double next = cell * std::min(std::max(f, 0.25), 4.0);
        if (g.h > (float)(cell * 1.01) && next < cell) break;              // the cell cap already enlarged the cells
        cell = next;
    }
    // the lists kept for the second pass: n * cap * 12 bytes, within 1 GiB and half of what the device has free
    bool keep = second_pass != 2;
    const size_t entries = (size_t)n * (size_t)cap;
    if (second_pass == 0) {
        size_t budget = (size_t)1 << 30, free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, free_b / 2);
        keep = entries * kNnListEntryBytes <= budget;
    }
    if (keep) {
        FPFH_TRY(B.alloc(&a.keep_d2, entries));
        FPFH_TRY(B.alloc(&a.keep_id, entries));
        FPFH_TRY(B.alloc(&a.keep_cnt, (size_t)n));
    }
    FPFH_TRY(hipEventRecord(B.ev[1], stream));
    if (use_r) FPFH_TRY((launch_fpfh<2, 0>(a, stream)));
    else FPFH_TRY((launch_fpfh<0, 0>(a, stream)));
    FPFH_TRY(hipEventRecord(B.ev[2], stream));
    if (keep) {
        hipLaunchKernelGGL(fpfh_from_lists_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
        FPFH_TRY(hipGetLastError());
    } else if (use_r) {
        FPFH_TRY((launch_fpfh<2, 1>(a, stream)));
    } else {
        FPFH_TRY((launch_fpfh<0, 1>(a, stream)));
    }
    FPFH_TRY(hipEventRecord(B.ev[3], stream));
    FPFH_TRY(hipMemcpyAsync(h_out, d_out, sizeof(double) * kFpfhDim * (size_t)n, hipMemcpyDeviceToHost, stream));
    FPFH_TRY(hipStreamSynchronize(stream));
    if (ms)
        for (int k = 0; k < 3; k++) {
            float t = 0.f;
            FPFH_TRY(hipEventElapsedTime(&t, B.ev[k], B.ev[k + 1]));
            ms[k] = (double)t;
        }
    return hipSuccess;
}

}  // namespace visma
