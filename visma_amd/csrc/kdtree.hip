// kdtree.hip -- open3d::KDTreeFlann on the device (visma_icp_kdtree_*): a cloud resident on the GPU, searched for ANY query
// points -- KNN, Radius, Hybrid -- with the neighbour search of nn_list.h over the grid of nn_grid.hip.  What is this
// file's own:
//   kd_query            the query of thread t from an external f64 array, binned with the arithmetic that binned the cloud
//                       and clamped into the grid; how far it lies outside the grid's box
//   kd_list_kernel      KNN / Hybrid: NnList in LDS up to kNormalsMaxList entries, NnHeap in global memory above, the rows
//                       written in the queries' order; the queries of a call go through it in slabs
//   kd_count_kernel,    Radius without a cap: count (NnCount), the exclusive scan of compact.h over the counts, and a write
//   kd_write_kernel     pass in which every query fills its own CSR segment as a heap and sorts it in place
// One thread per query in the caller's order, one writer per output element, no floating-point atomics.
#include "compact.h"
#include "dev_mem.h"
#include "nn_list.h"

#include <math.h>

#include <algorithm>
#include <memory>

namespace visma {

namespace {

struct KdArgs {
    NnGridView view;
    const double *q;             // the queries of this launch, nq x 3
    double origin[3];            // the cloud's binning origin (NnGrid::build)
    int nq;
    int cap;                     // list capacity: min(the caller's cap, n)
    int out_cap;                 // row length of idx / d2: the caller's cap
    double r2d;                  // (double)(float)(r * r); unused for KNN
    int *idx;                    // KNN / Hybrid: nq x out_cap, -1 behind the list.  Radius: the CSR entries
    double *d2;                  // ... +inf behind the list
    int *cnt;                    // nq
    double *heap_d2;             // (NnHeap) [cap][nq]
    int *heap_id;
    const long long *offsets;    // (Radius, write pass) where the segment of query t starts
};

// The query of thread t.  Its cell: (float)(x - origin), the subtraction in f64 -- what nn_pack_kernel stored for a point
// of the cloud --, through cell_coord, clamped into the grid.  A NaN coordinate lands in cell 0 of its axis (cell_coord's
// fmaxf drops the NaN), an infinite one in the first or the last; nn_accept then rejects what it must.
// *outside2: the squared distance from the query to the grid's box, 0.1 % of a cell short on every axis (the fp32 binning).
__device__ __forceinline__ NnQuery kd_query(const KdArgs &a, long long t, double *outside2)
{
    const GridParams &g = a.view.g;
    NnQuery q;
    q.p = Pt64{a.q[3 * t], a.q[3 * t + 1], a.q[3 * t + 2], (unsigned long long)t};
    const double x[3] = {q.p.x, q.p.y, q.p.z};
    const float inv[3] = {g.inv_h, g.inv_hs, g.inv_hs};
    const double edge[3] = {(double)g.h, (double)g.hs, (double)g.hs};
    int c[3];
    double o2 = 0.0;
    for (int k = 0; k < 3; k++) {
        q.b[k] = x[k] - a.origin[k];
        c[k] = min(max(cell_coord((float)q.b[k], g.mn[k], inv[k], g.dim[k]), 0), g.dim[k] - 1);
        const double u = q.b[k] - (double)g.mn[k];
        const double o = fmax(fmax(-u, u - (double)g.dim[k] * edge[k]) - 1e-3 * edge[k], 0.0);
        o2 += o * o;
    }
    q.cx = c[0]; q.cy = c[1]; q.cz = c[2];
    q.me = (int)t;
    *outside2 = o2;
    return q;
}

__device__ __forceinline__ void kd_copy_out(const KdArgs &a, long long t, const NnEntries &L)
{
    int *oi = a.idx + (size_t)t * a.out_cap;
    double *od = a.d2 + (size_t)t * a.out_cap;
    for (int j = 0; j < a.out_cap; j++) {
        const bool in = j < L.cnt;
        oi[j] = in ? L.id[(size_t)j * L.stride] : -1;
        od[j] = in ? L.d2[(size_t)j * L.stride] : INFINITY;
    }
    a.cnt[t] = L.cnt;
}

// Radius / Hybrid: a query farther than the radius from the grid's box has no partner and scans nothing
__device__ __forceinline__ bool kd_in_reach(bool knn, double outside2, double r2d) { return knn || !(outside2 > r2d); }

// KNN (true) or Hybrid.  HEAP: NnHeap in global memory instead of NnList in LDS.
template <bool KNN, int NTH, bool HEAP>
__global__ __launch_bounds__(NTH) void kd_list_kernel(KdArgs a)
{
    extern __shared__ double lds_raw[];
    const long long t = (long long)blockIdx.x * NTH + threadIdx.x;
    if (t >= a.nq) return;
    double outside2;
    const NnQuery q = kd_query(a, t, &outside2);
    const auto accept = nn_accept<KNN>(a.r2d);
    const bool reach = kd_in_reach(KNN, outside2, a.r2d);
    if constexpr (HEAP) {
        NnHeap L = nn_heap_global(a.heap_d2, a.heap_id, t, a.nq, a.cap);
        if (reach) nn_search<KNN>(a.view, q, L, accept);
        L.sort();
        kd_copy_out(a, t, L);
    } else {
        NnList L = nn_list_lds(lds_raw, threadIdx.x, NTH, a.cap);
        if (reach) nn_search<KNN>(a.view, q, L, accept);
        kd_copy_out(a, t, L);
    }
}

template <int NTH>
__global__ __launch_bounds__(NTH) void kd_count_kernel(KdArgs a)
{
    const long long t = (long long)blockIdx.x * NTH + threadIdx.x;
    if (t >= a.nq) return;
    double outside2;
    const NnQuery q = kd_query(a, t, &outside2);
    NnCount L;
    if (kd_in_reach(false, outside2, a.r2d)) nn_search<false>(a.view, q, L, nn_accept<false>(a.r2d));
    a.cnt[t] = L.cnt;
}

// the segment of query t, cnt[t] entries at offsets[t]: filled as a max-heap (never past its end: a full heap replaces its
// root), then heap-sorted in place into ascending (d2, index)
template <int NTH>
__global__ __launch_bounds__(NTH) void kd_write_kernel(KdArgs a)
{
    const long long t = (long long)blockIdx.x * NTH + threadIdx.x;
    if (t >= a.nq) return;
    const int len = a.cnt[t];
    if (len <= 0) return;
    double outside2;
    const NnQuery q = kd_query(a, t, &outside2);
    NnHeap L;
    L.d2 = a.d2 + a.offsets[t];
    L.id = a.idx + a.offsets[t];
    L.stride = 1;
    L.cap = len;
    nn_search<false>(a.view, q, L, nn_accept<false>(a.r2d));
    L.sort();
}


}  // namespace

struct KdTreeDevice {
    int64_t n = 0;
    double origin[3] = {0.0, 0.0, 0.0};
    DeviceBuf<double> xyz;               // the cloud, n x 3
    // the grid of the last search: built for a radius (Radius / Hybrid) or for a knn (NnGrid::build sizes the cells)
    std::unique_ptr<NnGrid> grid;
    bool grid_knn = false;
    double grid_radius = 0.0;
    int grid_cap = 0;
    // what a call works in: grow-only
    DeviceBuf<double> q, out_d2, heap_d2;
    DeviceBuf<int> out_idx, heap_id, cnt;
    DeviceBuf<long long> offsets;        // nq + 1: the last is the total
    // the lists of the last Radius search
    DeviceBuf<int> r_idx;
    DeviceBuf<double> r_d2;
    int64_t r_total = -1;                        // -1: none

    hipError_t ensure_grid(bool knn, double radius, int cap, hipStream_t stream)
    {
        if (grid && grid_knn == knn && (knn ? grid_cap == cap : grid_radius == radius)) return hipSuccess;
        grid.reset();                             // (a build keeps the cell tables of the one before it: start from none)
        std::unique_ptr<NnGrid> g(new NnGrid);
        VISMA_TRY(g->alloc(n));
        ColorGradientInput in;
        in.xyz = xyz.get(); in.n = n;
        for (int k = 0; k < 3; k++) in.origin[k] = origin[k];
        VISMA_TRY(g->build(in, nullptr, radius, knn ? cap : 0, stream));
        grid = std::move(g);
        grid_knn = knn; grid_radius = radius; grid_cap = cap;
        return hipSuccess;
    }
    KdArgs args(int64_t nq) const
    {
        KdArgs a{};
        a.view = grid->view;
        a.q = q.get();
        for (int k = 0; k < 3; k++) a.origin[k] = origin[k];
        a.nq = (int)nq;
        return a;
    }
};

hipError_t kdtree_device_create(const double *h_xyz, int64_t n, hipStream_t stream, KdTreeDevice **out)
{
    *out = nullptr;
    std::unique_ptr<KdTreeDevice> T(new KdTreeDevice);
    T->n = n;
    nn_binning_origin(h_xyz, n, T->origin);
    DEV_RESERVE(T->xyz, 3 * (size_t)n);
    VISMA_TRY(hipMemcpyAsync(T->xyz.get(), h_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = T.release();
    return hipSuccess;
}

void kdtree_device_destroy(KdTreeDevice *T) { delete T; }

namespace {

template <bool KNN, bool HEAP>
hipError_t launch_lists(const KdArgs &a, hipStream_t stream)
{
    return nn_launch(HEAP ? 0 : a.cap, a.nq, a, stream, [](auto nth) { return &kd_list_kernel<KNN, decltype(nth)::value, HEAP>; });
}

}  // namespace

hipError_t kdtree_device_search(KdTreeDevice *T, bool knn, const double *h_q, int64_t nq, double radius, int cap,
                                int32_t *h_idx, double *h_d2, int32_t *h_cnt, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    const int eff = (int)std::min<int64_t>(cap, T->n);
    VISMA_TRY(T->ensure_grid(knn, radius, eff, stream));
    const bool heap = eff > kNormalsMaxList;
    // slabs: the rows of one launch, and its heaps, hold kKdTreeSlabEntries entries at the most (one query where a row is longer)
    const int64_t slab = std::min<int64_t>(nq, std::max<int64_t>(1, kKdTreeSlabEntries / cap));
    DEV_RESERVE(T->q, 3 * (size_t)slab);
    DEV_RESERVE(T->out_idx, (size_t)slab * (size_t)cap);
    DEV_RESERVE(T->out_d2, (size_t)slab * (size_t)cap);
    DEV_RESERVE(T->cnt, (size_t)slab);
    if (heap) {
        DEV_RESERVE(T->heap_d2, (size_t)slab * (size_t)eff);
        DEV_RESERVE(T->heap_id, (size_t)slab * (size_t)eff);
    }
    for (int64_t at = 0; at < nq; at += slab) {
        const int64_t m = std::min<int64_t>(slab, nq - at);
        VISMA_TRY(hipMemcpyAsync(T->q.get(), h_q + 3 * at, sizeof(double) * 3 * (size_t)m, hipMemcpyHostToDevice, stream));
        KdArgs a = T->args(m);
        a.cap = eff; a.out_cap = cap;
        a.r2d = nn_radius2(radius);
        a.idx = T->out_idx.get(); a.d2 = T->out_d2.get(); a.cnt = T->cnt.get();
        a.heap_d2 = T->heap_d2.get(); a.heap_id = T->heap_id.get();
        if (knn) VISMA_TRY(heap ? (launch_lists<true, true>(a, stream)) : (launch_lists<true, false>(a, stream)));
        else VISMA_TRY(heap ? (launch_lists<false, true>(a, stream)) : (launch_lists<false, false>(a, stream)));
        const size_t rows = (size_t)m * (size_t)cap;
        VISMA_TRY(hipMemcpyAsync(h_idx + (size_t)at * cap, a.idx, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, stream));
        VISMA_TRY(hipMemcpyAsync(h_d2 + (size_t)at * cap, a.d2, sizeof(double) * rows, hipMemcpyDeviceToHost, stream));
        VISMA_TRY(hipMemcpyAsync(h_cnt + at, a.cnt, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream));
        VISMA_TRY(hipStreamSynchronize(stream));             // (the next slab writes the same buffers)
    }
    return hipSuccess;
}

hipError_t kdtree_device_search_radius(KdTreeDevice *T, const double *h_q, int64_t nq, double radius, int64_t *h_offsets,
                                       int64_t *total, hipStream_t stream)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "the offsets are copied out as they are");
    T->r_total = -1;
    *total = 0;
    h_offsets[0] = 0;
    if (nq <= 0) { T->r_total = 0; return hipSuccess; }
    VISMA_TRY(T->ensure_grid(false, radius, 0, stream));
    DEV_RESERVE(T->q, 3 * (size_t)nq);
    DEV_RESERVE(T->cnt, (size_t)nq);
    DEV_RESERVE(T->offsets, (size_t)nq + 1);
    VISMA_TRY(hipMemcpyAsync(T->q.get(), h_q, sizeof(double) * 3 * (size_t)nq, hipMemcpyHostToDevice, stream));
    KdArgs a = T->args(nq);
    a.r2d = nn_radius2(radius);
    a.cnt = T->cnt.get();
    VISMA_TRY(nn_launch(0, nq, a, stream, [](auto nth) { return &kd_count_kernel<decltype(nth)::value>; }));
    long long *const d_total = T->offsets.get() + nq;
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, (const int *)a.cnt, (long long)nq, T->offsets.get(), d_total);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(hipMemcpyAsync(h_offsets, T->offsets.get(), sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    *total = h_offsets[nq];
    if (*total > kKdTreeMaxRadiusEntries) return hipErrorOutOfMemory;
    DEV_RESERVE(T->r_idx, (size_t)*total);
    DEV_RESERVE(T->r_d2, (size_t)*total);
    a.idx = T->r_idx.get(); a.d2 = T->r_d2.get(); a.offsets = T->offsets.get();
    VISMA_TRY(nn_launch(0, nq, a, stream, [](auto nth) { return &kd_write_kernel<decltype(nth)::value>; }));
    VISMA_TRY(hipStreamSynchronize(stream));
    T->r_total = *total;
    return hipSuccess;
}

hipError_t kdtree_device_radius_result(KdTreeDevice *T, int32_t *h_idx, double *h_d2, hipStream_t stream)
{
    if (T->r_total < 0) return hipErrorNotReady;
    if (T->r_total == 0) return hipSuccess;                        // (nothing is written: the arrays may be NULL)
    if (!h_idx || !h_d2) return hipErrorInvalidValue;
    VISMA_TRY(hipMemcpyAsync(h_idx, T->r_idx.get(), sizeof(int32_t) * (size_t)T->r_total, hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipMemcpyAsync(h_d2, T->r_d2.get(), sizeof(double) * (size_t)T->r_total, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

}  // namespace visma
