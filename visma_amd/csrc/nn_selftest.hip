// nn_selftest.hip -- the neighbour lists of nn_list.h handed out as they are (visma_icp_selftest_neighbor_lists,
// visma_icp_testing.h): the grid of nn_grid.hip built as normals.hip builds it, nn_query, nn_search with nn_accept, and the
// list copied out in the caller's point order.  Both kinds of list: NnList in LDS through nn_launch, NnHeap in global memory
// as [cap][n], heap-sorted at the end.  Tests only; no product path calls it.
#include "nn_list.h"

#include <math.h>

#include <algorithm>

namespace visma {

namespace {

struct NnSelftestArgs {
    NnGridView view;
    int n;
    int cap;                     // list capacity: min(the caller's cap, n)
    int out_cap;                 // row length of idx / d2: the caller's cap
    double r2d;                  // (double)(float)(r * r); unused for KNN
    int *idx;                    // n x out_cap, -1 behind the list
    double *d2;                  // n x out_cap, +inf behind the list
    int *cnt;                    // n
    double *heap_d2;             // (NnHeap) [cap][n]
    int *heap_id;
};

__device__ __forceinline__ void copy_out(const NnSelftestArgs &a, int me, const NnEntries &L)
{
    int *oi = a.idx + (size_t)me * a.out_cap;
    double *od = a.d2 + (size_t)me * a.out_cap;
    for (int j = 0; j < a.out_cap; j++) {
        const bool in = j < L.cnt;
        oi[j] = in ? L.id[(size_t)j * L.stride] : -1;
        od[j] = in ? L.d2[(size_t)j * L.stride] : INFINITY;
    }
    a.cnt[me] = L.cnt;
}

// TYPE: 0 KNN, 1 Radius (the counting pass), 2 Hybrid.  HEAP: NnHeap in global memory instead of NnList in LDS.
template <int TYPE, int NTH, bool HEAP>
__global__ __launch_bounds__(NTH) void nn_selftest_kernel(NnSelftestArgs a)
{
    extern __shared__ double lds_raw[];
    const long long t = (long long)blockIdx.x * NTH + threadIdx.x;
    if (t >= a.n) return;
    const NnQuery q = nn_query(a.view, t);                          // queries in cell order
    const auto accept = nn_accept<TYPE == 0>(a.r2d);
    if constexpr (TYPE == 1) {
        NnCount L;
        nn_search<false>(a.view, q, L, accept);
        a.cnt[q.me] = L.cnt;
    } else if constexpr (HEAP) {
        NnHeap L = nn_heap_global(a.heap_d2, a.heap_id, t, a.n, a.cap);
        nn_search<TYPE == 0>(a.view, q, L, accept);
        L.sort();
        copy_out(a, q.me, L);
    } else {
        NnList L = nn_list_lds(lds_raw, threadIdx.x, NTH, a.cap);
        nn_search<TYPE == 0>(a.view, q, L, accept);
        copy_out(a, q.me, L);
    }
}

template <int TYPE, bool HEAP>
hipError_t launch_selftest(const NnSelftestArgs &a, hipStream_t stream)
{
    // only lists in LDS size the workgroup
    return nn_launch((TYPE == 1 || HEAP) ? 0 : a.cap, a.n, a, stream,
                     [](auto nth) { return &nn_selftest_kernel<TYPE, decltype(nth)::value, HEAP>; });
}

}  // namespace

// The arguments are checked by the caller (aux_api.cpp): n >= 1, search_type 0 | 1 | 2, cap >= 1 (list_kind 0: <=
// kNormalsMaxList), a finite radius > 0 unless KNN; h_idx / h_d2 may be NULL for search_type 1.
hipError_t nn_selftest_lists_device(const double *h_xyz, int64_t n, int search_type, int cap, double radius, int list_kind,
                                    int32_t *h_idx, double *h_d2, int32_t *h_cnt, hipStream_t stream)
{
    const bool lists = search_type != 1;
    const int eff = (int)std::min<int64_t>(cap, n);
    NnGrid G;
    DevBufs B;
    double *d_xyz = nullptr;
    NnSelftestArgs a{};
    VISMA_TRY(B.alloc(&d_xyz, 3 * (size_t)n));
    VISMA_TRY(B.alloc(&a.cnt, (size_t)n));
    if (lists) {
        VISMA_TRY(B.alloc(&a.idx, (size_t)n * (size_t)cap));
        VISMA_TRY(B.alloc(&a.d2, (size_t)n * (size_t)cap));
        if (list_kind == 1) {
            VISMA_TRY(B.alloc(&a.heap_d2, (size_t)n * (size_t)eff));
            VISMA_TRY(B.alloc(&a.heap_id, (size_t)n * (size_t)eff));
        }
    }
    VISMA_TRY(G.alloc(n));
    VISMA_TRY(hipMemcpyAsync(d_xyz, h_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    ColorGradientInput in;
    in.xyz = d_xyz; in.n = n;
    nn_binning_origin(h_xyz, n, in.origin);
    VISMA_TRY(G.build(in, nullptr, radius, search_type == 0 ? eff : 0, stream));
    a.view = G.view;
    a.n = (int)n; a.cap = eff; a.out_cap = cap;
    a.r2d = nn_radius2(radius);
    if (search_type == 1) VISMA_TRY((launch_selftest<1, false>(a, stream)));
    else if (search_type == 0 && list_kind == 0) VISMA_TRY((launch_selftest<0, false>(a, stream)));
    else if (search_type == 0) VISMA_TRY((launch_selftest<0, true>(a, stream)));
    else if (list_kind == 0) VISMA_TRY((launch_selftest<2, false>(a, stream)));
    else VISMA_TRY((launch_selftest<2, true>(a, stream)));
    if (lists) {
        VISMA_TRY(hipMemcpyAsync(h_idx, a.idx, sizeof(int32_t) * (size_t)n * (size_t)cap, hipMemcpyDeviceToHost, stream));
        VISMA_TRY(hipMemcpyAsync(h_d2, a.d2, sizeof(double) * (size_t)n * (size_t)cap, hipMemcpyDeviceToHost, stream));
    }
    VISMA_TRY(hipMemcpyAsync(h_cnt, a.cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    return hipSuccess;
}

}  // namespace visma
