// nn_list.h -- the neighbour search of one query point on the radius-cell grid of grid.hip, as normals.hip, color_gradient.hip
// and fpfh.hip run it: one thread per point in cell order over the grid of one cloud (nn_grid.hip builds it: NnGrid), the
// result in the order of the reference's KDTreeFlann result list: ascending (d2, index), flann's sum of squares in f64.
//   NnGridView, nn_query   what every such kernel is given first, and the query of thread t
//   NnList                 the list in LDS as [cap][threads] (element j of thread t at j * threads + t), squared distances
//                          first, indices behind them; kept sorted
//   NnHeap                 the same surface over global memory: a max-heap while the search runs, sorted at the end
//   nn_accept              which distances enter a list: the one rule of every caller
//   nn_search              the walk over the rings of cells
//   nn_launch              threads per workgroup by the LDS the lists take, the kernel instantiated for them
// What a kernel does with its list -- moments, gradient rows, histograms -- is its own file's.
#pragma once
#include "device_common.h"

#include <type_traits>

namespace visma {

// bytes of LDS one thread's list of `cap` entries takes: a double and an int per entry
constexpr size_t kNnListEntryBytes = 12;

// threads per workgroup for lists of `cap` entries: a workgroup's lists within 60 KiB down to 64 threads (64 threads:
// up to 128 KiB of the 160 at cap = kNormalsMaxList)
inline int nn_list_threads(int cap)
{
    int nth = 256;
    while (nth > 64 && (size_t)cap * kNnListEntryBytes * nth > 60 * 1024) nth >>= 1;
    return nth;
}
inline size_t nn_list_lds_bytes(int cap, int nth) { return (size_t)cap * kNnListEntryBytes * nth + 64; }

// the bound of flann's radiusSearch: r * r rounded to fp32 (KDTreeFlann.cpp:157-158, 184-185)
inline double nn_radius2(double radius) { return (double)(float)(radius * radius); }

#ifdef __HIPCC__
// One workgroup of `queries` / NTH per NTH queries, NTH = nn_list_threads(lds_cap) and the dynamic LDS its lists take
// (lds_cap = 0: the kernel keeps no list there).  kernel_of(std::integral_constant<int, NTH>) returns the kernel's
// instantiation for NTH threads.
template <class Args, class KernelOf>
hipError_t nn_launch(int lds_cap, long long queries, const Args &a, hipStream_t stream, KernelOf kernel_of)
{
    if (queries <= 0) return hipSuccess;
    const int nth = nn_list_threads(lds_cap);
    const size_t lds = nn_list_lds_bytes(lds_cap, nth);
    auto launch = [&](auto nth_c) -> hipError_t {
        constexpr int NTH = decltype(nth_c)::value;
        void (*const kernel)(Args) = kernel_of(nth_c);
        if (lds > 48 * 1024)
            VISMA_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3((unsigned)((queries + NTH - 1) / NTH)), dim3(NTH), lds, stream, a);
        return hipGetLastError();
    };
    if (nth == 256) return launch(std::integral_constant<int, 256>{});
    if (nth == 128) return launch(std::integral_constant<int, 128>{});
    return launch(std::integral_constant<int, 64>{});
}

// the query of thread t (cell order): the point, its cell, its index in the caller's order; b: where the binning saw it
// (its coordinates relative to the binning origin) -- what the KNN stopping rule measures from
struct NnQuery {
    Pt64 p;
    double b[3];
    int cx, cy, cz;
    int me;
};
__device__ __forceinline__ NnQuery nn_query(const NnGridView &v, long long t)
{
    NnQuery q;
    q.p = v.sorted64[t];
    const float4 qf = v.sorted[t];
    // the cell the build put the point in (cell_count_kernel clamps the same way): an infinite coordinate collapses its
    // axis to one cell, and an unclamped query two cells beyond it would scan nothing
    q.cx = min(max(cell_coord(qf.x, v.g.mn[0], v.g.inv_h, v.g.dim[0]), 0), v.g.dim[0] - 1);
    q.cy = min(max(cell_coord(qf.y, v.g.mn[1], v.g.inv_hs, v.g.dim[1]), 0), v.g.dim[1] - 1);
    q.cz = min(max(cell_coord(qf.z, v.g.mn[2], v.g.inv_hs, v.g.dim[2]), 0), v.g.dim[2] - 1);
    q.b[0] = (double)qf.x; q.b[1] = (double)qf.y; q.b[2] = (double)qf.z;
    q.me = (int)q.p.w;
    return q;
}

// flann L2 (dist.h:159-176): result += diff * diff over x, y, z
__device__ __forceinline__ double nn_dist2(const Pt64 &q, const Pt64 &p)
{
    const double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    double d = dx * dx;
    d += dy * dy;
    d += dz * dz;
    return d;
}

// Which squared distances enter a list, for every caller.  A neighbour at a NaN distance is NEVER listed: a NaN has no place
// in an ordered list (in NnList it would sit at the end and block every later, nearer candidate; in NnHeap it would not).
//   KNN = true   every distance that is one (an infinite distance is a legitimate entry)
//   KNN = false  Radius / Hybrid: flann's radiusSearch, d2 < (double)(float)(r * r), strict -- false for a NaN
template <bool KNN>
struct NnAccept {
    double r2d;
    __device__ __forceinline__ bool operator()(double d) const { return KNN ? d == d : d < r2d; }
};
template <bool KNN>
__device__ __forceinline__ NnAccept<KNN> nn_accept(double r2d) { return NnAccept<KNN>{r2d}; }

// `cnt` of `cap` entries (d2, id), entry j at [j * stride]: what NnList and NnHeap keep, each in its own order
struct NnEntries {
    double *d2;
    int *id;
    size_t stride;
    int cap;
    int cnt = 0;

    __device__ __forceinline__ void set(int j, double d, int i) { d2[(size_t)j * stride] = d; id[(size_t)j * stride] = i; }
    __device__ __forceinline__ void move(int to, int from)
    {
        d2[(size_t)to * stride] = d2[(size_t)from * stride];
        id[(size_t)to * stride] = id[(size_t)from * stride];
    }
    // (d, i) before entry j
    __device__ __forceinline__ bool less(double d, int i, int j) const
    {
        const double dj = d2[(size_t)j * stride];
        return d < dj || (d == dj && i < id[(size_t)j * stride]);
    }
};

// the sorted list: ascending (d2, id) at any time
struct NnList : NnEntries {
    // keep the cap nearest: insertion into the sorted list, the farthest entry dropped when it is full
    __device__ __forceinline__ void insert(double d, int i)
    {
        int pos;
        if (cnt < cap) pos = cnt++;
        else if (less(d, i, cap - 1)) pos = cap - 1;
        else return;
        while (pos > 0 && less(d, i, pos - 1)) {
            move(pos, pos - 1);
            pos--;
        }
        set(pos, d, i);
    }
    // of a full list
    __device__ __forceinline__ double farthest() const { return d2[(size_t)(cap - 1) * stride]; }
};

// the list of thread `tid` of `nth` in the workgroup's dynamic LDS
__device__ __forceinline__ NnList nn_list_lds(double *lds_raw, int tid, int nth, int cap)
{
    NnList l;
    l.d2 = lds_raw + tid;
    l.id = reinterpret_cast<int *>(lds_raw + (size_t)cap * nth) + tid;
    l.stride = (size_t)nth;
    l.cap = cap;
    return l;
}

// the max-heap on (d2, id): the root is the entry a nearer candidate replaces; sort() then leaves the order of NnList
struct NnHeap : NnEntries {
    // (d, i) into the hole at `pos` of a heap of `len`: larger children move up
    __device__ __forceinline__ void sift_down(int pos, int len, double d, int i)
    {
        for (;;) {
            int ch = 2 * pos + 1;
            if (ch >= len) break;
            if (ch + 1 < len && less(d2[(size_t)ch * stride], id[(size_t)ch * stride], ch + 1)) ch++;
            if (!less(d, i, ch)) break;
            move(pos, ch);
            pos = ch;
        }
        set(pos, d, i);
    }
    __device__ __forceinline__ void insert(double d, int i)
    {
        if (cnt < cap) {
            // sift up: parents smaller than the new entry move down
            int pos = cnt++;
            while (pos > 0) {
                const int par = (pos - 1) >> 1;
                const double dp = d2[(size_t)par * stride];
                const int ip = id[(size_t)par * stride];
                if (!(dp < d || (dp == d && ip < i))) break;
                set(pos, dp, ip);
                pos = par;
            }
            set(pos, d, i);
        } else if (less(d, i, 0)) {
            sift_down(0, cap, d, i);
        }
    }
    // of a full heap
    __device__ __forceinline__ double farthest() const { return d2[0]; }
    // heap sort in place: ascending (d2, id) = the order of the reference's result list
    __device__ __forceinline__ void sort()
    {
        for (int end = cnt - 1; end > 0; end--) {
            const double dl = d2[(size_t)end * stride];
            const int il = id[(size_t)end * stride];
            move(end, 0);
            sift_down(0, end, dl, il);
        }
    }
};

// the heap of query `u` of a slab of `queries`, in global memory as [cap][queries] (coalesced across threads)
__device__ __forceinline__ NnHeap nn_heap_global(double *d2, int *id, long long u, int queries, int cap)
{
    NnHeap l;
    l.d2 = d2 + u;
    l.id = id + u;
    l.stride = (size_t)queries;
    l.cap = cap;
    return l;
}

// the "list" of a Radius counting pass
struct NnCount {
    int cnt = 0;
    __device__ __forceinline__ void insert(double, int) { cnt++; }
};

// cells xa..xb of row (y, z), clipped: consider(point) for every point in them
template <class F>
__device__ __forceinline__ void nn_scan_cells(const GridParams &g, const unsigned *start, const Pt64 *sorted64, int z, int y,
                                              int xa, int xb, F &consider)
{
    if (z < 0 || z >= g.dim[2] || y < 0 || y >= g.dim[1]) return;
    xa = max(xa, 0); xb = min(xb, g.dim[0] - 1);
    if (xa > xb) return;
    const long long row = ((long long)z * g.dim[1] + y) * g.dim[0];
    const unsigned b = start[row + xa], e = start[row + xb + 1];
    for (unsigned j = b; j < e; j++) consider(sorted64[j]);
}

// the shell of cells at Chebyshev distance R of cell (cx, cy, cz), a cell of the grid: full x-runs on its y/z faces, two
// cells elsewhere.  CLIP (KNN, whose rings may reach far beyond the grid): only the rows the grid has -- a lone point R cells
// from the rest of a grid one cell wide in y and z would otherwise walk (2 R + 1)^2 empty rows a ring, R^3 in all (a cloud
// with one outlier some 870 cells away: of the order of 1e9 empty rows for that one query, tests/test_nn_lists.py `outlier`).
template <bool CLIP, class F>
__device__ __forceinline__ void nn_scan_shell(const GridParams &g, const unsigned *start, const Pt64 *sorted64, int cx, int cy,
                                              int cz, int R, F &consider)
{
    const int z0 = CLIP ? max(-R, -cz) : -R, z1 = CLIP ? min(R, g.dim[2] - 1 - cz) : R;
    const int y0 = CLIP ? max(-R, -cy) : -R, y1 = CLIP ? min(R, g.dim[1] - 1 - cy) : R;
    for (int dz = z0; dz <= z1; dz++)
        for (int dy = y0; dy <= y1; dy++) {
            if (max(abs(dy), abs(dz)) == R) nn_scan_cells(g, start, sorted64, cz + dz, cy + dy, cx - R, cx + R, consider);
            else {
                nn_scan_cells(g, start, sorted64, cz + dz, cy + dy, cx - R, cx - R, consider);
                nn_scan_cells(g, start, sorted64, cz + dz, cy + dy, cx + R, cx + R, consider);
            }
        }
}

// After rings 0 .. R around the query's cell: the squared distance from the query to the nearest point that may still be
// unscanned, +inf with *open = false once the whole grid has been scanned.  True for ANY query, inside its cell or clamped
// into the grid from outside: an unscanned point lies in a cell beyond one of the six faces of the scanned block, so inside
// the slab of the grid's box beyond that face (the finite coordinates of the cloud lie inside the box: grid.hip, bbox_kernel),
// and the distance from the query to a slab is that to an axis-aligned box: beyond the face along its axis, outside the
// grid's box along the other two.  Only faces with cells of the grid beyond them count.  The fp32 binning may see a point
// 1e-3 cell from where it is (kGridMaxDim), and the query of a self-search likewise: every length is taken short by
// 0.1 % of the R + 1 cells it spans.  (A point whose coordinate is not finite sits in a clamped cell outside every slab: its
// distance is infinite or NaN, and nn_search stops only on a farthest entry below the bound: a finite one.)
__device__ __forceinline__ double nn_unscanned_d2(const GridParams &g, const NnQuery &q, int R, bool *open)
{
    const double edge[3] = {(double)g.h, (double)g.hs, (double)g.hs};
    const int c[3] = {q.cx, q.cy, q.cz};
    double lo[3], hi[3], out2[3];                                   // to the two faces (-1: none beyond); outside the box, squared
    for (int a = 0; a < 3; a++) {
        const double slack = 1e-3 * (double)(R + 1) * edge[a];
        const double u = q.b[a] - (double)g.mn[a];                  // from the box's lower corner
        const double o = fmax(fmax(-u, u - (double)g.dim[a] * edge[a]) - slack, 0.0);
        out2[a] = o * o;
        lo[a] = c[a] - R > 0 ? fmax(u - (double)(c[a] - R) * edge[a] - slack, 0.0) : -1.0;
        hi[a] = c[a] + R < g.dim[a] - 1 ? fmax((double)(c[a] + R + 1) * edge[a] - u - slack, 0.0) : -1.0;
    }
    double best = INFINITY;
    *open = false;
    for (int a = 0; a < 3; a++) {
        const double rest = out2[(a + 1) % 3] + out2[(a + 2) % 3];
        if (lo[a] >= 0.0) { *open = true; best = fmin(best, lo[a] * lo[a] + rest); }
        if (hi[a] >= 0.0) { *open = true; best = fmin(best, hi[a] * hi[a] + rest); }
    }
    return best;
}

// Every point of the cells around q whose squared distance d passes accept(d) (nn_accept) goes to list.insert(d, index).
//   KNN = false  cells of edge 1.001 r: the 27 cells (rings 0 and 1) cover the radius, `accept` holds the radius test;
//                for a query clamped into the grid from outside they still do (the block only moves towards the cloud)
//   KNN = true   any cell size: rings are added until the list is full and its farthest entry lies nearer than anything
//                unscanned can (nn_unscanned_d2), or the whole grid has been scanned
// `list` needs insert and, for KNN, cnt, cap and farthest: NnList, NnHeap, or a caller's own that only counts.
template <bool KNN, class List, class Accept>
__device__ __forceinline__ void nn_search(const NnGridView &v, const NnQuery &q, List &list, Accept accept)
{
    const GridParams g = v.g;
    auto consider = [&](const Pt64 &p) {
        const double d = nn_dist2(q.p, p);
        if (accept(d)) list.insert(d, (int)p.w);
    };
    const int rmax = KNN ? max(max(g.dim[0], g.dim[1]), g.dim[2]) : 1;
    for (int R = 0; R <= rmax; R++) {
        nn_scan_shell<KNN>(g, v.start, v.sorted64, q.cx, q.cy, q.cz, R, consider);
        if constexpr (KNN) {
            bool open;
            const double beyond = nn_unscanned_d2(g, q, R, &open);
            if (!open) break;                                       // the whole grid has been scanned
            if (list.cnt == list.cap && list.farthest() < beyond) break;     // (strictly: a finite entry, and no tie left open)
        }
    }
}
#endif  // __HIPCC__

}  // namespace visma
