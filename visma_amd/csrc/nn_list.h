// nn_list.h -- the neighbour list of one query point on the radius-cell grid of grid.hip, in the order of the reference's
// KDTreeFlann result list: ascending (d2, index), flann's sum of squares in f64.  One thread per query; the list lives
// in LDS as [cap][threads] (element j of thread t at j * threads + t), squared distances first, indices behind them.
// Shared by normals.hip (KNN / Hybrid / the counting pass; its lists beyond the LDS live in a heap of its own) and
// color_gradient.hip (Hybrid).
#pragma once
#include "device_common.h"

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

#ifdef __HIPCC__
struct NnList {
    double *d2;                  // element j at d2[j * stride]
    int *id;
    size_t stride;
    int cap;
    int cnt = 0;
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

// flann L2 (dist.h:159-176): result += diff * diff over x, y, z
__device__ __forceinline__ double nn_dist2(const Pt64 &q, const Pt64 &p)
{
    const double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    double d = dx * dx;
    d += dy * dy;
    d += dz * dz;
    return d;
}

// (d, id) before entry j
__device__ __forceinline__ bool nn_list_less(const NnList &l, double d, int id, int j)
{
    const double dj = l.d2[(size_t)j * l.stride];
    return d < dj || (d == dj && id < l.id[(size_t)j * l.stride]);
}

// keep the cap nearest: insertion into the sorted list, the farthest entry dropped when it is full
__device__ __forceinline__ void nn_list_insert(NnList &l, double d, int id)
{
    int pos;
    if (l.cnt < l.cap) pos = l.cnt++;
    else if (nn_list_less(l, d, id, l.cap - 1)) pos = l.cap - 1;
    else return;
    while (pos > 0 && nn_list_less(l, d, id, pos - 1)) {
        l.d2[(size_t)pos * l.stride] = l.d2[(size_t)(pos - 1) * l.stride];
        l.id[(size_t)pos * l.stride] = l.id[(size_t)(pos - 1) * l.stride];
        pos--;
    }
    l.d2[(size_t)pos * l.stride] = d;
    l.id[(size_t)pos * l.stride] = id;
}

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

// the shell of cells at Chebyshev distance R of cell (cx, cy, cz): full x-runs on its y/z faces, two cells elsewhere
template <class F>
__device__ __forceinline__ void nn_scan_shell(const GridParams &g, const unsigned *start, const Pt64 *sorted64, int cx, int cy,
                                              int cz, int R, F &consider)
{
    for (int dz = -R; dz <= R; dz++)
        for (int dy = -R; dy <= R; dy++) {
            if (max(abs(dy), abs(dz)) == R) nn_scan_cells(g, start, sorted64, cz + dz, cy + dy, cx - R, cx + R, consider);
            else {
                nn_scan_cells(g, start, sorted64, cz + dz, cy + dy, cx - R, cx - R, consider);
                nn_scan_cells(g, start, sorted64, cz + dz, cy + dy, cx + R, cx + R, consider);
            }
        }
}
#endif  // __HIPCC__

}  // namespace visma
