// trimesh.hip -- open3d::TriangleMesh on the device (visma_icp_trimesh_*): ComputeTriangleNormals, ComputeVertexNormals,
// NormalizeNormals, the four steps of Purge, SelectDownSample, CropTriangleMesh and Transform over a mesh that stays resident
// (Core/Geometry/TriangleMesh.cpp, DownSample.cpp :107-177, :256-274; Eigen's Dot.h for normalize()).  Every result is the
// reference's bit for bit: f64, one operation per rounding (the build's -ffp-contract=off), correctly rounded sqrt and
// division, and every sum in the reference's serial order.  No floating-point atomics; one writer per output row.
//   BadIndexSource          creation: an index outside [0, nv) is counted (compact.h's count pass); no other kernel of this
//                           file reads a vertex array through an index that has not passed it, and every remap keeps that
//   tm_triangle_normals     one lane per triangle: (v1 - v0) x (v2 - v0), Eigen's component formula
//   rows_normalize          (row_kernels.h, shared with cloud.hip) n2 = (x x + y y) + z z; n2 > 0: every component / sqrt(n2); then x NaN -> (0, 0, 1)
//   tm_pairs, tm_vertex_sum ComputeVertexNormals: the 3 nt pairs (vertex, 3 t + c) in ONE stable radix sort by vertex over
//                           ceil(log2 nv) bits, segment starts by head flags and compact.h, then one lane per vertex adds its
//                           segment's triangle normals in ascending 3 t + c: the reference's order.  A vertex shared by very
//                           many triangles is summed by one lane: that is the price of that order
//   tm_vertex_key ...       RemoveDuplicatedVertices: three stable radix sorts of the indices by the 64 bits of z, y, x
//                           (-0.0 as +0.0), heads where a == comparison of the doubles fails (a NaN row is always a head),
//                           the lowest index of a group (first in it: the sorts are stable) its representative; an ordered
//                           compaction over the ORIGINAL index keeps the survivors' order
//   tm_triangle_key ...     RemoveDuplicatedTriangles: the reference's rotation with its <= ties, three stable sorts
//   tm_manifold_flag        RemoveNonManifoldTriangles;  tm_mark_corners: RemoveNonManifoldVertices and Select (lanes that
//                           mark the same vertex all store the same 1)
// The passes are streaming: grid-capped stride loops of 256 lanes (compact.h's shape).
#include "compact.h"
#include "dev_mem.h"
#include "kernels.h"
#include "row_kernels.h"

#include <hipcub/hipcub.hpp>

#include <math.h>

#include <algorithm>
#include <memory>

namespace visma {

namespace {

#define TM_LOOP(i, n) \
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < (n); i += (long long)gridDim.x * kThreads)

// ---- validation --------------------------------------------------------------------------------------------------------
struct BadIndexSource {
    const int *tri;
    int nv;
    __device__ int count(long long i) const { return (unsigned)tri[i] >= (unsigned)nv; }
    __device__ void emit(long long, long long) const {}
};

// ---- normals -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tm_triangle_normals(const double *v, const int *tri, double *tn, long long nt)
{
    TM_LOOP(t, nt) {
        const double *p0 = v + 3 * (long long)tri[3 * t], *p1 = v + 3 * (long long)tri[3 * t + 1], *p2 = v + 3 * (long long)tri[3 * t + 2];
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        tn[3 * t] = ay * bz - az * by;
        tn[3 * t + 1] = az * bx - ax * bz;
        tn[3 * t + 2] = ax * by - ay * bx;
    }
}

__global__ __launch_bounds__(kThreads) void tm_pairs(const int *tri, unsigned *key, int *val, long long n3)
{
    TM_LOOP(i, n3) { key[i] = (unsigned)tri[i]; val[i] = (int)i; }
}

// heads of the runs of equal keys: row r of the compaction is where run r starts
struct RunHeadSource {
    const unsigned *key;
    int *start;
    __device__ int count(long long i) const { return i == 0 || key[i] != key[i - 1]; }
    __device__ void emit(long long i, long long row) const { start[row] = (int)i; }
};

// one lane per vertex that a triangle uses: vn[v] (+)= the triangle normals of its run, in ascending 3 t + c
__global__ __launch_bounds__(kThreads) void tm_vertex_sum(const unsigned *key, const int *val, const int *start, long long runs, long long n3,
                                                          const double *tn, double *vn)
{
    TM_LOOP(r, runs) {
        const long long lo = start[r], hi = r + 1 < runs ? (long long)start[r + 1] : n3;
        const long long v = key[lo];
        double x = vn[3 * v], y = vn[3 * v + 1], z = vn[3 * v + 2];
        for (long long j = lo; j < hi; j++) {
            const double *n = tn + 3 * (long long)(val[j] / 3);
            x = x + n[0]; y = y + n[1]; z = z + n[2];
        }
        vn[3 * v] = x; vn[3 * v + 1] = y; vn[3 * v + 2] = z;
    }
}

// ---- sorting by key components -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tm_iota(int *idx, long long n)
{
    TM_LOOP(i, n) idx[i] = (int)i;
}

// the 64 bits of coordinate `axis` of vertex idx[i], -0.0 as +0.0
__global__ __launch_bounds__(kThreads) void tm_vertex_key(const double *v, const int *idx, int axis, unsigned long long *key, long long n)
{
    TM_LOOP(i, n) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v[3 * (long long)idx[i] + axis]);
        key[i] = b == 0x8000000000000000ull ? 0ull : b;
    }
}

__device__ __forceinline__ bool tm_same_vertex(const double *a, const double *b)
{
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2];     // (-0.0 == 0.0; a NaN equals nothing, itself included)
}

struct VertexHeadSource {
    const double *v;
    const int *idx;
    int *start;
    __device__ int count(long long i) const { return i == 0 || !tm_same_vertex(v + 3 * (long long)idx[i], v + 3 * (long long)idx[i - 1]); }
    __device__ void emit(long long i, long long row) const { start[row] = (int)i; }
};

// rep[idx[i]] = the first index of the run that holds position i (the largest start <= i, by bisection); flag: is its own
__global__ __launch_bounds__(kThreads) void tm_representative(const int *idx, const int *start, long long runs, int *rep, int *flag, long long n)
{
    TM_LOOP(i, n) {
        long long lo = 0, hi = runs - 1;                  // start[0] == 0 <= i
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if ((long long)start[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const int me = idx[i], first = idx[start[lo]];
        rep[me] = first;
        flag[me] = me == first;
    }
}

// TriangleMesh.cpp:235-251, the <= as written
__device__ __forceinline__ void tm_rotate(const int *t, int *k)
{
    if (t[0] <= t[1]) {
        if (t[0] <= t[2]) { k[0] = t[0]; k[1] = t[1]; k[2] = t[2]; }
        else { k[0] = t[2]; k[1] = t[0]; k[2] = t[1]; }
    } else {
        if (t[1] <= t[2]) { k[0] = t[1]; k[1] = t[2]; k[2] = t[0]; }
        else { k[0] = t[2]; k[1] = t[0]; k[2] = t[1]; }
    }
}

__global__ __launch_bounds__(kThreads) void tm_triangle_key(const int *tri, const int *idx, int comp, unsigned *key, long long n)
{
    TM_LOOP(i, n) {
        int k[3];
        tm_rotate(tri + 3 * (long long)idx[i], k);
        key[i] = (unsigned)k[comp];
    }
}

// flag[idx[i]] = position i opens a run of equal keys: the first occurrence (lowest index) of its key
__global__ __launch_bounds__(kThreads) void tm_triangle_first(const int *tri, const int *idx, int *flag, long long n)
{
    TM_LOOP(i, n) {
        bool head = i == 0;
        if (!head) {
            int a[3], b[3];
            tm_rotate(tri + 3 * (long long)idx[i], a);
            tm_rotate(tri + 3 * (long long)idx[i - 1], b);
            head = a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
        }
        flag[idx[i]] = head;
    }
}

__global__ __launch_bounds__(kThreads) void tm_manifold_flag(const int *tri, int *flag, long long nt)
{
    TM_LOOP(t, nt) {
        const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        flag[t] = a != b && b != c && c != a;
    }
}

// mark[corner] = 1 for every corner of a triangle whose tri_flag is set (NULL: every triangle)
__global__ __launch_bounds__(kThreads) void tm_mark_corners(const int *tri, const int *tri_flag, int *mark, long long nt)
{
    TM_LOOP(t, nt) {
        if (tri_flag && !tri_flag[t]) continue;
        for (int c = 0; c < 3; c++) mark[tri[3 * t + c]] = 1;
    }
}

__global__ __launch_bounds__(kThreads) void tm_mark_selected(const long long *indices, long long n, int *mark)
{
    TM_LOOP(i, n) mark[indices[i]] = 1;
}

// DownSample.cpp:267-269: a NaN fails every comparison, in the vertex and in the bound
struct Box { double lo[3], hi[3]; };
__global__ __launch_bounds__(kThreads) void tm_mark_inside(const double *v, long long nv, Box b, int *mark)
{
    TM_LOOP(i, nv) {
        const double *p = v + 3 * i;
        mark[i] = p[0] >= b.lo[0] && p[0] <= b.hi[0] && p[1] >= b.lo[1] && p[1] <= b.hi[1] && p[2] >= b.lo[2] && p[2] <= b.hi[2];
    }
}

__global__ __launch_bounds__(kThreads) void tm_all_selected(const int *tri, const int *mark, int *flag, long long nt)
{
    TM_LOOP(t, nt) flag[t] = mark[tri[3 * t]] && mark[tri[3 * t + 1]] && mark[tri[3 * t + 2]];
}

__global__ __launch_bounds__(kThreads) void tm_remap(int *tri, const int *rep, const int *new_index, long long n3)
{
    TM_LOOP(i, n3) {
        const int v = rep ? rep[tri[i]] : tri[i];
        tri[i] = new_index[v];
    }
}

// ---- the ordered compactions (compact.h) ---------------------------------------------------------------------------------
struct VertexCompact {
    const int *flag;
    const double *v, *vn, *vc;
    double *ov, *ovn, *ovc;
    int *new_index;
    __device__ int count(long long i) const { return flag[i] != 0; }
    __device__ void emit(long long i, long long row) const
    {
        for (int k = 0; k < 3; k++) ov[3 * row + k] = v[3 * i + k];
        if (vn) for (int k = 0; k < 3; k++) ovn[3 * row + k] = vn[3 * i + k];
        if (vc) for (int k = 0; k < 3; k++) ovc[3 * row + k] = vc[3 * i + k];
        new_index[i] = (int)row;
    }
};

struct TriangleCompact {
    const int *flag;
    const int *tri;
    const double *tn;
    const int *remap;                // NULL: the indices as they are
    int *otri;
    double *otn;
    __device__ int count(long long i) const { return flag[i] != 0; }
    __device__ void emit(long long i, long long row) const
    {
        for (int k = 0; k < 3; k++) otri[3 * row + k] = remap ? remap[tri[3 * i + k]] : tri[3 * i + k];
        if (tn) for (int k = 0; k < 3; k++) otn[3 * row + k] = tn[3 * i + k];
    }
};


int bits_for(long long n)            // the bits that hold 0 .. n - 1, at least one
{
    int b = 1;
    while ((1ll << b) < n) b++;
    return b;
}

}  // namespace

struct TriMeshDevice {
    int64_t nv = 0, nt = 0;
    bool has_vn = false, has_vc = false, has_tn = false;     // the reference's HasVertexNormals() ...: never set on no rows
    DeviceBuf<double> v, vn, vc, tn;
    DeviceBuf<int> tri;
    // what a call works in: grow-only
    Compactor comp;
    DeviceBuf<unsigned long long> k64a, k64b;
    DeviceBuf<unsigned> k32a, k32b;
    DeviceBuf<int> ia, ib, start, rep, flag, tflag, map;
    DeviceBuf<long long> sel;
    DeviceBuf<char> tmp;
};

namespace {

// a stable sort of (key, val) by the low `bits` of key; the sorted rows land in (kout, vout)
template <class K>
hipError_t sort_pairs(TriMeshDevice *M, K *kin, K *kout, int *vin, int *vout, long long n, int bits, hipStream_t stream)
{
    size_t bytes = 0;
    VISMA_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, kin, kout, vin, vout, (int)n, 0, bits, stream));
    DEV_RESERVE(M->tmp, bytes);
    return hipcub::DeviceRadixSort::SortPairs((void *)M->tmp.get(), bytes, kin, kout, vin, vout, (int)n, 0, bits, stream);
}

hipError_t validate(TriMeshDevice *M, hipStream_t stream)
{
    BadIndexSource s{M->tri.get(), (int)M->nv};
    long long bad = 0;
    VISMA_TRY(compact_count(M->comp, s, 3 * M->nt, stream, &bad));
    return bad == 0 ? hipSuccess : hipErrorInvalidValue;
}

void set_flags(TriMeshDevice *M, bool vn, bool vc, bool tn)
{
    M->has_vn = vn && M->nv > 0;
    M->has_vc = vc && M->nv > 0;
    M->has_tn = tn && M->nv > 0 && M->nt > 0;
}

// S's vertices with flag != 0, in order, into O (which may be S); S's scratch `map` receives the new index of every kept one
hipError_t compact_vertices(TriMeshDevice *S, TriMeshDevice *O, const int *flag, hipStream_t stream)
{
    VertexCompact c{flag, S->v.get(), S->has_vn ? S->vn.get() : nullptr, S->has_vc ? S->vc.get() : nullptr, nullptr, nullptr, nullptr, nullptr};
    long long rows = 0;
    VISMA_TRY(compact_count(S->comp, c, S->nv, stream, &rows));
    DeviceBuf<double> ov, ovn, ovc;
    DEV_RESET(ov, 3 * (size_t)rows);
    if (c.vn) DEV_RESET(ovn, 3 * (size_t)rows);
    if (c.vc) DEV_RESET(ovc, 3 * (size_t)rows);
    DEV_RESERVE(S->map, (size_t)std::max<int64_t>(S->nv, 1));
    VISMA_TRY(hipMemsetAsync(S->map.get(), 0, sizeof(int) * (size_t)std::max<int64_t>(S->nv, 1), stream));
    c.ov = ov.get(); c.ovn = ovn.get(); c.ovc = ovc.get(); c.new_index = S->map.get();
    VISMA_TRY(compact_write(S->comp, c, S->nv, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    const bool vn = c.vn != nullptr, vc = c.vc != nullptr;
    O->v = std::move(ov); O->vn = std::move(ovn); O->vc = std::move(ovc);
    O->nv = rows;
    O->has_vn = vn && rows > 0; O->has_vc = vc && rows > 0;
    if (rows == 0) O->has_tn = false;
    return hipSuccess;
}

// S's triangles with flag != 0, in order, into O (which may be S), their indices through remap where given
hipError_t compact_triangles(TriMeshDevice *S, TriMeshDevice *O, const int *flag, const int *remap, hipStream_t stream)
{
    TriangleCompact c{flag, S->tri.get(), S->has_tn ? S->tn.get() : nullptr, remap, nullptr, nullptr};
    long long rows = 0;
    VISMA_TRY(compact_count(S->comp, c, S->nt, stream, &rows));
    DeviceBuf<int> otri;
    DeviceBuf<double> otn;
    DEV_RESET(otri, 3 * (size_t)rows);
    if (c.tn) DEV_RESET(otn, 3 * (size_t)rows);
    c.otri = otri.get(); c.otn = otn.get();
    VISMA_TRY(compact_write(S->comp, c, S->nt, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    const bool tn = c.tn != nullptr;
    O->tri = std::move(otri); O->tn = std::move(otn);
    O->nt = rows;
    O->has_tn = tn && rows > 0 && O->nv > 0;
    return hipSuccess;
}

hipError_t remove_duplicated_vertices(TriMeshDevice *M, hipStream_t stream, int64_t *removed)
{
    const long long n = M->nv;
    *removed = 0;
    if (n == 0) return hipSuccess;
    const unsigned g = capped_blocks(n);
    DEV_RESERVE(M->ia, (size_t)n); DEV_RESERVE(M->ib, (size_t)n);
    DEV_RESERVE(M->k64a, (size_t)n); DEV_RESERVE(M->k64b, (size_t)n);
    DEV_RESERVE(M->start, (size_t)n); DEV_RESERVE(M->rep, (size_t)n); DEV_RESERVE(M->flag, (size_t)n);
    int *cur = M->ia.get(), *nxt = M->ib.get();
    tm_iota<<<g, kThreads, 0, stream>>>(cur, n);
    for (int axis = 2; axis >= 0; axis--) {                  // least significant first: z, then y, then x
        tm_vertex_key<<<g, kThreads, 0, stream>>>(M->v.get(), cur, axis, M->k64a.get(), n);
        VISMA_TRY(hipGetLastError());
        VISMA_TRY(sort_pairs(M, M->k64a.get(), M->k64b.get(), cur, nxt, n, 64, stream));
        std::swap(cur, nxt);
    }
    VertexHeadSource h{M->v.get(), cur, M->start.get()};
    long long runs = 0;
    VISMA_TRY(compact_count(M->comp, h, n, stream, &runs));
    VISMA_TRY(compact_write(M->comp, h, n, stream));
    tm_representative<<<g, kThreads, 0, stream>>>(cur, M->start.get(), runs, M->rep.get(), M->flag.get(), n);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(compact_vertices(M, M, M->flag.get(), stream));
    if (M->nt > 0) {
        tm_remap<<<capped_blocks(3 * M->nt), kThreads, 0, stream>>>(M->tri.get(), M->rep.get(), M->map.get(), 3 * M->nt);
        VISMA_TRY(hipGetLastError());
        VISMA_TRY(hipStreamSynchronize(stream));
    }
    *removed = n - M->nv;
    return hipSuccess;
}

hipError_t remove_duplicated_triangles(TriMeshDevice *M, hipStream_t stream, int64_t *removed)
{
    const long long n = M->nt;
    *removed = 0;
    if (n == 0) return hipSuccess;
    const unsigned g = capped_blocks(n);
    DEV_RESERVE(M->ia, (size_t)n); DEV_RESERVE(M->ib, (size_t)n);
    DEV_RESERVE(M->k32a, (size_t)n); DEV_RESERVE(M->k32b, (size_t)n);
    DEV_RESERVE(M->tflag, (size_t)n);
    int *cur = M->ia.get(), *nxt = M->ib.get();
    const int bits = bits_for(M->nv);
    tm_iota<<<g, kThreads, 0, stream>>>(cur, n);
    for (int comp = 2; comp >= 0; comp--) {
        tm_triangle_key<<<g, kThreads, 0, stream>>>(M->tri.get(), cur, comp, M->k32a.get(), n);
        VISMA_TRY(hipGetLastError());
        VISMA_TRY(sort_pairs(M, M->k32a.get(), M->k32b.get(), cur, nxt, n, bits, stream));
        std::swap(cur, nxt);
    }
    tm_triangle_first<<<g, kThreads, 0, stream>>>(M->tri.get(), cur, M->tflag.get(), n);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(compact_triangles(M, M, M->tflag.get(), nullptr, stream));
    *removed = n - M->nt;
    return hipSuccess;
}

hipError_t remove_non_manifold_triangles(TriMeshDevice *M, hipStream_t stream, int64_t *removed)
{
    const long long n = M->nt;
    *removed = 0;
    if (n == 0) return hipSuccess;
    DEV_RESERVE(M->tflag, (size_t)n);
    tm_manifold_flag<<<capped_blocks(n), kThreads, 0, stream>>>(M->tri.get(), M->tflag.get(), n);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(compact_triangles(M, M, M->tflag.get(), nullptr, stream));
    *removed = n - M->nt;
    return hipSuccess;
}

hipError_t remove_non_manifold_vertices(TriMeshDevice *M, hipStream_t stream, int64_t *removed)
{
    const long long n = M->nv;
    *removed = 0;
    if (n == 0) return hipSuccess;
    DEV_RESERVE(M->flag, (size_t)n);
    VISMA_TRY(hipMemsetAsync(M->flag.get(), 0, sizeof(int) * (size_t)n, stream));
    if (M->nt > 0) {
        tm_mark_corners<<<capped_blocks(M->nt), kThreads, 0, stream>>>(M->tri.get(), nullptr, M->flag.get(), M->nt);
        VISMA_TRY(hipGetLastError());
    }
    VISMA_TRY(compact_vertices(M, M, M->flag.get(), stream));
    if (M->nt > 0) {
        tm_remap<<<capped_blocks(3 * M->nt), kThreads, 0, stream>>>(M->tri.get(), nullptr, M->map.get(), 3 * M->nt);
        VISMA_TRY(hipGetLastError());
        VISMA_TRY(hipStreamSynchronize(stream));
    }
    *removed = n - M->nv;
    return hipSuccess;
}

// DownSample.cpp:107-177 behind the marks in S->flag: the triangles whose three corners are marked, the vertices they use
hipError_t select_marked(TriMeshDevice *S, hipStream_t stream, TriMeshDevice *O)
{
    if (S->nv == 0) return hipSuccess;
    DEV_RESERVE(S->rep, (size_t)S->nv);                       // (here: the vertices a surviving triangle uses)
    VISMA_TRY(hipMemsetAsync(S->rep.get(), 0, sizeof(int) * (size_t)S->nv, stream));
    if (S->nt > 0) {
        DEV_RESERVE(S->tflag, (size_t)S->nt);
        const unsigned g = capped_blocks(S->nt);
        tm_all_selected<<<g, kThreads, 0, stream>>>(S->tri.get(), S->flag.get(), S->tflag.get(), S->nt);
        tm_mark_corners<<<g, kThreads, 0, stream>>>(S->tri.get(), S->tflag.get(), S->rep.get(), S->nt);
        VISMA_TRY(hipGetLastError());
    }
    VISMA_TRY(compact_vertices(S, O, S->rep.get(), stream));
    if (S->nt > 0) VISMA_TRY(compact_triangles(S, O, S->tflag.get(), S->map.get(), stream));
    int64_t removed[4];
    return trimesh_device_purge(O, removed, stream);
}

}  // namespace

void trimesh_device_destroy(TriMeshDevice *M) { delete M; }

hipError_t trimesh_device_create(const double *h_v, int64_t nv, const double *h_vn, const double *h_vc, const int32_t *h_tri, int64_t nt,
                                 const double *h_tn, bool on_device, hipStream_t stream, TriMeshDevice **out)
{
    *out = nullptr;
    std::unique_ptr<TriMeshDevice> M(new TriMeshDevice);
    M->nv = nv; M->nt = nt;
    if (nv == 0 && nt > 0) return hipErrorInvalidValue;      // (no index can be in [0, 0))
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t vb = sizeof(double) * 3 * (size_t)nv, tb = sizeof(double) * 3 * (size_t)nt;
    set_flags(M.get(), h_vn != nullptr, h_vc != nullptr, h_tn != nullptr);
    if (nv > 0) {
        DEV_RESET(M->v, 3 * (size_t)nv);
        VISMA_TRY(hipMemcpyAsync(M->v.get(), h_v, vb, kind, stream));
        if (M->has_vn) { DEV_RESET(M->vn, 3 * (size_t)nv); VISMA_TRY(hipMemcpyAsync(M->vn.get(), h_vn, vb, kind, stream)); }
        if (M->has_vc) { DEV_RESET(M->vc, 3 * (size_t)nv); VISMA_TRY(hipMemcpyAsync(M->vc.get(), h_vc, vb, kind, stream)); }
    }
    if (nt > 0) {
        DEV_RESET(M->tri, 3 * (size_t)nt);
        VISMA_TRY(hipMemcpyAsync(M->tri.get(), h_tri, sizeof(int32_t) * 3 * (size_t)nt, kind, stream));
        if (M->has_tn) { DEV_RESET(M->tn, 3 * (size_t)nt); VISMA_TRY(hipMemcpyAsync(M->tn.get(), h_tn, tb, kind, stream)); }
        VISMA_TRY(validate(M.get(), stream));
    }
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = M.release();
    return hipSuccess;
}

void trimesh_device_size(const TriMeshDevice *M, int64_t *nv, int64_t *nt, int *flags)
{
    *nv = M->nv; *nt = M->nt;
    *flags = (M->has_vn ? kTriMeshVertexNormals : 0) | (M->has_vc ? kTriMeshVertexColors : 0) | (M->has_tn ? kTriMeshTriangleNormals : 0);
}

void trimesh_device_arrays(const TriMeshDevice *M, int64_t *nv, int64_t *nt, const double **v, const int **tri)
{
    *nv = M->nv; *nt = M->nt; *v = M->v.get(); *tri = M->tri.get();
}

hipError_t trimesh_device_get(TriMeshDevice *M, double *v, double *vn, double *vc, int32_t *tri, double *tn, hipStream_t stream)
{
    const size_t vb = sizeof(double) * 3 * (size_t)M->nv, tb = sizeof(double) * 3 * (size_t)M->nt;
    if (M->nv > 0) {
        if (v) VISMA_TRY(hipMemcpyAsync(v, M->v.get(), vb, hipMemcpyDeviceToHost, stream));
        if (vn && M->has_vn) VISMA_TRY(hipMemcpyAsync(vn, M->vn.get(), vb, hipMemcpyDeviceToHost, stream));
        if (vc && M->has_vc) VISMA_TRY(hipMemcpyAsync(vc, M->vc.get(), vb, hipMemcpyDeviceToHost, stream));
    }
    if (M->nt > 0) {
        if (tri) VISMA_TRY(hipMemcpyAsync(tri, M->tri.get(), sizeof(int32_t) * 3 * (size_t)M->nt, hipMemcpyDeviceToHost, stream));
        if (tn && M->has_tn) VISMA_TRY(hipMemcpyAsync(tn, M->tn.get(), tb, hipMemcpyDeviceToHost, stream));
    }
    return hipStreamSynchronize(stream);
}

hipError_t trimesh_device_normalize_normals(TriMeshDevice *M, hipStream_t stream)
{
    if (M->has_vn) rows_normalize<<<capped_blocks(M->nv), kThreads, 0, stream>>>(M->vn.get(), M->nv, true);
    if (M->has_tn) rows_normalize<<<capped_blocks(M->nt), kThreads, 0, stream>>>(M->tn.get(), M->nt, true);
    VISMA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

hipError_t trimesh_device_compute_triangle_normals(TriMeshDevice *M, bool normalized, hipStream_t stream)
{
    if (M->nt > 0) {
        DEV_RESERVE(M->tn, 3 * (size_t)M->nt);
        tm_triangle_normals<<<capped_blocks(M->nt), kThreads, 0, stream>>>(M->v.get(), M->tri.get(), M->tn.get(), M->nt);
        VISMA_TRY(hipGetLastError());
        M->has_tn = true;
    }
    if (normalized) return trimesh_device_normalize_normals(M, stream);
    return hipStreamSynchronize(stream);
}

hipError_t trimesh_device_compute_vertex_normals(TriMeshDevice *M, bool normalized, hipStream_t stream)
{
    if (!M->has_tn) VISMA_TRY(trimesh_device_compute_triangle_normals(M, false, stream));
    if (M->nv > 0 && !M->has_vn) {                            // resize(n, Zero): rows that exist keep their values
        DEV_RESERVE(M->vn, 3 * (size_t)M->nv);
        VISMA_TRY(hipMemsetAsync(M->vn.get(), 0, sizeof(double) * 3 * (size_t)M->nv, stream));
        M->has_vn = true;
    }
    const long long n3 = 3 * M->nt;
    if (n3 > 0) {
        DEV_RESERVE(M->k32a, (size_t)n3); DEV_RESERVE(M->k32b, (size_t)n3);
        DEV_RESERVE(M->ia, (size_t)n3); DEV_RESERVE(M->ib, (size_t)n3);
        DEV_RESERVE(M->start, (size_t)n3);
        tm_pairs<<<capped_blocks(n3), kThreads, 0, stream>>>(M->tri.get(), M->k32a.get(), M->ia.get(), n3);
        VISMA_TRY(hipGetLastError());
        VISMA_TRY(sort_pairs(M, M->k32a.get(), M->k32b.get(), M->ia.get(), M->ib.get(), n3, bits_for(M->nv), stream));
        RunHeadSource h{M->k32b.get(), M->start.get()};
        long long runs = 0;
        VISMA_TRY(compact_count(M->comp, h, n3, stream, &runs));
        VISMA_TRY(compact_write(M->comp, h, n3, stream));
        tm_vertex_sum<<<capped_blocks(runs), kThreads, 0, stream>>>(M->k32b.get(), M->ib.get(), M->start.get(), runs, n3, M->tn.get(), M->vn.get());
        VISMA_TRY(hipGetLastError());
    }
    if (normalized) return trimesh_device_normalize_normals(M, stream);
    return hipStreamSynchronize(stream);
}

hipError_t trimesh_device_remove(TriMeshDevice *M, int step, int64_t *removed, hipStream_t stream)
{
    switch (step) {
    case 0: return remove_duplicated_vertices(M, stream, removed);
    case 1: return remove_duplicated_triangles(M, stream, removed);
    case 2: return remove_non_manifold_triangles(M, stream, removed);
    case 3: return remove_non_manifold_vertices(M, stream, removed);
    }
    return hipErrorInvalidValue;
}

hipError_t trimesh_device_purge(TriMeshDevice *M, int64_t removed[4], hipStream_t stream)
{
    for (int step = 0; step < 4; step++) VISMA_TRY(trimesh_device_remove(M, step, &removed[step], stream));
    return hipSuccess;
}

hipError_t trimesh_device_select(TriMeshDevice *S, const int64_t *h_indices, int64_t n, hipStream_t stream, TriMeshDevice **out)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "the indices are uploaded as they are");
    *out = nullptr;
    for (int64_t i = 0; i < n; i++)
        if (h_indices[i] < 0 || h_indices[i] >= S->nv) return hipErrorInvalidValue;   // (the reference reads out of bounds)
    std::unique_ptr<TriMeshDevice> O(new TriMeshDevice);
    if (S->nv > 0) {
        DEV_RESERVE(S->flag, (size_t)S->nv);
        VISMA_TRY(hipMemsetAsync(S->flag.get(), 0, sizeof(int) * (size_t)S->nv, stream));
        if (n > 0) {
            DEV_RESERVE(S->sel, (size_t)n);
            VISMA_TRY(hipMemcpyAsync(S->sel.get(), h_indices, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, stream));
            tm_mark_selected<<<capped_blocks(n), kThreads, 0, stream>>>(S->sel.get(), n, S->flag.get());
            VISMA_TRY(hipGetLastError());
        }
        VISMA_TRY(select_marked(S, stream, O.get()));
    }
    *out = O.release();
    return hipSuccess;
}

hipError_t trimesh_device_crop(TriMeshDevice *S, const double lo[3], const double hi[3], hipStream_t stream, TriMeshDevice **out)
{
    *out = nullptr;
    std::unique_ptr<TriMeshDevice> O(new TriMeshDevice);
    const bool illegal = lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2];   // DownSample.cpp:259-263: an empty mesh
    if (!illegal && S->nv > 0) {
        DEV_RESERVE(S->flag, (size_t)S->nv);
        Box b;
        for (int k = 0; k < 3; k++) { b.lo[k] = lo[k]; b.hi[k] = hi[k]; }
        tm_mark_inside<<<capped_blocks(S->nv), kThreads, 0, stream>>>(S->v.get(), S->nv, b, S->flag.get());
        VISMA_TRY(hipGetLastError());
        VISMA_TRY(select_marked(S, stream, O.get()));
    }
    *out = O.release();
    return hipSuccess;
}

hipError_t trimesh_device_transform(TriMeshDevice *M, const double T[16], hipStream_t stream)
{
    const Mat34 m(T);
    if (M->nv > 0) rows_transform<<<capped_blocks(M->nv), kThreads, 0, stream>>>(M->v.get(), M->nv, m, 1.0);
    if (M->has_vn) rows_transform<<<capped_blocks(M->nv), kThreads, 0, stream>>>(M->vn.get(), M->nv, m, 0.0);
    if (M->has_tn) rows_transform<<<capped_blocks(M->nt), kThreads, 0, stream>>>(M->tn.get(), M->nt, m, 0.0);
    VISMA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

}  // namespace visma
