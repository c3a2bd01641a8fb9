// normals.hip -- open3d::EstimateNormals on the GPU
// (O3D/Core/Geometry/EstimateNormals.cpp:38-163; declared O3D/Core/Geometry/PointCloud.h:140-146):
// the step a caller needs before the point-to-plane estimator when its clouds carry no normals
// (Registration.cpp:152-157 refuses to run without them).
//
// Per point: neighbours by one of the three KDTreeFlann searches (KDTreeFlann.cpp:114-189) --
//   KNN     the knn nearest points (the point itself included), ascending distance,
//   Radius  every point with d2 < (double)(float)(r*r)  (flann radiusSearch, strict),
//   Hybrid  the max_nn nearest of those --
// then the covariance of the neighbours from their first and second moments summed in the order of
// the result list (EstimateNormals.cpp:86-112), the eigenvector of its smallest eigenvalue by the
// closed form of FastEigen3x3 (:40-83), (0,0,1) when fewer than 3 neighbours or a zero vector,
// and the sign of an existing normal kept (:133-146).  All f64, flann's sum of squares.
//
// The search runs on the radius-cell grid of grid.hip: cells of edge 1.001 r (Radius / Hybrid: the
// 27 cells cover the radius), or of about the distance to the knn-th neighbour (KNN: rings of cells
// are added until the knn-th distance is covered -- exact for any cell size).  One thread per
// point, in cell order; the result list (d2, index) lives in LDS, sorted by (d2, index) -- the
// reference's order up to exactly equal distances, which flann orders by tree traversal.  Lists longer than
// kNormalsMaxList entries (the LDS capacity at 64 threads) live in global memory as a max-heap per point that is
// heap-sorted at the end: any knn / max_nn.  Radius searches (no bound on the list) first COUNT every point's
// neighbours, then run as a Hybrid search whose max_nn is the largest count: the moments are summed in list order
// like the reference's (round 2 summed them in scan order: 3e-7 off where two eigenvalues nearly coincide).
// The grid of the cloud and the tuning of its cells are nn_grid.hip's, the walk over the cells and both kinds of list
// nn_list.h's, as is the rule which distances enter a list (shared with color_gradient.hip and fpfh.hip: a neighbour at a
// NaN distance is never listed); the counting pass, the runs and the slabs of heaps are this file's.
#include "nn_list.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace visma {

namespace {

struct NormalArgs {
    NnGridView view;
    const double *nrm_in;        // n x 3 or NULL
    double *nrm_out;             // n x 3
    int n;
    int cap;                     // list capacity (knn / max_nn); unused for Radius
    double r2d;                  // (double)(float)(r * r); unused for KNN
    int *count_out;              // (counting pass) neighbours within the radius, per point in cell order
    double *spill_d2;            // (spilled lists) [cap][q_count] squared distances ...
    int *spill_id;               // ... and indices, one max-heap per query of the slab
    int q_begin, q_count;        // the slab of queries (cell order) this launch works on
};

__device__ __forceinline__ double sqr(double x) { return x * x; }

// EstimateNormals.cpp:40-83.  A symmetric; returns false for a zero vector.
__device__ bool fast_eigen_3x3(const double A[3][3], double out[3])
{
    const double p1 = sqr(A[0][1]) + sqr(A[0][2]) + sqr(A[1][2]);
    double ev0, ev1, ev2;
    const double trace = A[0][0] + A[1][1] + A[2][2];
    if (p1 == 0.0) {
        ev2 = fmin(A[0][0], fmin(A[1][1], A[2][2]));
        ev0 = fmax(A[0][0], fmax(A[1][1], A[2][2]));
        ev1 = trace - ev0 - ev2;
    } else {
        const double q = trace / 3.0;
        const double p2 = sqr(A[0][0] - q) + sqr(A[1][1] - q) + sqr(A[2][2] - q) + 2 * p1;
        const double p = sqrt(p2 / 6.0);
        const double ip = 1.0 / p;
        double B[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) B[i][j] = ip * (A[i][j] - (i == j ? q : 0.0));
        // Eigen's 3x3 determinant (Determinant.h: bruteforce_det3_helper)
        const double det = B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1]) -
                           B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0]) +
                           B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0]);
        const double r = det / 2.0;
        double phi;
        if (r <= -1) phi = M_PI / 3.0;
        else if (r >= 1) phi = 0.0;
        else phi = acos(r) / 3.0;
        ev0 = q + 2.0 * p * cos(phi);
        ev2 = q + 2.0 * p * cos(phi + 2.0 * M_PI / 3.0);
        ev1 = q * 3.0 - ev0 - ev2;
    }
    (void)ev2;
    // (A - I ev0) * (A.col(0) - (ev1, 0, 0))
    const double v[3] = {A[0][0] - ev1, A[1][0], A[2][0]};
    double e[3];
    for (int i = 0; i < 3; i++) {
        const double m0 = A[i][0] - (i == 0 ? ev0 : 0.0), m1 = A[i][1] - (i == 1 ? ev0 : 0.0),
                     m2 = A[i][2] - (i == 2 ? ev0 : 0.0);
        e[i] = m0 * v[0] + m1 * v[1] + m2 * v[2];
    }
    const double len = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    if (len == 0.0) return false;
    out[0] = e[0] / len; out[1] = e[1] / len; out[2] = e[2] / len;
    return true;
}

// the normal of point `me` from its list in the reference's order (EstimateNormals.cpp:86-149)
__device__ __forceinline__ void normal_from_list(const NormalArgs &a, int me, const NnEntries &L)
{
    double nrm[3] = {0.0, 0.0, 1.0};                                // fewer than 3 neighbours (:147-149)
    if (L.cnt >= 3) {
        double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < L.cnt; j++) {
            // EstimateNormals.cpp:95-105
            const Pt64 p = a.view.pts[L.id[(size_t)j * L.stride]];
            const double x = p.x, y = p.y, z = p.z;
            c[0] += x; c[1] += y; c[2] += z;
            c[3] += x * x; c[4] += x * y; c[5] += x * z;
            c[6] += y * y; c[7] += y * z; c[8] += z * z;
        }
        const double inv = (double)L.cnt;
        for (int k = 0; k < 9; k++) c[k] /= inv;
        double A[3][3];
        A[0][0] = c[3] - c[0] * c[0];
        A[1][1] = c[6] - c[1] * c[1];
        A[2][2] = c[8] - c[2] * c[2];
        A[0][1] = A[1][0] = c[4] - c[0] * c[1];
        A[0][2] = A[2][0] = c[5] - c[0] * c[2];
        A[1][2] = A[2][1] = c[7] - c[1] * c[2];
        const bool ok = fast_eigen_3x3(A, nrm);
        if (!ok) {
            if (a.nrm_in) { nrm[0] = a.nrm_in[3ll * me]; nrm[1] = a.nrm_in[3ll * me + 1]; nrm[2] = a.nrm_in[3ll * me + 2]; }
            else { nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 1.0; }
        }
        if (a.nrm_in) {
            const double dot = nrm[0] * a.nrm_in[3ll * me] + nrm[1] * a.nrm_in[3ll * me + 1] + nrm[2] * a.nrm_in[3ll * me + 2];
            if (dot < 0.0) { nrm[0] *= -1.0; nrm[1] *= -1.0; nrm[2] *= -1.0; }
        }
    }
    a.nrm_out[3ll * me] = nrm[0];
    a.nrm_out[3ll * me + 1] = nrm[1];
    a.nrm_out[3ll * me + 2] = nrm[2];
}

// TYPE: 0 KNN, 1 Radius (counting pass only), 2 Hybrid.  COUNT: only count the neighbours within the radius.  SPILL: the
// list is a max-heap in global memory instead of a sorted array in LDS.
template <int TYPE, int NTH, bool COUNT, bool SPILL>
__global__ __launch_bounds__(NTH) void estimate_normals_kernel(NormalArgs a)
{
    extern __shared__ double lds_raw[];
    const long long u = (long long)blockIdx.x * NTH + threadIdx.x;  // query of the slab
    if (u >= a.q_count) return;
    const long long t = a.q_begin + u;
    const NnQuery q = nn_query(a.view, t);                          // queries in cell order
    // nn_list.h's rule: a neighbour at a NaN distance is never listed.  A point with a NaN coordinate is then nobody's
    // neighbour and its own list is empty: the fall-back normal
    const auto accept = nn_accept<TYPE == 0>(a.r2d);
    if constexpr (COUNT) {
        NnCount L;
        nn_search<false>(a.view, q, L, accept);
        a.count_out[t] = L.cnt;
    } else if constexpr (SPILL) {
        NnHeap L = nn_heap_global(a.spill_d2, a.spill_id, u, a.q_count, a.cap);
        nn_search<TYPE == 0>(a.view, q, L, accept);
        if (L.cnt >= 3) L.sort();
        normal_from_list(a, q.me, L);
    } else {
        NnList L = nn_list_lds(lds_raw, threadIdx.x, NTH, a.cap);
        nn_search<TYPE == 0>(a.view, q, L, accept);
        normal_from_list(a, q.me, L);
    }
}

template <int TYPE, bool COUNT, bool SPILL>
hipError_t launch_normals(const NormalArgs &a, hipStream_t stream)
{
    // only lists in LDS size the workgroup
    return nn_launch((COUNT || SPILL) ? 0 : a.cap, a.q_count, a, stream,
                     [](auto nth) { return &estimate_normals_kernel<TYPE, decltype(nth)::value, COUNT, SPILL>; });
}

}  // namespace

bool estimate_normals_trivial(int search_type, int knn, double radius)
{
    // fewer than 3 neighbours for every point (KDTreeFlann.cpp:121-126,171-176 return -1 / k < 3)
    return (search_type != 1 && knn < 3) || (search_type != 0 && !(radius > 0.0));
}

// The device part: n > 0 resident points (d_nrm_in or NULL) -> d_out, binned from `origin` (nn_binning_origin's point).
// Not for the trivial case.  Returns with the stream idle.
hipError_t estimate_normals_core(const double *d_xyz, int64_t n, const double *d_nin, const double origin[3], int search_type,
                                 int knn, double radius, double *d_out, hipStream_t stream)
{
    if (search_type < 0 || search_type > 2 || n > 0x7fffffff) return hipErrorInvalidValue;
    const bool use_r = search_type != 0;
    int cap = search_type == 1 ? 1 : (int)std::min<int64_t>(knn, n);           // (Radius: set from the counting pass)
    NnGrid G;
    DevBufs B;
    VISMA_TRY(G.alloc(n));
    ColorGradientInput in;
    in.xyz = d_xyz; in.n = n;
    for (int k = 0; k < 3; k++) in.origin[k] = origin[k];
    VISMA_TRY(G.build(in, nullptr, radius, use_r ? 0 : cap, stream));
    NormalArgs a{};
    a.view = G.view;
    a.nrm_in = d_nin; a.nrm_out = d_out; a.n = (int)n; a.cap = cap;
    a.q_begin = 0; a.q_count = (int)n;
    a.r2d = nn_radius2(radius);
    int type = search_type;
    std::vector<int> cnt;                                        // (Radius) neighbours per query, cell order
    if (search_type == 1) {
        // Radius: count every point's neighbours, then run as a Hybrid search that keeps them all
        int *d_cnt = nullptr;
        VISMA_TRY(B.alloc(&d_cnt, (size_t)n));
        a.count_out = d_cnt;
        VISMA_TRY((launch_normals<1, true, false>(a, stream)));
        cnt.resize((size_t)n);
        VISMA_TRY(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, stream));
        VISMA_TRY(hipStreamSynchronize(stream));
        type = 2;
    }
    // Runs of queries (cell order) and the list capacity each needs.  KNN / Hybrid: one run, the caller's bound.
    // Radius: the capacity of a run is the largest count AMONG ITS OWN queries (one dense corner of a scan
    // used to give every query of the cloud a list -- and, beyond the LDS, a global-memory heap -- of that corner's
    // length); runs of kSlab queries, neighbouring runs whose lists fit the LDS merged into one launch.
    struct Run { int64_t q0, qn; int cap; };
    std::vector<Run> runs;
    if (search_type == 1) {
        const int64_t kSlab = 16384;
        for (int64_t q0 = 0; q0 < n; q0 += kSlab) {
            const int64_t qn = std::min<int64_t>(kSlab, n - q0);
            const int c = std::max(1, *std::max_element(cnt.begin() + q0, cnt.begin() + q0 + qn));
            if (!runs.empty() && c <= kNormalsMaxList && runs.back().cap <= kNormalsMaxList) {
                runs.back().qn += qn;
                runs.back().cap = std::max(runs.back().cap, c);
            } else {
                runs.push_back(Run{q0, qn, c});
            }
        }
    } else {
        runs.push_back(Run{0, n, cap});
    }
    // lists longer than the LDS holds: one max-heap per query in global memory, a slab of queries at a time; the
    // slab's heaps take at most 1 GiB or half of what the device has free
    size_t budget = (size_t)1 << 30;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, free_b / 2);
    }
    size_t spill_entries = 0;
    for (Run &r : runs)
        if (r.cap > kNormalsMaxList) {
            if ((size_t)r.cap * 12 * 64 > budget) return hipErrorOutOfMemory;   // (64 queries' heaps do not fit)
            const int64_t slab = std::min<int64_t>(r.qn, std::max<int64_t>(64, (int64_t)(budget / ((size_t)r.cap * 12))));
            spill_entries = std::max(spill_entries, (size_t)r.cap * (size_t)slab);
        }
    double *d_sd = nullptr;
    int *d_si = nullptr;
    if (spill_entries) {
        VISMA_TRY(B.alloc(&d_sd, spill_entries));
        VISMA_TRY(B.alloc(&d_si, spill_entries));
        a.spill_d2 = d_sd; a.spill_id = d_si;
    }
    for (const Run &r : runs) {
        a.cap = r.cap;
        if (r.cap <= kNormalsMaxList) {
            a.q_begin = (int)r.q0;
            a.q_count = (int)r.qn;
            if (type == 0) VISMA_TRY((launch_normals<0, false, false>(a, stream)));
            else VISMA_TRY((launch_normals<2, false, false>(a, stream)));
            continue;
        }
        const int64_t slab = std::min<int64_t>(r.qn, std::max<int64_t>(64, (int64_t)(budget / ((size_t)r.cap * 12))));
        for (int64_t q0 = r.q0; q0 < r.q0 + r.qn; q0 += slab) {
            a.q_begin = (int)q0;
            a.q_count = (int)std::min<int64_t>(slab, r.q0 + r.qn - q0);
            if (type == 0) VISMA_TRY((launch_normals<0, false, true>(a, stream)));
            else VISMA_TRY((launch_normals<2, false, true>(a, stream)));
        }
    }
    return hipStreamSynchronize(stream);
}

// search_type 0 KNN(knn) | 1 Radius(radius) | 2 Hybrid(radius, knn = max_nn); h_nrm_in may be NULL: upload, the core, download
hipError_t estimate_normals_device(const double *h_xyz, int64_t n, const double *h_nrm_in, int search_type,
                                   int knn, double radius, double *h_out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (search_type < 0 || search_type > 2 || n > 0x7fffffff) return hipErrorInvalidValue;
    if (estimate_normals_trivial(search_type, knn, radius)) {
        for (int64_t i = 0; i < n; i++) { h_out[3 * i] = 0.0; h_out[3 * i + 1] = 0.0; h_out[3 * i + 2] = 1.0; }
        return hipSuccess;
    }
    DevBufs B;
    double *d_xyz = nullptr, *d_nin = nullptr, *d_out = nullptr;
    VISMA_TRY(B.alloc(&d_xyz, 3 * (size_t)n));
    VISMA_TRY(B.alloc(&d_out, 3 * (size_t)n));
    if (h_nrm_in) {
        VISMA_TRY(B.alloc(&d_nin, 3 * (size_t)n));
        VISMA_TRY(hipMemcpyAsync(d_nin, h_nrm_in, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    }
    VISMA_TRY(hipMemcpyAsync(d_xyz, h_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    double origin[3] = {0.0, 0.0, 0.0};
    nn_binning_origin(h_xyz, n, origin);
    VISMA_TRY(estimate_normals_core(d_xyz, n, d_nin, origin, search_type, knn, radius, d_out, stream));
    VISMA_TRY(hipMemcpyAsync(h_out, d_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

}  // namespace visma
