// cloud_distance.hip -- exact, unbounded nearest-neighbour distances between point clouds:
//
//  point_cloud_distance_device      open3d::ComputePointCloudToPointCloudDistance (O3D/Core/Geometry/PointCloud.cpp:
//                                   122-142): for every source point, the distance to the nearest target point.
//  nearest_neighbor_distance_device open3d::ComputePointCloudNearestNeighborDistance (PointCloud.cpp:200-219): for
//                                   every point, the distance to the nearest OTHER point of the same cloud (the
//                                   reference's SearchKNN(p, 2) -> dists[1]; a duplicate point gives 0).
//
// The reference answers both with flann's exact KD-tree search (checks = -1), whose distance is L2<double>:
// ((dx*dx) + dy*dy) + dz*dz in f64.  Here the target goes into a point BVH of the same shape as mesh.hip's
// (bvh_common.h): points sorted by the 30-bit Morton code over the target's bounding box (stable radix sort),
// kPtLeaf consecutive points per leaf with their exact min/max box, and the implicit heap-ordered tree above the
// leaves.  The queries are walked in Morton order too (neighbouring lanes take the same path), one per lane, depth
// first, nearer child first, with the LDS stack of point_mesh_bvh_kernel; each lane first scans the leaf at its
// Morton rank, so that most of the tree is pruned at the first box tests.
//
// Exactness.  A box holding point q has lo_a <= q_a <= hi_a exactly, so for a query p with p_a < lo_a the computed
// lo_a - p_a never exceeds the computed q_a - p_a (rounding is monotone), and likewise above the box; inside it the
// bound's term is 0.  Squared and summed in the same x, y, z order as d2, the box's lower bound therefore never
// exceeds a computed d2 of any of its points: no box inflation is needed.  Only the distance is returned, never an
// index, so a box whose bound is >= the best d2 so far cannot lower it and is pruned, and the walk ends as soon as
// the best is 0 (otherwise a cloud of repeated points would visit every leaf for every query).  The result is the
// minimum of the same computed values the reference minimises: bit for bit, whichever of several equal candidates
// is met first.
#include "bvh_common.h"

#include <math.h>

namespace visma {

#ifndef VISMA_CLOUD_LEAF
#define VISMA_CLOUD_LEAF 4              // points per leaf (4 / 8 / 16 measured: DESIGN 4.4c2)
#endif
constexpr int kPtLeaf = VISMA_CLOUD_LEAF;
constexpr int kCloudBlock = 64;

// the target points in Morton order: pts[j] = P[order[j]]
__global__ __launch_bounds__(256) void cloud_gather_kernel(const double *__restrict__ P,
                                                           const unsigned *__restrict__ order, long long n,
                                                           double *__restrict__ pts)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const long long i = order[j];
#pragma unroll
    for (int a = 0; a < 3; a++) pts[3 * j + a] = P[3 * i + a];
}

// leaf boxes: the exact min / max of their points (fmin / fmax pass over a NaN coordinate); the missing leaves
// [ceil(n / kPtLeaf), P) keep an inverted box, whose lower bound is +inf
__global__ __launch_bounds__(256) void cloud_leaf_kernel(const double *__restrict__ pts, long long n, long long P,
                                                         double *__restrict__ nodes)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long t = g * kPtLeaf; t < (g + 1) * kPtLeaf && t < n; t++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double v = pts[3 * t + a];
            lo[a] = fmin(lo[a], v);
            hi[a] = fmax(hi[a], v);
        }
    double *b = nodes + 6 * (P + g);
#pragma unroll
    for (int a = 0; a < 3; a++) { b[a] = lo[a]; b[3 + a] = hi[a]; }
}

// flann's L2<double> on 3 values: ((0 + dx*dx) + dy*dy) + dz*dz, the leading 0 + exact
__device__ __forceinline__ double point_d2(const double p[3], const double *__restrict__ q)
{
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return dx * dx + dy * dy + dz * dz;
}

// d2 of p to the points [t0, t1) of `pts`, except the point `skip`, folded into best
__device__ __forceinline__ void scan_leaf(const double p[3], const double *__restrict__ pts, long long t0,
                                          long long t1, long long skip, double &best)
{
    for (long long t = t0; t < t1; t++) {
        const double d = point_d2(p, pts + 3 * t);
        if (t != skip && d < best) best = d;
    }
}

// One query per lane, queries in Morton order.  Cross mode (Pq != NULL): slot s is the caller's query qorder[s],
// whose code is qkey[s].  Self mode (Pq == NULL): the queries are the sorted targets themselves, slot s skips sorted
// slot s, and its result goes to the caller's row qorder[s] (the target's own sort order).  d2_out in caller order.
// Dynamic LDS: `depth` stack levels of (node u32, lower bound f32 rounded DOWN) per lane.
__global__ __launch_bounds__(kCloudBlock) void cloud_nn_kernel(
    const double *__restrict__ Pq, long long nq, const unsigned *__restrict__ qorder, const unsigned *__restrict__ qkey,
    const double *__restrict__ pts, const unsigned *__restrict__ tkey, long long nt, const double *__restrict__ nodes,
    long long P, int depth, double *__restrict__ d2_out)
{
    extern __shared__ unsigned cloud_smem[];
    unsigned *stk_node = cloud_smem;
    float *stk_lb = (float *)(cloud_smem + depth * kCloudBlock);
    const long long slot = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (slot >= nq) return;
    const long long i = qorder[slot];
    const bool self = Pq == nullptr;
    const double *src = self ? pts + 3 * slot : Pq + 3 * i;
    const double p[3] = {src[0], src[1], src[2]};
    if (p[0] != p[0] || p[1] != p[1] || p[2] != p[2]) {   // a NaN query: its value is unspecified, do not walk
        d2_out[i] = NAN;
        return;
    }
    const long long skip = self ? slot : -1;
    long long seed;                                        // the leaf at the query's Morton rank
    if (self) {
        seed = slot / kPtLeaf;
    } else {
        const unsigned code = qkey[slot];
        long long lo = 0, hi = nt;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (tkey[mid] < code) lo = mid + 1; else hi = mid;
        }
        seed = (lo < nt ? lo : nt - 1) / kPtLeaf;
    }
    double best = INFINITY;
    scan_leaf(p, pts, seed * kPtLeaf, min((seed + 1) * kPtLeaf, nt), skip, best);
    int sp = 1;
    stk_node[threadIdx.x] = 1u;
    stk_lb[threadIdx.x] = 0.f;
    while (sp > 0 && best > 0.0) {
        --sp;
        const unsigned node = stk_node[sp * kCloudBlock + threadIdx.x];
        if ((double)stk_lb[sp * kCloudBlock + threadIdx.x] >= best) continue;
        if ((long long)node >= P) {
            const long long g = (long long)node - P;
            if (g != seed) scan_leaf(p, pts, g * kPtLeaf, min((g + 1) * kPtLeaf, nt), skip, best);
        } else {
            const unsigned c0 = 2u * node, c1 = c0 + 1u;
            const double l0 = box_lower_bound(nodes + 6 * (long long)c0, p);
            const double l1 = box_lower_bound(nodes + 6 * (long long)c1, p);
            const bool first0 = l0 <= l1;
            const double lfar = first0 ? l1 : l0, lnear = first0 ? l0 : l1;
            if (lfar < best) {                            // farther child below the nearer one
                stk_node[sp * kCloudBlock + threadIdx.x] = first0 ? c1 : c0;
                stk_lb[sp * kCloudBlock + threadIdx.x] = round_down_f32(lfar);
                ++sp;
            }
            if (lnear < best) {
                stk_node[sp * kCloudBlock + threadIdx.x] = first0 ? c0 : c1;
                stk_lb[sp * kCloudBlock + threadIdx.x] = round_down_f32(lnear);
                ++sp;
            }
        }
    }
    d2_out[i] = best;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

struct DevCloudTree {
    DeviceBuf<double> pts, nodes;        // sorted points, 2P boxes
    DeviceBuf<unsigned> key, order;      // their sorted codes and caller indices
    int64_t n = 0, P = 0;
    MortonParams mp;
};

hipError_t build_cloud_tree(const double *h_xyz, int64_t n, DevCloudTree &t, hipStream_t stream)
{
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < n; i++)                     // (a NaN coordinate takes no part)
        for (int a = 0; a < 3; a++) {
            const double v = h_xyz[3 * i + a];
            if (v < lo[a]) lo[a] = v;
            if (v > hi[a]) hi[a] = v;
        }
    t.n = n;
    t.mp = morton_params(lo, hi);
    DeviceBuf<double> raw;
    DeviceBuf<unsigned> key, val;
    DeviceBuf<char> tmp;
    DEV_RESET(raw, 3 * n);
    DEV_RESET(key, n);
    DEV_RESET(val, n);
    DEV_RESET(t.key, n);
    DEV_RESET(t.order, n);
    DEV_RESET(t.pts, 3 * n);
    VISMA_TRY(hipMemcpyAsync(raw, h_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(point_code_kernel, dim3(nb), dim3(256), 0, stream, raw, (long long)n, t.mp,
                       key, val);
    VISMA_TRY(morton_sort(key, t.key, val, t.order, n, tmp,
                        stream));
    hipLaunchKernelGGL(cloud_gather_kernel, dim3(nb), dim3(256), 0, stream, raw,
                       t.order, (long long)n, t.pts);
    const int64_t nleaf = (n + kPtLeaf - 1) / kPtLeaf;
    int64_t P = 1;
    while (P < nleaf) P <<= 1;
    t.P = P;
    DEV_RESET(t.nodes, 6 * 2 * P);
    hipLaunchKernelGGL(cloud_leaf_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream,
                       t.pts, (long long)n, (long long)P, t.nodes);
    VISMA_TRY(build_bvh_levels(t.nodes, P, stream));
    // the temporaries above are freed when this function returns: wait for the kernels using them
    return hipStreamSynchronize(stream);
}

// d2 of the nq queries (d_q in caller order, or NULL for the tree's own points) -> distances in h_dist
hipError_t query_cloud_tree(const DevCloudTree &t, const double *d_q, int64_t nq, const unsigned *qorder,
                            const unsigned *qkey, double *h_dist, hipStream_t stream)
{
    DeviceBuf<double> d2;
    DEV_RESET(d2, nq);
    int depth = 2;                                   // levels below the root + slack
    for (int64_t q = t.P; q > 1; q >>= 1) depth++;
    hipLaunchKernelGGL(cloud_nn_kernel, dim3((unsigned)((nq + kCloudBlock - 1) / kCloudBlock)), dim3(kCloudBlock),
                       (size_t)depth * kCloudBlock * 8, stream, d_q, (long long)nq, qorder, qkey, t.pts,
                       t.key, (long long)t.n, t.nodes, (long long)t.P, depth,
                       d2);
    hipLaunchKernelGGL(sqrt_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, d2,
                       (long long)nq);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(hipMemcpyAsync(h_dist, d2, sizeof(double) * nq, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

}  // namespace

hipError_t point_cloud_distance_device(const double *h_src, int64_t ns, const double *h_tgt, int64_t nt,
                                       double *h_dist, hipStream_t stream)
{
    if (ns <= 0) return hipSuccess;
    if (ns > 0x7fffffff || nt > 0x7fffffff) return hipErrorInvalidValue;
    if (nt <= 0) {                                   // SearchKNN on an empty tree: the preset dists[0] = 0 stays
        for (int64_t i = 0; i < ns; i++) h_dist[i] = 0.0;
        return hipSuccess;
    }
    DevCloudTree tree;
    VISMA_TRY(build_cloud_tree(h_tgt, nt, tree, stream));
    DeviceBuf<double> q;
    DeviceBuf<unsigned> key, val, qkey, qorder;
    DeviceBuf<char> tmp;
    DEV_RESET(q, 3 * ns);
    DEV_RESET(key, ns);
    DEV_RESET(val, ns);
    DEV_RESET(qkey, ns);
    DEV_RESET(qorder, ns);
    VISMA_TRY(hipMemcpyAsync(q, h_src, sizeof(double) * 3 * ns, hipMemcpyHostToDevice, stream));
    // the queries sorted by their code over the TARGET's box: the rank of that code among the target's is the seed
    hipLaunchKernelGGL(point_code_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, stream, q,
                       (long long)ns, tree.mp, key, val);
    VISMA_TRY(morton_sort(key, qkey, val, qorder, ns, tmp,
                        stream));
    return query_cloud_tree(tree, q, ns, qorder, qkey, h_dist, stream);
}

hipError_t nearest_neighbor_distance_device(const double *h_xyz, int64_t n, double *h_dist, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    if (n == 1) {                                    // SearchKNN(p, 2) finds one point: the reference writes 0
        h_dist[0] = 0.0;
        return hipSuccess;
    }
    DevCloudTree tree;
    VISMA_TRY(build_cloud_tree(h_xyz, n, tree, stream));
    return query_cloud_tree(tree, nullptr, n, tree.order, nullptr, h_dist, stream);
}

}  // namespace visma
