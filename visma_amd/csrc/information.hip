// information.hip -- the information matrix of a registered pair of clouds (Open3D's GetInformationMatrixFromPointClouds,
// Registration.cpp:352-413; Choi, Zhou, Koltun: "Robust Reconstruction of Indoor Scenes", CVPR 2015) on gfx950: the
// weight a pose-graph edge enters the global optimisation with.  Per pair of the last nn_pass, with q the TARGET point
// in the caller's frame, G = [-hat(q) | I] (3 x 6) and the result is sum G^T G -- WITHOUT the identity terms the
// reference adds (visma_icp.h states the deviation).
//
//  InformationReduce   per pair: q = t_j + off as gicp.hip forms it, then the ten sums the 6 x 6 consists of: K, sum x, y, z,
//                      sum xx, yy, zz, xy, xz, yz.  In the frame of pair_pass.h; the last workgroup publishes the column
//                      totals as they are; information_from_sums (host_math.hpp) lays them out as the matrix.
//  ... one launch per edge: the batched entry point (visma_icp_information_matrices) is a host loop over edges that
//  uploads a shared target once, so an edge's sums never depend on what else the call computed.  A second entry that
//  reduces many edges in one launch was deliberately not built: it needs every edge's winners on the device at once,
//  which the per-edge search does not leave.
// The source's coordinates are not read: only which source positions have a pair.  A target point is never an index or
// an address: a non-finite one reaches the sums only.
// No floating-point atomics: a run is bit-identical to itself.  (Reasoning and numbers: DESIGN.md 4.4c9.)
#include "pair_pass.h"

namespace visma {

struct InformationReduce {
    using Args = InformationArgs;
    static constexpr int kAcc = kInfoAcc;
    static constexpr int kPublished = kInfoAcc;
    static constexpr bool kPublishTotals = true;

    __device__ explicit InformationReduce(const Args &) {}
    template <bool S64>
    __device__ __forceinline__ void visit(const Args &a, long long, int j, double *acc)
    {
        if (j < 0) return;
        double q[3];
        pair_load3<S64>(a.tgt, a.tgt64, j, q);
        // into the frame of `off`: the caller's
        const double x = q[0] + a.off.v[0], y = q[1] + a.off.v[1], z = q[2] + a.off.v[2];
        acc[0] += 1.0;
        acc[1] += x; acc[2] += y; acc[3] += z;
        acc[4] += x * x; acc[5] += y * y; acc[6] += z * z;
        acc[7] += x * y; acc[8] += x * z; acc[9] += y * z;
    }
};

// (the source's coordinates are not read: the f64 target decides)
hipError_t launch_information_reduce(const InformationArgs &a, hipStream_t stream) { return launch_pair_reduce<InformationReduce>(a, a.tgt64 != nullptr, stream); }

}  // namespace visma
