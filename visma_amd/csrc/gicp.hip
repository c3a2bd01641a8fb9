// gicp.hip -- generalized ICP (plane-to-plane; Segal, Haehnel, Thrun: "Generalized-ICP", RSS 2009) on gfx950: every pair of
// a pass enters the normal equations with the 3 x 3 weight M = (C_t + R C_s R^T)^-1, the two covariances those of a
// surface element with the point's normal: C = I - (1 - eps) n n^T.  So the sum is C = 2 I - (1 - eps)(n n^T + m m^T),
// n the target's normal, m = R n_s the source's normal in the target frame (visma_icp.h states the step).
//
//  GicpReduce   per pair: p, q as the plain reduction forms them, d = p - q, C, M by the adjugate and the determinant of a
//               symmetric 3 x 3, then with J = [-hat(p) | I] the 21 upper entries of J^T M J = [[-P M P, P M], [., M]], the
//               6 of J^T M d = [p x M d; M d], K, |d|^2 and d^T M d: 30 accumulators.  In the frame of pair_pass.h; the
//               last workgroup publishes 38 statistics and the cost.
// A normal is never an index or an address: a non-finite one reaches the sums only; a zero one leaves its point isotropic.
// No floating-point atomics: a run is bit-identical to itself.  (Reasoning and numbers: DESIGN.md 4.4c5.)
#include "pair_pass.h"

namespace visma {

struct GicpReduce {
    using Args = GicpArgs;
    static constexpr int kAcc = 30;                      // K, sum |d|^2, 21 of J^T M J, 6 of J^T M d, sum d^T M d
    static constexpr int kPublished = kGicpPublished;
    static constexpr bool kPublishTotals = false;
    double k1;

    __device__ explicit GicpReduce(const Args &a) : k1(1.0 - a.epsilon) {}
    template <bool S64>
    __device__ __forceinline__ void visit(const Args &a, long long i, int j, double *acc)
    {
        if (j < 0) return;
        const double *T = a.T64.m;
        double s[3], q[3], n[3], ns[3];
        pair_load3<S64>(a.src, a.src64, i, s);
        pair_load3<S64>(a.tgt, a.tgt64, j, q);
        pair_load3<S64>(a.nrm, a.nrm64, j, n);
        pair_load3<S64>(a.snrm, a.snrm64, i, ns);
        // p = T64 * s, then both points into the frame of `off`
        double p[3], d[3], m[3];
        pair_transform(a.T64, s, p);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            p[k] += a.off.v[k];
            d[k] = p[k] - (q[k] + a.off.v[k]);
            m[k] = T[4 * k] * ns[0] + T[4 * k + 1] * ns[1] + T[4 * k + 2] * ns[2];
        }
        // C = 2 I - (1 - eps)(n n^T + m m^T), symmetric: c00 c01 c02 c11 c12 c22
        const double c00 = 2.0 - k1 * (n[0] * n[0] + m[0] * m[0]), c01 = -k1 * (n[0] * n[1] + m[0] * m[1]);
        const double c02 = -k1 * (n[0] * n[2] + m[0] * m[2]), c11 = 2.0 - k1 * (n[1] * n[1] + m[1] * m[1]);
        const double c12 = -k1 * (n[1] * n[2] + m[1] * m[2]), c22 = 2.0 - k1 * (n[2] * n[2] + m[2] * m[2]);
        // M = adj(C) / det(C)
        const double a00 = c11 * c22 - c12 * c12, a01 = c02 * c12 - c01 * c22, a02 = c01 * c12 - c02 * c11;
        const double a11 = c00 * c22 - c02 * c02, a12 = c01 * c02 - c00 * c12, a22 = c00 * c11 - c01 * c01;
        const double det = c00 * a00 + c01 * a01 + c02 * a02;
        const double rdet = 1.0 / det;                       // (one division per pair)
        double M[3][3];
        M[0][0] = a00 * rdet; M[0][1] = a01 * rdet; M[0][2] = a02 * rdet;
        M[1][1] = a11 * rdet; M[1][2] = a12 * rdet; M[2][2] = a22 * rdet;
        M[1][0] = M[0][1]; M[2][0] = M[0][2]; M[2][1] = M[1][2];
        // G = hat(p) M (the upper right block), B = -G hat(p) (the upper left one), e = M d
        double G[3][3], B[3][3], e[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            G[0][k] = p[1] * M[2][k] - p[2] * M[1][k];
            G[1][k] = p[2] * M[0][k] - p[0] * M[2][k];
            G[2][k] = p[0] * M[1][k] - p[1] * M[0][k];
            e[k] = M[k][0] * d[0] + M[k][1] * d[1] + M[k][2] * d[2];
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {
            B[r][0] = G[r][2] * p[1] - G[r][1] * p[2];
            B[r][1] = G[r][0] * p[2] - G[r][2] * p[0];
            B[r][2] = G[r][1] * p[0] - G[r][0] * p[1];
        }
        acc[0] += 1.0;
        acc[1] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        // the upper triangle of the 6 x 6, row by row
        acc[2] += B[0][0]; acc[3] += B[0][1]; acc[4] += B[0][2]; acc[5] += G[0][0]; acc[6] += G[0][1]; acc[7] += G[0][2];
        acc[8] += B[1][1]; acc[9] += B[1][2]; acc[10] += G[1][0]; acc[11] += G[1][1]; acc[12] += G[1][2];
        acc[13] += B[2][2]; acc[14] += G[2][0]; acc[15] += G[2][1]; acc[16] += G[2][2];
        acc[17] += M[0][0]; acc[18] += M[0][1]; acc[19] += M[0][2];
        acc[20] += M[1][1]; acc[21] += M[1][2];
        acc[22] += M[2][2];
        // J^T M d = [p x e; e]
        acc[23] += p[1] * e[2] - p[2] * e[1];
        acc[24] += p[2] * e[0] - p[0] * e[2];
        acc[25] += p[0] * e[1] - p[1] * e[0];
        acc[26] += e[0]; acc[27] += e[1]; acc[28] += e[2];
        acc[29] += d[0] * e[0] + d[1] * e[1] + d[2] * e[2];
    }
    __device__ void finish(const double *tot, double *stats) const
    {
        expand_moments<true>(tot, stats);                    // (the point-to-plane layout: the totals are the statistics)
        stats[kNStats] = tot[29];                            // sum d^T M d
    }
};

hipError_t launch_gicp_reduce(const GicpArgs &a, hipStream_t stream) { return launch_pair_reduce<GicpReduce>(a, a.src64 != nullptr, stream); }

}  // namespace visma
