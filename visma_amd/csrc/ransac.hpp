// ransac.hpp -- ONE trial of open3d::RegistrationRANSACBasedOnFeatureMatching / ...BasedOnCorrespondence
// (O3D/Core/Registration/Registration.cpp:188-353, CorrespondenceChecker.cpp:35-89), host + device: the kernels of
// ransac.hip and visma_icp_ransac_hypotheses_host run these very functions, so there is one copy of the arithmetic.
// f64, -ffp-contract=off, every comparison written as the reference writes it (one with a NaN is false and rejects nothing, as there).
// Semantics: include/visma_icp.h, "RANSAC global registration"; DESIGN.md 4.4c8.
#pragma once

#include "host_math.hpp"

namespace visma {

constexpr int kRansacMinN = 3, kRansacMaxN = 8;
// verdict of a trial
constexpr int kRansacPass = 0;      // solved, every checker passed: to be validated
constexpr int kRansacBefore = 1;    // rejected before alignment: a pair without a partner (-1), or the edge-length checker
constexpr int kRansacAfter = 2;     // solved, rejected by the distance or the normal checker

// The problem as a trial sees it; every pointer in the memory space of whoever calls (host arrays or device arrays).
struct RansacView {
    const double *src = nullptr, *tgt = nullptr;          // ns x 3, nt x 3
    const double *src_n = nullptr, *tgt_n = nullptr;      // normals, or NULL
    const int32_t *pair_src = nullptr;                    // pair k = (pair_src[k], pair_tgt[k]); NULL: (k, pair_tgt[k])
    const int32_t *pair_tgt = nullptr;                    // -1: no partner (a NaN feature row)
    long long n_pairs = 0;
    const int32_t *draws = nullptr;                       // ransac_n per trial, by absolute trial; NULL: Philox keyed by seed
    unsigned long long seed = 0;
    double edge = 0.0, dist = 0.0, cos_normal = 0.0;      // thresholds of the three checkers ...
    int use_edge = 0, use_dist = 0, use_normal = 0;       // ... and whether each one runs
};

template <int N>
struct RansacSample {
    double p[N][3], q[N][3];
    int si[N], ti[N];
};

// the pairs trial t draws (Registration.cpp:206-208, :273-293): false where one of them has no partner
template <int N>
VISMA_HD bool ransac_gather(const RansacView &v, long long t, RansacSample<N> &s)
{
    bool ok = true;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < N; j++) {
        long long k;
        if (v.draws) {
            k = (((long long)v.draws[t * N + j] % v.n_pairs) + v.n_pairs) % v.n_pairs;
        } else {
            if ((j & 3) == 0)
                philox4x32_host((uint32_t)t, (uint32_t)((unsigned long long)t >> 32), (uint32_t)(j >> 2), 0u, (uint32_t)v.seed,
                                (uint32_t)(v.seed >> 32), w);
            k = (long long)(w[j & 3] % (unsigned long long)v.n_pairs);
        }
        s.si[j] = v.pair_src ? v.pair_src[k] : (int)k;
        s.ti[j] = v.pair_tgt[k];
        if (s.ti[j] < 0) ok = false;
    }
    if (!ok) return false;
#pragma unroll
    for (int j = 0; j < N; j++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            s.p[j][a] = v.src[3 * (long long)s.si[j] + a];
            s.q[j][a] = v.tgt[3 * (long long)s.ti[j] + a];
        }
    return true;
}

// CorrespondenceCheckerBasedOnEdgeLength::Check (CorrespondenceChecker.cpp:35-53)
template <int N>
VISMA_HD bool ransac_edge_ok(const RansacSample<N> &s, double similarity)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i + 1; j < N; j++) {
            const double ds = norm3(s.p[i][0] - s.p[j][0], s.p[i][1] - s.p[j][1], s.p[i][2] - s.p[j][2]);
            const double dt = norm3(s.q[i][0] - s.q[j][0], s.q[i][1] - s.q[j][1], s.q[i][2] - s.q[j][2]);
            if (ds < dt * similarity || dt < ds * similarity) ok = false;
        }
    return ok;
}

// TransformationEstimationPointToPoint(false)::ComputeTransformation (TransformationEstimation.cpp:46-59: Eigen::umeyama
// without scaling, Umeyama.h:118-159) of the N pairs into T (row-major 3 x 4), then the checkers that need the alignment
// (CorrespondenceChecker.cpp:55-89)
template <int N>
VISMA_HD int ransac_solve_check(const RansacView &v, const RansacSample<N> &s, double T[12])
{
    const double inv = 1.0 / (double)N;
    double pm[3] = {0.0, 0.0, 0.0}, qm[3] = {0.0, 0.0, 0.0}, sigma[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < N; j++)
#pragma unroll
        for (int a = 0; a < 3; a++) { pm[a] += s.p[j][a]; qm[a] += s.q[j][a]; }
#pragma unroll
    for (int a = 0; a < 3; a++) { pm[a] *= inv; qm[a] *= inv; }
#pragma unroll
    for (int j = 0; j < N; j++)
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) sigma[a * 3 + b] += (s.q[j][a] - qm[a]) * (s.p[j][b] - pm[b]);
#pragma unroll
    for (int i = 0; i < 9; i++) sigma[i] *= inv;
    double R[9];
    (void)umeyama_rotation(sigma, R);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T[i * 4 + j] = R[i * 3 + j];
        T[i * 4 + 3] = qm[i] - (R[i * 3] * pm[0] + R[i * 3 + 1] * pm[1] + R[i * 3 + 2] * pm[2]);
    }
    bool ok = true;
    if (v.use_dist) {
#pragma unroll
        for (int j = 0; j < N; j++) {
            double d[3];
#pragma unroll
            for (int i = 0; i < 3; i++)
                d[i] = s.q[j][i] - (T[i * 4] * s.p[j][0] + T[i * 4 + 1] * s.p[j][1] + T[i * 4 + 2] * s.p[j][2] + T[i * 4 + 3]);
            if (norm3(d[0], d[1], d[2]) > v.dist) ok = false;
        }
    }
    if (v.use_normal && v.src_n && v.tgt_n) {
#pragma unroll
        for (int j = 0; j < N; j++) {
            const double *a = v.src_n + 3 * (long long)s.si[j], *b = v.tgt_n + 3 * (long long)s.ti[j];
            double dot = 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) dot += b[i] * (T[i * 4] * a[0] + T[i * 4 + 1] * a[1] + T[i * 4 + 2] * a[2]);
            if (dot < v.cos_normal) ok = false;
        }
    }
    return ok ? kRansacPass : kRansacAfter;
}

// the whole trial; T is all zeros where nothing was solved
template <int N>
VISMA_HD int ransac_trial(const RansacView &v, long long t, double T[12])
{
    RansacSample<N> s;
    if (!ransac_gather<N>(v, t, s) || (v.use_edge && !ransac_edge_ok<N>(s, v.edge))) {
#pragma unroll
        for (int i = 0; i < 12; i++) T[i] = 0.0;
        return kRansacBefore;
    }
    return ransac_solve_check<N>(v, s, T);
}

// EvaluateRANSACBasedOnCorrespondence (Registration.cpp:98-123) for pair c: the squared distance after T
VISMA_HD double ransac_pair_dis2(const double *src, const double *tgt, int si, int ti, const double T[12])
{
    const double *p = src + 3 * (long long)si, *q = tgt + 3 * (long long)ti;
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double d = (T[i * 4] * p[0] + T[i * 4 + 1] * p[1] + T[i * 4 + 2] * p[2] + T[i * 4 + 3]) - q[i];
        d2 += d * d;
    }
    return d2;
}

}  // namespace visma
