// odometry.hip -- the reductions of RGB-D odometry (Open3D's NormalizeIntensity and DoSingleIteration: Odometry.cpp,
// RGBDOdometryJacobian.cpp; Steinbruecker, Sturm, Cremers 2011 for the colour term, Park, Zhou, Koltun, ICCV 2017 for the
// hybrid one) on gfx950, in the frame of pair_pass.h: the "source positions" are the source pixels, idx is what the
// correspondence kernel (odometry_image.hip) wrote.
//
//  OdoMeanReduce    K, the sum of the source's gray over the pairs' source pixels and of the target's over their target
//                   pixels, fp32 values widened and summed in f64; the host divides (NormalizeIntensity's two means).
//  OdometryReduce   per pair, p = T * xyz_s[i]: the photometric row -- the target's intensity gradient (Sobel, scaled by
//                   1 / 8) carried through the projection, residual gray_t - gray_s as ONE fp32 subtraction (as the
//                   reference writes it) -- and, with the hybrid term, the depth row the same way with d/dz - 1 (`d2 - 1.0f`
//                   there) and residual depth_t - p.z, the two weighted sqrt(1 - 0.968) and sqrt(0.968); a NaN depth
//                   gradient counts as 0.  Every image value is widened first, everything after that is f64.  29
//                   accumulators: K, sum r^2, the 21 upper entries of J^T J, the 6 of J^T r; finish() lays them out as the
//                   38 statistics, so that unpack_stats / gn_from_stats(expmap = false) solve the step.
// No floating-point atomics: a run is bit-identical to itself.  (Reasoning and numbers: DESIGN.md 4.4c10.)
#include "pair_pass.h"

namespace visma {

namespace {

constexpr double kSobelScale = 0.125;

// the row J with residual r: acc[1] += r^2, acc[2 .. 23) += upper triangle of J^T J (row by row), acc[23 .. 29) += J^T r
__device__ __forceinline__ void add_row(double *acc, const double J[6], double r)
{
    acc[1] += r * r;
    int k = 2;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) acc[k++] += J[i] * J[j];
#pragma unroll
    for (int i = 0; i < 6; i++) acc[23 + i] += J[i] * r;
}

}  // namespace

struct OdoMeanReduce {
    using Args = OdoMeanArgs;
    static constexpr int kAcc = kOdoMeanAcc;
    static constexpr int kPublished = kOdoMeanAcc;
    static constexpr bool kPublishTotals = true;

    __device__ explicit OdoMeanReduce(const Args &) {}
    template <bool S64>
    __device__ __forceinline__ void visit(const Args &a, long long i, int j, double *acc)
    {
        if (j < 0) return;
        acc[0] += 1.0;
        acc[1] += (double)a.gray_s[i];
        acc[2] += (double)a.gray_t[j];
    }
};

template <bool HYBRID>
struct OdometryReduce {
    using Args = OdometryArgs;
    static constexpr int kAcc = 29;                      // K, sum r^2, 21 of J^T J, 6 of J^T r
    static constexpr int kPublished = kNStats;
    static constexpr bool kPublishTotals = false;

    double s_img, s_dep;
    __device__ explicit OdometryReduce(const Args &a) : s_img(HYBRID ? a.w_photo : 1.0), s_dep(a.w_depth) {}
    template <bool S64>
    __device__ __forceinline__ void visit(const Args &a, long long i, int j, double *acc)
    {
        if (j < 0) return;
        const float4 s4 = a.xyz_s[i];
        const double s[3] = {(double)s4.x, (double)s4.y, (double)s4.z};
        double p[3];
        pair_transform(a.T64, s, p);
        const double diff_photo = (double)(a.gray_t[j] - a.gray_s[i]);
        const double dIdx = kSobelScale * (double)a.gray_dx[j], dIdy = kSobelScale * (double)a.gray_dy[j];
        const double invz = 1.0 / p[2];
        const double c0 = dIdx * a.fx * invz, c1 = dIdy * a.fy * invz;
        const double c2 = -(c0 * p[0] + c1 * p[1]) * invz;
        double J[6];
        J[0] = s_img * (-p[2] * c1 + p[1] * c2);
        J[1] = s_img * (p[2] * c0 - p[0] * c2);
        J[2] = s_img * (-p[1] * c0 + p[0] * c1);
        J[3] = s_img * c0; J[4] = s_img * c1; J[5] = s_img * c2;
        acc[0] += 1.0;
        add_row(acc, J, s_img * diff_photo);
        if constexpr (HYBRID) {
            double dDdx = kSobelScale * (double)a.depth_dx[j], dDdy = kSobelScale * (double)a.depth_dy[j];
            if (isnan(dDdx)) dDdx = 0.0;
            if (isnan(dDdy)) dDdy = 0.0;
            const double diff_geo = (double)a.depth_t[j] - p[2];
            const double d0 = dDdx * a.fx * invz, d1 = dDdy * a.fy * invz;
            const double d2 = -(d0 * p[0] + d1 * p[1]) * invz;
            J[0] = s_dep * ((-p[2] * d1 + p[1] * d2) - p[1]);
            J[1] = s_dep * ((p[2] * d0 - p[0] * d2) + p[0]);
            J[2] = s_dep * (-p[1] * d0 + p[0] * d1);
            J[3] = s_dep * d0; J[4] = s_dep * d1; J[5] = s_dep * (d2 - 1.0);
            add_row(acc, J, s_dep * diff_geo);
        }
    }
    __device__ void finish(const double *tot, double *stats) const
    {
        for (int k = 0; k < kAcc; k++) stats[k] = tot[k];
        for (int k = kAcc; k < kNStats; k++) stats[k] = 0.0;     // (the moments of the closed-form solvers: none here)
    }
};

hipError_t launch_odo_mean_reduce(const OdoMeanArgs &a, hipStream_t stream) { return launch_pair_reduce<OdoMeanReduce>(a, false, stream); }

hipError_t launch_odometry_reduce(const OdometryArgs &a, hipStream_t stream)
{
    if (a.method == kOdoHybrid) return launch_pair_reduce<OdometryReduce<true>>(a, false, stream);
    return launch_pair_reduce<OdometryReduce<false>>(a, false, stream);
}

}  // namespace visma
