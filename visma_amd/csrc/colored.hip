// colored.hip -- colored ICP (Park, Zhou, Koltun: "Colored Point Cloud Registration Revisited", ICCV 2017; the reference's
// O3D/Core/Registration/ColoredICP.cpp:139-232) on gfx950: every pair of a pass enters the normal equations with two
// rows, the point-to-plane row and a photometric row that compares the source point's intensity with the target's
// intensity carried along the target's colour gradient g (color_gradient.hip) to the source point's projection into
// the target's tangent plane (visma_icp.h states the step).
//
//  ColoredReduce   per pair: p, q as the plain reduction forms them, the two rows J_g = sg [p x n | n], r_g = sg (p - q).n
//                  and J_c = sc [p x h | h], h = -(I - n n^T) g, r_c = sc (I_s - (g.(p' - q) + I_t)), sg = sqrt(lambda),
//                  sc = sqrt(1 - lambda); both rows have the shape [p x v | v], so one helper adds the 21 upper entries of
//                  J^T J and the 6 of J^T r for each.  With K, |p - q|^2, r_g^2 and r_c^2: 31 accumulators.  In the frame
//                  of pair_pass.h; the last workgroup publishes 38 statistics and the two costs.
// Intensities and gradients exist in f64 only (k / 255 is not an fp32 number, and the photometric residual is a difference
// of nearby values); points and normals are the copies the search ran on.  A colour, a gradient or a normal is never an
// index or an address: a non-finite one reaches the sums only.  No floating-point atomics: a run is bit-identical to
// itself.  (Reasoning and numbers: DESIGN.md 4.4c6.)
#include "pair_pass.h"

namespace visma {

namespace {

// the row J = s [p x v | v] with residual r: acc[2 .. 23) += upper triangle of J^T J (row by row), acc[23 .. 29) += J^T r
__device__ __forceinline__ void add_row(double *acc, const double p[3], const double v[3], double s, double r)
{
    double J[6];
    J[0] = s * (p[1] * v[2] - p[2] * v[1]);
    J[1] = s * (p[2] * v[0] - p[0] * v[2]);
    J[2] = s * (p[0] * v[1] - p[1] * v[0]);
    J[3] = s * v[0]; J[4] = s * v[1]; J[5] = s * v[2];
    int k = 2;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) acc[k++] += J[i] * J[j];
#pragma unroll
    for (int i = 0; i < 6; i++) acc[23 + i] += J[i] * r;
}

}  // namespace

struct ColoredReduce {
    using Args = ColoredArgs;
    static constexpr int kAcc = 31;                      // K, sum |d|^2, 21 of J^T J, 6 of J^T r, sum r_g^2, sum r_c^2
    static constexpr int kPublished = kColoredPublished;
    static constexpr bool kPublishTotals = false;

    __device__ explicit ColoredReduce(const Args &) {}
    template <bool S64>
    __device__ __forceinline__ void visit(const Args &a, long long i, int j, double *acc)
    {
        if (j < 0) return;
        const double sg = a.sqrt_lambda, sc = a.sqrt_one_minus_lambda;
        double s[3], q[3], n[3];
        pair_load3<S64>(a.src, a.src64, i, s);
        pair_load3<S64>(a.tgt, a.tgt64, j, q);
        pair_load3<S64>(a.nrm, a.nrm64, j, n);
        const double g[3] = {a.grad[3ll * j], a.grad[3ll * j + 1], a.grad[3ll * j + 2]};
        const double is = a.src_int[i], it = a.tgt_int[j];
        // p = T64 * s, then both points into the frame of `off`
        double p[3], d[3];
        pair_transform(a.T64, s, p);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            p[k] += a.off.v[k];
            q[k] += a.off.v[k];
            d[k] = p[k] - q[k];
        }
        const double dn = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
        // the photometric residual at p' = p - ((p - q).n) n (:171-177)
        const double e0 = (p[0] - dn * n[0]) - q[0], e1 = (p[1] - dn * n[1]) - q[1], e2 = (p[2] - dn * n[2]) - q[2];
        const double rc = sc * (is - ((g[0] * e0 + g[1] * e1 + g[2] * e2) + it));
        const double rg = sg * dn;
        // h = -(I - n n^T) g, the matrix entry by entry as :179-184
        double h[3];
        h[0] = -(g[0] * (1.0 - n[0] * n[0]) + g[1] * (-n[0] * n[1]) + g[2] * (-n[0] * n[2]));
        h[1] = -(g[0] * (-n[0] * n[1]) + g[1] * (1.0 - n[1] * n[1]) + g[2] * (-n[1] * n[2]));
        h[2] = -(g[0] * (-n[0] * n[2]) + g[1] * (-n[1] * n[2]) + g[2] * (1.0 - n[2] * n[2]));
        acc[0] += 1.0;
        acc[1] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        add_row(acc, p, n, sg, rg);
        add_row(acc, p, h, sc, rc);
        acc[29] += rg * rg;
        acc[30] += rc * rc;
    }
    __device__ void finish(const double *tot, double *stats) const
    {
        expand_moments<true>(tot, stats);                    // (the point-to-plane layout: the totals are the statistics)
        stats[kNStats] = tot[29];                            // sum r_g^2
        stats[kNStats + 1] = tot[30];                        // sum r_c^2
    }
};

hipError_t launch_colored_reduce(const ColoredArgs &a, hipStream_t stream) { return launch_pair_reduce<ColoredReduce>(a, a.src64 != nullptr, stream); }

// I = (r + g + b) / 3 per point, in f64 and in that order (:94-95), from rows of `stride` doubles picked through `order`
// (NULL: identity) -- on the host: the one place a colour is read
void color_intensities(const double *rgb, int64_t n, int stride, const int32_t *order, double *out)
{
    for (int64_t i = 0; i < n; i++) out[i] = color_intensity(rgb + (size_t)(order ? order[i] : i) * stride);
}

}  // namespace visma
