// color_gradient.hip -- the colour gradient per target point of colored ICP (Park, Zhou, Koltun: "Colored Point Cloud
// Registration Revisited", ICCV 2017) on gfx950: the step the reference runs once per registration before its loop
// (O3D/Core/Registration/ColoredICP.cpp:74-137, InitializePointCloudForColoredICP).
//
// Per point k with normal n and intensity I_k: neighbours by the Hybrid search (radius, max_nn) in the order of the
// reference's result list -- the grid, the search and the list are nn_grid.hip's and nn_list.h's, shared with
// normals.hip and fpfh.hip --; fewer than 3 entries: the gradient is 0.  Else entry 0 is skipped whatever index it holds (the
// reference takes it for the point itself), every other entry a gives the row a' - p, a' = a - ((a - p).n) n its
// projection into the tangent plane, with the right side I_a - I_k, and one more row (nn - 1) n with right side 0 keeps
// the gradient in the plane.  A^T A (3 x 3) and A^T b are summed in f64 in list order; |det| < 1e-6 or a determinant
// that is not finite leaves 0 (Eigen.cpp:41-43), else the symmetric 3 x 3 is solved by its L D L^T factors written out.
//
// One thread per point, in cell order; lists of up to kNormalsMaxList entries in LDS: 12 bytes per entry and thread,
// so max_nn = 30 runs 128 threads on 45 KiB (3 workgroups per CU by LDS), max_nn = 170 runs 64 threads on 128 KiB of the
// 160 (one workgroup per CU) -- nn_launch.  A colour or a normal is never an index or an address: a non-finite
// one reaches the sums only.  (Reasoning and numbers: DESIGN.md 4.4c6.)
#include "nn_list.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace visma {

namespace {

struct GradArgs {
    NnGridView view;
    const double *nrm;           // n x 3
    const double *inten;         // n
    double *grad;                // n x 3, original order
    int n;
    int cap;                     // max_nn
    double r2d;                  // (double)(float)(r * r)
};

template <int NTH>
__global__ __launch_bounds__(NTH) void color_gradient_kernel(GradArgs a)
{
    extern __shared__ double lds_raw[];
    const long long t = (long long)blockIdx.x * NTH + threadIdx.x;
    if (t >= a.n) return;
    NnList L = nn_list_lds(lds_raw, threadIdx.x, NTH, a.cap);
    const NnQuery query = nn_query(a.view, t);
    nn_search<false>(a.view, query, L, nn_accept<false>(a.r2d));                 // flann radiusSearch: strict
    const Pt64 q = query.p;
    const int me = query.me;
    double x[3] = {0.0, 0.0, 0.0};
    if (L.cnt >= 3) {
        const double n[3] = {a.nrm[3ll * me], a.nrm[3ll * me + 1], a.nrm[3ll * me + 2]};
        const double it = a.inten[me];
        double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int j = 1; j < L.cnt; j++) {                          // :108-120
            const int id = L.id[(size_t)j * L.stride];
            const Pt64 p = a.view.pts[id];
            const double dot = (p.x - q.x) * n[0] + (p.y - q.y) * n[1] + (p.z - q.z) * n[2];
            const double r0 = (p.x - dot * n[0]) - q.x, r1 = (p.y - dot * n[1]) - q.y, r2 = (p.z - dot * n[2]) - q.z;
            const double rhs = a.inten[id] - it;
            m00 += r0 * r0; m01 += r0 * r1; m02 += r0 * r2; m11 += r1 * r1; m12 += r1 * r2; m22 += r2 * r2;
            b0 += r0 * rhs; b1 += r1 * rhs; b2 += r2 * rhs;
        }
        {
            const double w = (double)(L.cnt - 1);                  // :122-125, right side 0
            const double r0 = w * n[0], r1 = w * n[1], r2 = w * n[2];
            m00 += r0 * r0; m01 += r0 * r1; m02 += r0 * r2; m11 += r1 * r1; m12 += r1 * r2; m22 += r2 * r2;
        }
        const double det = m00 * (m11 * m22 - m12 * m12) - m01 * (m01 * m22 - m12 * m02) + m02 * (m01 * m12 - m11 * m02);
        if (!(fabs(det) < 1e-6) && isfinite(det)) {
            // M = L D L^T (no pivoting: M is a Gram matrix), then L y = b, D z = y, L^T x = z
            const double d0 = m00, l10 = m01 / d0, l20 = m02 / d0;
            const double d1 = m11 - l10 * m01;
            const double l21 = (m12 - l20 * m01) / d1;
            const double d2 = m22 - l20 * m02 - l21 * (l21 * d1);
            const double y0 = b0, y1 = b1 - l10 * y0, y2 = b2 - l20 * y0 - l21 * y1;
            x[2] = y2 / d2;
            x[1] = y1 / d1 - l21 * x[2];
            x[0] = y0 / d0 - l10 * x[1] - l20 * x[2];
        }
    }
    a.grad[3ll * me] = x[0];
    a.grad[3ll * me + 1] = x[1];
    a.grad[3ll * me + 2] = x[2];
}

}  // namespace

hipError_t color_gradient_on_device(const ColorGradientInput &in, double radius, int max_nn, double *d_grad, hipStream_t stream)
{
    const int64_t n = in.n;
    if (n <= 0) return hipSuccess;
    if (max_nn < 3 || max_nn > kNormalsMaxList || n > 0x7fffffff || !in.intensity || !d_grad) return hipErrorInvalidValue;
    if (!(radius > 0.0) || !std::isfinite(radius)) {             // no neighbours (KDTreeFlann.cpp:171-176): every gradient 0
        VISMA_TRY(hipMemsetAsync(d_grad, 0, sizeof(double) * 3 * (size_t)n, stream));
        return hipStreamSynchronize(stream);
    }
    NnGrid G;
    DevBufs B;
    double *d_nrm3 = nullptr;
    VISMA_TRY(G.alloc(n));
    if (!in.nrm) VISMA_TRY(B.alloc(&d_nrm3, 3 * (size_t)n));
    VISMA_TRY(G.build(in, d_nrm3, radius, 0, stream));
    GradArgs a{};
    a.view = G.view;
    a.nrm = in.nrm ? in.nrm : d_nrm3; a.inten = in.intensity; a.grad = d_grad;
    a.n = (int)n;
    a.cap = (int)std::min<int64_t>(max_nn, n);
    a.r2d = nn_radius2(radius);
    VISMA_TRY(nn_launch(a.cap, n, a, stream, [](auto nth) { return &color_gradient_kernel<decltype(nth)::value>; }));
    return hipStreamSynchronize(stream);                          // (the buffers of G and B go with this scope)
}

hipError_t color_gradient_device(const double *h_xyz, int64_t n, const double *h_nrm, const double *h_rgb, double radius,
                                 int max_nn, double *h_out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (max_nn < 3 || max_nn > kNormalsMaxList || n > 0x7fffffff) return hipErrorInvalidValue;
    std::vector<double> inten((size_t)n);
    for (int64_t i = 0; i < n; i++) inten[(size_t)i] = color_intensity(h_rgb + 3 * i);
    DevBufs B;
    double *d_xyz = nullptr, *d_nrm = nullptr, *d_int = nullptr, *d_out = nullptr;
    VISMA_TRY(B.alloc(&d_xyz, 3 * (size_t)n));
    VISMA_TRY(B.alloc(&d_nrm, 3 * (size_t)n));
    VISMA_TRY(B.alloc(&d_int, (size_t)n));
    VISMA_TRY(B.alloc(&d_out, 3 * (size_t)n));
    VISMA_TRY(hipMemcpyAsync(d_xyz, h_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    VISMA_TRY(hipMemcpyAsync(d_nrm, h_nrm, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    VISMA_TRY(hipMemcpyAsync(d_int, inten.data(), sizeof(double) * n, hipMemcpyHostToDevice, stream));
    ColorGradientInput in;
    in.xyz = d_xyz; in.nrm = d_nrm; in.intensity = d_int; in.n = n;
    nn_binning_origin(h_xyz, n, in.origin);
    VISMA_TRY(color_gradient_on_device(in, radius, max_nn, d_out, stream));
    VISMA_TRY(hipMemcpyAsync(h_out, d_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

}  // namespace visma
