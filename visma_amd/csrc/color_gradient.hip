// color_gradient.hip -- the colour gradient per target point of colored ICP (Park, Zhou, Koltun: "Colored Point Cloud
// Registration Revisited", ICCV 2017) on gfx950: the step the reference runs once per registration before its loop
// (O3D/Core/Registration/ColoredICP.cpp:74-137, InitializePointCloudForColoredICP).
//
// Per point k with normal n and intensity I_k: neighbours by the Hybrid search (radius, max_nn) in the order of the
// reference's result list -- the list, its order and the walk over the cells are nn_list.h's, shared with
// normals.hip --; fewer than 3 entries: the gradient is 0.  Else entry 0 is skipped whatever index it holds (the
// reference takes it for the point itself), every other entry a gives the row a' - p, a' = a - ((a - p).n) n its
// projection into the tangent plane, with the right side I_a - I_k, and one more row (nn - 1) n with right side 0 keeps
// the gradient in the plane.  A^T A (3 x 3) and A^T b are summed in f64 in list order; |det| < 1e-6 or a determinant
// that is not finite leaves 0 (Eigen.cpp:41-43), else the symmetric 3 x 3 is solved by its L D L^T factors written out.
//
// One thread per point, in cell order; lists of up to kNormalsMaxList entries in LDS: 12 bytes per entry and thread,
// so max_nn = 30 runs 128 threads on 45 KiB (3 workgroups per CU by LDS), max_nn = 170 runs 64 threads on 128 KiB of the
// 160 (one workgroup per CU) -- nn_list_threads.  A colour or a normal is never an index or an address: a non-finite
// one reaches the sums only.  (Reasoning and numbers: DESIGN.md 4.4c6.)
#include "nn_list.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace visma {

namespace {

struct GradArgs {
    const float4 *sorted;        // cell-sorted fp32 copy (cell binning only)
    const Pt64 *sorted64;        // cell-sorted points, w = original index
    const unsigned *start;
    GridParams g;
    const Pt64 *pts;             // original order
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
    const int tid = threadIdx.x;
    const long long t = (long long)blockIdx.x * NTH + tid;
    if (t >= a.n) return;
    NnList L = nn_list_lds(lds_raw, tid, NTH, a.cap);
    const Pt64 q = a.sorted64[t];                                 // queries in cell order
    const float4 qf = a.sorted[t];
    const GridParams g = a.g;
    const int cx = cell_coord(qf.x, g.mn[0], g.inv_h, g.dim[0]);
    const int cy = cell_coord(qf.y, g.mn[1], g.inv_hs, g.dim[1]);
    const int cz = cell_coord(qf.z, g.mn[2], g.inv_hs, g.dim[2]);
    auto consider = [&](const Pt64 &p) {
        const double d = nn_dist2(q, p);
        if (!(d < a.r2d)) return;                                 // flann radiusSearch: strict
        nn_list_insert(L, d, (int)p.w);
    };
    nn_scan_shell(g, a.start, a.sorted64, cx, cy, cz, 0, consider);
    nn_scan_shell(g, a.start, a.sorted64, cx, cy, cz, 1, consider);     // cells of edge 1.001 r: the 27 cover the radius
    const int me = (int)q.w;
    double x[3] = {0.0, 0.0, 0.0};
    if (L.cnt >= 3) {
        const double n[3] = {a.nrm[3ll * me], a.nrm[3ll * me + 1], a.nrm[3ll * me + 2]};
        const double it = a.inten[me];
        double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int j = 1; j < L.cnt; j++) {                          // :108-120
            const int id = L.id[(size_t)j * L.stride];
            const Pt64 p = a.pts[id];
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

// points and normals from whichever form the caller holds them in: n x 3 doubles, Pt64 or float4 (exactly one of each
// three).  The fp32 copy is used for BINNING only and is taken relative to `c` (normals.hip: pack_points_kernel).
__global__ void pack_gradient_input_kernel(ColorGradientInput in, float4 *__restrict__ f4, Pt64 *__restrict__ p8,
                                           double *__restrict__ nrm3)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.n) return;
    double x, y, z;
    if (in.xyz) { x = in.xyz[3 * i]; y = in.xyz[3 * i + 1]; z = in.xyz[3 * i + 2]; }
    else if (in.xyz64) { const Pt64 p = in.xyz64[i]; x = p.x; y = p.y; z = p.z; }
    else { const float4 p = in.xyz32[i]; x = (double)p.x; y = (double)p.y; z = (double)p.z; }
    f4[i] = make_float4((float)(x - in.origin[0]), (float)(y - in.origin[1]), (float)(z - in.origin[2]), __uint_as_float((unsigned)i));
    p8[i] = Pt64{x, y, z, (unsigned long long)i};
    if (in.nrm) return;                                           // (read in place)
    if (in.nrm64) { const Pt64 p = in.nrm64[i]; x = p.x; y = p.y; z = p.z; }
    else { const float4 p = in.nrm32[i]; x = (double)p.x; y = (double)p.y; z = (double)p.z; }
    nrm3[3 * i] = x; nrm3[3 * i + 1] = y; nrm3[3 * i + 2] = z;
}

struct GradBufs {
    std::vector<void *> ptrs;
    ~GradBufs() { for (void *p : ptrs) (void)hipFree(p); }
    template <class T>
    hipError_t alloc(T **out, size_t count)
    {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, sizeof(T) * std::max<size_t>(count, 1));
        if (e != hipSuccess) return e;
        ptrs.push_back(p);
        *out = (T *)p;
        return hipSuccess;
    }
};

template <int NTH>
hipError_t launch_gradient(const GradArgs &a, size_t lds, hipStream_t stream)
{
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)color_gradient_kernel<NTH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((color_gradient_kernel<NTH>), dim3((unsigned)((a.n + NTH - 1) / NTH)), dim3(NTH), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

#define GRAD_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

hipError_t color_gradient_on_device(const ColorGradientInput &in, double radius, int max_nn, double *d_grad, hipStream_t stream)
{
    const int64_t n = in.n;
    if (n <= 0) return hipSuccess;
    if (max_nn < 3 || max_nn > kNormalsMaxList || n > 0x7fffffff || !in.intensity || !d_grad) return hipErrorInvalidValue;
    if (!(radius > 0.0) || !std::isfinite(radius)) {             // no neighbours (KDTreeFlann.cpp:171-176): every gradient 0
        GRAD_TRY(hipMemsetAsync(d_grad, 0, sizeof(double) * 3 * (size_t)n, stream));
        return hipStreamSynchronize(stream);
    }
    GradBufs B;
    float4 *d_f4 = nullptr, *d_sorted = nullptr;
    Pt64 *d_p8 = nullptr, *d_sorted64 = nullptr;
    double *d_nrm3 = nullptr;
    unsigned *d_box = nullptr, *d_cell_of = nullptr, *d_count = nullptr, *d_start = nullptr, *d_bsum = nullptr;
    GRAD_TRY(B.alloc(&d_f4, (size_t)n));
    GRAD_TRY(B.alloc(&d_sorted, (size_t)n + kSortedSlack));
    GRAD_TRY(B.alloc(&d_p8, (size_t)n));
    GRAD_TRY(B.alloc(&d_sorted64, (size_t)n));
    GRAD_TRY(B.alloc(&d_box, 8));
    GRAD_TRY(B.alloc(&d_cell_of, 2 * (size_t)n));
    if (!in.nrm) GRAD_TRY(B.alloc(&d_nrm3, 3 * (size_t)n));
    hipLaunchKernelGGL(pack_gradient_input_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, d_f4, d_p8, d_nrm3);
    GRAD_TRY(hipGetLastError());
    GRAD_TRY(launch_grid_bbox(d_f4, n, d_box, stream));
    unsigned box[6];
    GRAD_TRY(hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, stream));
    GRAD_TRY(hipStreamSynchronize(stream));
    float mn[3], mx[3];
    grid_decode_bbox(box, mn, mx);
    const int64_t max_cells = std::min<int64_t>(kGridMaxCells, std::max<int64_t>(4096, 8 * n));
    const GridParams g = grid_plan(mn, mx, radius, max_cells);
    GRAD_TRY(B.alloc(&d_count, (size_t)g.ncell + 1));
    GRAD_TRY(B.alloc(&d_start, (size_t)g.ncell + 9));
    GRAD_TRY(B.alloc(&d_bsum, (size_t)grid_scan_blocks(g.ncell) + 1));
    GRAD_TRY(launch_grid_build(d_f4, n, g, d_cell_of, d_count, d_bsum, d_start, d_sorted, stream, d_p8, d_sorted64));
    GradArgs a{};
    a.sorted = d_sorted; a.sorted64 = d_sorted64; a.start = d_start; a.g = g; a.pts = d_p8;
    a.nrm = in.nrm ? in.nrm : d_nrm3; a.inten = in.intensity; a.grad = d_grad;
    a.n = (int)n;
    a.cap = (int)std::min<int64_t>(max_nn, n);
    const float r2f = (float)(radius * radius);
    a.r2d = (double)r2f;
    const int nth = nn_list_threads(a.cap);
    const size_t lds = nn_list_lds_bytes(a.cap, nth);
    if (nth == 256) GRAD_TRY(launch_gradient<256>(a, lds, stream));
    else if (nth == 128) GRAD_TRY(launch_gradient<128>(a, lds, stream));
    else GRAD_TRY(launch_gradient<64>(a, lds, stream));
    return hipStreamSynchronize(stream);                          // (the buffers of B go with this scope)
}

hipError_t color_gradient_device(const double *h_xyz, int64_t n, const double *h_nrm, const double *h_rgb, double radius,
                                 int max_nn, double *h_out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (max_nn < 3 || max_nn > kNormalsMaxList || n > 0x7fffffff) return hipErrorInvalidValue;
    std::vector<double> inten((size_t)n);
    for (int64_t i = 0; i < n; i++) inten[(size_t)i] = color_intensity(h_rgb + 3 * i);
    GradBufs B;
    double *d_xyz = nullptr, *d_nrm = nullptr, *d_int = nullptr, *d_out = nullptr;
    GRAD_TRY(B.alloc(&d_xyz, 3 * (size_t)n));
    GRAD_TRY(B.alloc(&d_nrm, 3 * (size_t)n));
    GRAD_TRY(B.alloc(&d_int, (size_t)n));
    GRAD_TRY(B.alloc(&d_out, 3 * (size_t)n));
    GRAD_TRY(hipMemcpyAsync(d_xyz, h_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    GRAD_TRY(hipMemcpyAsync(d_nrm, h_nrm, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream));
    GRAD_TRY(hipMemcpyAsync(d_int, inten.data(), sizeof(double) * n, hipMemcpyHostToDevice, stream));
    ColorGradientInput in;
    in.xyz = d_xyz; in.nrm = d_nrm; in.intensity = d_int; in.n = n;
    // a finite point of the cloud as the binning origin (normals.hip)
    for (int64_t i = 0; i < n; i++)
        if (std::isfinite(h_xyz[3 * i]) && std::isfinite(h_xyz[3 * i + 1]) && std::isfinite(h_xyz[3 * i + 2])) {
            in.origin[0] = h_xyz[3 * i]; in.origin[1] = h_xyz[3 * i + 1]; in.origin[2] = h_xyz[3 * i + 2];
            break;
        }
    GRAD_TRY(color_gradient_on_device(in, radius, max_nn, d_out, stream));
    GRAD_TRY(hipMemcpyAsync(h_out, d_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

}  // namespace visma
