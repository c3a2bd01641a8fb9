// colormap.hip -- color map optimization (Zhou and Koltun 2014; Open3D's ColorMapOptimization, rigid variant:
// Core/ColorMap/ColorMapOptimization.cpp) on gfx950: every camera's pose refined so that all images that see a vertex
// agree on its intensity, then the vertices re-coloured from the images.  One object (ColorMapDevice) holds the frames,
// the vertices and everything derived from them on the device.
//
//  images       per frame: RGB8 -> fp32 gray ((0.2990f R + 0.5870f G + 0.1140f B) / 255.0f), Gaussian3, Sobel3Dx, Sobel3Dy
//               through filter3_kernel of odometry_image.hip (the one 3-tap filter: bit for bit the reference's), then
//               {gray, dx, dy, 0} interleaved into ONE float4 texel per pixel: a corner of the bilinear samples of a visit is
//               one 16-byte load instead of three 4-byte loads from three planes.
//  masks        Sobel3Dx / Sobel3Dy of the raw depth, promoted to f64, sqrt(dx dx + dy dy) > threshold -> 255; a square
//               maximum of half-size k as a row pass and a column pass (neighbours outside the image are ignored).
//  visibility   one lane per (camera, vertex) through the count / scan / write compaction of compact.h: item c * nvp + v
//               (nvp: the vertex count padded to the tile), so that camera c's list is ascending in vertex id and starts at
//               the offset of its first tile.  The per-vertex view is a bit matrix, words x n_vertices (word-major: the
//               lanes of a wave read neighbouring words), bit c % 32 of word c / 32; its bits are set with integer OR.  A
//               vertex's cameras are read off it in ascending camera id: the order of every per-vertex sum is defined (the
//               reference's is a race).
//  proxy        one lane per vertex: over its cameras, the current pose's projection in the reference's fp32, the 10-pixel
//               margin, gray at the rounded pixel, the f64 mean.
//  iteration    ALL cameras in one launch: grid (blocks, cameras), a grid-stride loop over the camera's list, 29 f64
//               accumulators per thread (21 upper entries of JJ, 6 of Jb, rr, count), block_reduce_store + pair_pass_fold
//               with a ticket per camera into one row per camera.  No floating-point atomics; the order of every addition is
//               fixed by (blocks, list) alone.  What an iteration reads: the list (4 B per visit), the vertex (24 B), the
//               proxy (8 B), four texels (64 B); it never reads the bit matrix.  The 6 x 6 solve and the pose update run on
//               the host (host_math.hpp) with one read-back per iteration.
//  colours      one lane per vertex, as the proxy, from the RGB8 images.
// The non-rigid variant (a warping field per image) shares this object: its vertex passes are the WARP instantiations here,
// its iteration is colormap_warp.hip.
// (Reasoning: DESIGN.md 4.4c12, 4.4c13.)
#include "kernels.h"
#include "colormap_device.h"
#include "compact.h"
#include "device_common.h"
#include "host_math.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace visma {

namespace {

__global__ __launch_bounds__(kThreads) void cm_gray_kernel(const unsigned char *__restrict__ rgb, float *__restrict__ out, long long n)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned char *p = rgb + 3 * i;
    out[i] = (0.2990f * (float)p[0] + 0.5870f * (float)p[1] + 0.1140f * (float)p[2]) / 255.0f;
}

__global__ __launch_bounds__(kThreads) void cm_texel_kernel(const float *__restrict__ g, const float *__restrict__ dx,
                                                            const float *__restrict__ dy, float4 *__restrict__ out, long long n)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    out[i] = make_float4(g[i], dx[i], dy[i], 0.0f);
}

__global__ __launch_bounds__(kThreads) void cm_mask_kernel(const float *__restrict__ ddx, const float *__restrict__ ddy,
                                                           unsigned char *__restrict__ out, long long n, double threshold)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double dx = (double)ddx[i], dy = (double)ddy[i];
    const double mag = sqrt(dx * dx + dy * dy);
    out[i] = mag > threshold ? 255 : 0;
}

template <bool VERTICAL>
__global__ __launch_bounds__(kThreads) void cm_dilate_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out,
                                                             int w, int h, int k)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)w * h) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    const int at = VERTICAL ? y : x, end = VERTICAL ? h : w;
    const int lo = at - k > 0 ? at - k : 0, hi = at + k < end - 1 ? at + k : end - 1;   // k <= 64 (the driver): no overflow
    unsigned char m = 0;
    for (int q = lo; q <= hi; q++) {
        const unsigned char p = VERTICAL ? in[(long long)q * w + x] : in[(long long)y * w + q];
        if (p == 255) m = 255;
    }
    out[i] = m;
}

// Project3DPointAndGetUVDepth: Vt = E (X, Y, Z, 1) in f64, each row ((e0 X + e1 Y) + e2 Z) + e3, then the three casts
__device__ __forceinline__ void cm_project(const double *__restrict__ E, const CmCamera &K, double X, double Y, double Z, float *u,
                                           float *v, float *z)
{
    const double t0 = ((E[0] * X + E[1] * Y) + E[2] * Z) + E[3];
    const double t1 = ((E[4] * X + E[5] * Y) + E[6] * Z) + E[7];
    const double t2 = ((E[8] * X + E[9] * Y) + E[10] * Z) + E[11];
    *u = (float)((t0 * K.fx) / t2 + K.cx);
    *v = (float)((t1 * K.fy) / t2 + K.cy);
    *z = (float)t2;
}

// the compaction's Source: item i = c * nvp + v
struct VisibilitySource {
    const double *vertices;          // n_vertices x 3
    const double *extrinsics;        // n_cameras x 16, the poses of prepare
    const float *depth;              // n_cameras planes of w x h
    const unsigned char *mask;
    CmCamera K;
    long long nv, nvp;
    double max_depth, visibility_threshold;
    int32_t *list;                   // out: the cameras' lists, one after another
    unsigned *bits;                  // out: words x nv, zeroed before the write pass
    __device__ int count(long long i) const
    {
        const long long c = i / nvp, j = i - c * nvp;
        if (j >= nv) return 0;
        float u, v, z;
        cm_project(extrinsics + 16 * c, K, vertices[3 * j], vertices[3 * j + 1], vertices[3 * j + 2], &u, &v, &z);
        // (a NaN fails every comparison; beyond +-2^30 no pixel)
        if (!(z >= 0.0f) || !(fabsf(u) < 1073741824.0f) || !(fabsf(v) < 1073741824.0f) || !(fabsf(z) <= 3.0e38f)) return 0;
        const int ud = (int)roundf(u), vd = (int)roundf(v);
        if (ud < 0 || ud >= K.w || vd < 0 || vd >= K.h) return 0;
        const long long p = c * (long long)K.w * K.h + (long long)vd * K.w + ud;
        const float d = depth[p];
        if ((double)d > max_depth) return 0;
        if (mask[p] == 255) return 0;
        return (double)fabsf(z - d) < visibility_threshold ? 1 : 0;
    }
    __device__ void emit(long long i, long long row) const
    {
        const long long c = i / nvp, j = i - c * nvp;
        list[row] = (int32_t)j;
        atomicOr(bits + (c >> 5) * nv + j, 1u << (unsigned)(c & 31));
    }
};

inline unsigned cm_blocks(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

struct VertexPassArgs {
    const double *vertices, *extrinsics;
    const unsigned *bits;
    const float4 *texels;            // n_cameras planes
    const unsigned char *rgb;        // n_cameras planes of w x h x 3
    CmCamera K;
    long long nv;
    int words, n_cameras;
    double *out;                     // proxy: nv; colours: nv x 3
    const double *flow;              // WARP: n_cameras fields of 2 aw ah
    int aw, ah;
    double step;
};

// COLOR false: the proxy intensity; true: the colour average.  One lane per vertex, its cameras in ascending id.
// WARP (the non-rigid map): the pixel is the field's shift of (u, v), after a margin test of its own.
template <bool COLOR, bool WARP>
__global__ __launch_bounds__(kThreads) void cm_vertex_kernel(VertexPassArgs a)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j >= a.nv) return;
    const double X = a.vertices[3 * j], Y = a.vertices[3 * j + 1], Z = a.vertices[3 * j + 2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, cnt = 0.0;
    const long long plane = (long long)a.K.w * a.K.h;
    for (int wd = 0; wd < a.words; wd++) {
        unsigned m = a.bits[(long long)wd * a.nv + j];
        while (m) {
            const int b = __ffs((int)m) - 1;
            m &= m - 1u;
            const int c = wd * 32 + b;
            if (c >= a.n_cameras) break;
            float u, v, z;
            cm_project(a.extrinsics + 16 * c, a.K, X, Y, Z, &u, &v, &z);
            if (!cm_inside((double)u, (double)v, a.K)) continue;
            // inside the margin: the rounded pixel is inside the image
            long long p;
            if (WARP) {
                // 10 <= u < w - 10 puts (int)(u / step) in 0 .. aw - 2 (aw - 1 >= w / step): the clamp never acts
                const double du = (double)u, dv = (double)v;
                int ci = (int)(du / a.step), cj = (int)(dv / a.step);
                ci = ci < a.aw - 2 ? ci : a.aw - 2; cj = cj < a.ah - 2 ? cj : a.ah - 2;
                const double pp = (du - ci * a.step) / a.step, qq = (dv - cj * a.step) / a.step;
                double su, sv;
                cm_warp_shift(cm_warp_cell(a.flow + (long long)c * 2 * a.aw * a.ah, a.aw, ci, cj), pp, qq, &su, &sv);
                if (!cm_inside(su, sv, a.K)) continue;
                p = (long long)c * plane + (long long)(int)round(sv) * a.K.w + (int)round(su);
            } else {
                p = (long long)c * plane + (long long)(int)roundf(v) * a.K.w + (int)roundf(u);
            }
            if (COLOR) {
                const unsigned char *q = a.rgb + 3 * p;
                s0 += (double)((float)q[0] / 255.0f); s1 += (double)((float)q[1] / 255.0f); s2 += (double)((float)q[2] / 255.0f);
            } else {
                s0 += (double)a.texels[p].x;
            }
            cnt += 1.0;
        }
    }
    if (COLOR) {
        if (cnt > 0.0) { s0 /= cnt; s1 /= cnt; s2 /= cnt; }
        a.out[3 * j] = s0; a.out[3 * j + 1] = s1; a.out[3 * j + 2] = s2;
    } else {
        a.out[j] = cnt > 0.0 ? s0 / cnt : 0.0;
    }
}

constexpr int kCmAcc = 29;                               // 21 upper entries of JJ, 6 of Jb, rr, count

struct IterationArgs {
    const double *vertices, *extrinsics, *proxy;
    const float4 *texels;
    const int32_t *list;
    const long long *offsets;        // n_cameras + 1
    CmCamera K;
    double *partials;                // cameras x gridDim.x rows of kPairRow
    unsigned *tickets;               // one per camera, zero between launches
    double *sums;                    // out: cameras x kPairRow, the first kCmAcc used
};

// blockIdx.y: the camera; blockIdx.x strides over its list
__global__ __launch_bounds__(kPairThreads) void cm_iteration_kernel(IterationArgs a)
{
    __shared__ double f_tot[32];
    const int cam = blockIdx.y, tid = threadIdx.x;
    const double *P = a.extrinsics + 16 * cam;
    const double p0 = P[0], p1 = P[1], p2 = P[2], p3 = P[3], p4 = P[4], p5 = P[5], p6 = P[6], p7 = P[7], p8 = P[8], p9 = P[9], p10 = P[10],
                 p11 = P[11];
    const CmCamera K = a.K;
    const float4 *img = a.texels + (long long)cam * K.w * K.h;
    const long long begin = a.offsets[cam], end = a.offsets[cam + 1];
    double acc[kCmAcc];
#pragma unroll
    for (int k = 0; k < kCmAcc; k++) acc[k] = 0.0;
    for (long long at = begin + (long long)blockIdx.x * kPairThreads + tid; at < end; at += (long long)gridDim.x * kPairThreads) {
        const int j = a.list[at];
        const double X = a.vertices[3 * (long long)j], Y = a.vertices[3 * (long long)j + 1], Z = a.vertices[3 * (long long)j + 2];
        const double G0 = ((p0 * X + p1 * Y) + p2 * Z) + p3;
        const double G1 = ((p4 * X + p5 * Y) + p6 * Z) + p7;
        const double G2 = ((p8 * X + p9 * Y) + p10 * Z) + p11;
        // L = intr G with intr = [fx 0 cx 0; 0 fy cy 0; 0 0 1 0; 0 0 0 1]: the zero products add nothing
        const double u = (K.fx * G0 + K.cx * G2) / G2, v = (K.fy * G1 + K.cy * G2) / G2;
        if (!cm_inside(u, v, K)) continue;
        // FloatValueAt: inside the margin 0 <= (int)u <= w - 2 holds already; the clamp is the reference's
        int ui = (int)u, vi = (int)v;
        ui = ui < K.w - 2 ? ui : K.w - 2; ui = ui > 0 ? ui : 0;
        vi = vi < K.h - 2 ? vi : K.h - 2; vi = vi > 0 ? vi : 0;
        const double pu = u - (double)ui, pv = v - (double)vi;
        const float4 *q = img + (long long)vi * K.w + ui;
        const float4 t00 = q[0], t10 = q[1], t01 = q[K.w], t11 = q[K.w + 1];
        const double qu = 1 - pu, qv = 1 - pv;
        const double gray = ((double)t00.x * qv + (double)t01.x * pv) * qu + ((double)t10.x * qv + (double)t11.x * pv) * pu;
        const double dIdx = ((double)t00.y * qv + (double)t01.y * pv) * qu + ((double)t10.y * qv + (double)t11.y * pv) * pu;
        const double dIdy = ((double)t00.z * qv + (double)t01.z * pv) * qu + ((double)t10.z * qv + (double)t11.z * pv) * pu;
        const double invz = 1. / G2;
        const double v0 = dIdx * K.fx * invz, v1 = dIdy * K.fy * invz;
        const double v2 = -(v0 * G0 + v1 * G1) * invz;
        double C[6];
        C[0] = -G2 * v1 + G1 * v2;
        C[1] = G2 * v0 - G0 * v2;
        C[2] = -G1 * v0 + G0 * v1;
        C[3] = v0; C[4] = v1; C[5] = v2;
        const double r = a.proxy[j] - gray;
        int k = 0;
#pragma unroll
        for (int x = 0; x < 6; x++)
#pragma unroll
            for (int y = x; y < 6; y++) acc[k++] += C[x] * C[y];
#pragma unroll
        for (int x = 0; x < 6; x++) acc[21 + x] -= r * C[x];
        acc[27] += r * r;
        acc[28] += 1.0;
    }
    double *rows = a.partials + (long long)cam * gridDim.x * kPairRow;
    block_reduce_store<kCmAcc, kPairThreads / 64, false, kPairRow>(acc, rows, true);
    if (!pair_pass_fold<kCmAcc, kPairRow>(rows, a.tickets + cam, f_tot)) return;
    if (tid < kPairRow) a.sums[(long long)cam * kPairRow + tid] = tid < kCmAcc ? f_tot[tid] : 0.0;
}

}  // namespace

void color_map_device_destroy(ColorMapDevice *D) { delete D; }

static hipError_t cm_create_buffers(ColorMapDevice *D)
{
    const size_t n = (size_t)D->cfg.n_images, px = (size_t)D->plane;
    DEV_RESET(D->depth, n * px);
    DEV_RESET(D->rgb, n * px * 3);
    DEV_RESET(D->mask, n * px);
    DEV_RESET(D->texels, n * px);
    DEV_RESET(D->extrinsics, n * 16);
    DEV_RESET(D->extr0, n * 16);
    for (auto &t : D->tmp) DEV_RESET(t, px);
    for (auto &t : D->mtmp) DEV_RESET(t, px);
    DEV_RESET(D->offsets, n + 1);
    DEV_RESET(D->sums, n * kPairRow);
    DEV_RESET(D->tickets, n);
    VISMA_TRY(hipMemsetAsync(D->tickets, 0, sizeof(unsigned) * n, D->stream));
    if (D->cfg.anchors > 0) VISMA_TRY(color_map_warp_create(D));
    return hipStreamSynchronize(D->stream);
}

hipError_t color_map_device_create(const ColorMapConfig &cfg, hipStream_t stream, ColorMapDevice **out)
{
    ColorMapDevice *D = new ColorMapDevice;
    D->cfg = cfg; D->stream = stream;
    D->K = CmCamera{cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.w, cfg.h};
    D->plane = (long long)cfg.w * cfg.h;
    D->words = (cfg.n_images + 31) / 32;
    const hipError_t e = cm_create_buffers(D);
    if (e != hipSuccess) { delete D; return e; }
    D->host_extr.assign((size_t)cfg.n_images * 16, 0.0);
    *out = D;
    return hipSuccess;
}

// the frame's arrays are the caller's pageable memory: returns with the copies done
hipError_t color_map_device_set_image(ColorMapDevice *D, int i, const float *depth, const unsigned char *rgb, const double extrinsic[16])
{
    const size_t px = (size_t)D->plane;
    hipError_t e = hipMemcpyAsync(D->depth + (size_t)i * px, depth, sizeof(float) * px, hipMemcpyHostToDevice, D->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(D->rgb + (size_t)i * px * 3, rgb, px * 3, hipMemcpyHostToDevice, D->stream);
    if (e != hipSuccess) return e;
    std::memcpy(D->host_extr.data() + 16 * (size_t)i, extrinsic, sizeof(double) * 16);
    D->proxy_valid = false;
    return hipStreamSynchronize(D->stream);
}

hipError_t color_map_device_set_vertices(ColorMapDevice *D, const double *vertices, int64_t n)
{
    D->vertices.release(); D->proxy.release(); D->colors.release(); D->bits.release(); D->list.release();
    D->nv = n;
    D->nvp = (n + kThreads - 1) / kThreads * kThreads;
    D->proxy_valid = false;
    DEV_RESET(D->vertices, (size_t)n * 3);
    DEV_RESET(D->proxy, (size_t)n);
    DEV_RESET(D->colors, (size_t)n * 3);
    DEV_RESET(D->bits, (size_t)n * D->words);
    if (n > 0) VISMA_TRY(hipMemcpyAsync(D->vertices, vertices, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, D->stream));
    return hipStreamSynchronize(D->stream);
}

static hipError_t cm_upload_extrinsics(ColorMapDevice *D)
{
    return hipMemcpyAsync(D->extrinsics, D->host_extr.data(), sizeof(double) * D->host_extr.size(), hipMemcpyHostToDevice, D->stream);
}

// images, masks and visibility from the poses as they are now; counts[n_images]
hipError_t color_map_device_prepare(ColorMapDevice *D, int64_t *counts)
{
    static const float kGauss[3] = {0.25f, 0.5f, 0.25f}, kSobel1[3] = {-1.0f, 0.0f, 1.0f}, kSobel2[3] = {1.0f, 2.0f, 1.0f};
    const int w = D->cfg.w, h = D->cfg.h, n = D->cfg.n_images;
    const long long px = D->plane;
    hipStream_t s = D->stream;
    const dim3 grid(cm_blocks(px)), block(kThreads);
    // rows into tmp[0], columns into `out`
    auto filter = [&](const float *src, float *out, const float kx[3], const float ky[3]) {
        hipError_t e = launch_odo_filter3(src, D->tmp[0], w, h, kx[0], kx[1], kx[2], 0, s);
        return e != hipSuccess ? e : launch_odo_filter3(D->tmp[0], out, w, h, ky[0], ky[1], ky[2], 1, s);
    };
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; i++) {
        const float *depth = D->depth + (long long)i * px;
        hipLaunchKernelGGL(cm_gray_kernel, grid, block, 0, s, D->rgb + (long long)i * px * 3, D->tmp[1], px);
        e = filter(D->tmp[1], D->tmp[2], kGauss, kGauss);
        if (e == hipSuccess) e = filter(D->tmp[2], D->tmp[3], kSobel1, kSobel2);
        if (e == hipSuccess) e = filter(D->tmp[2], D->tmp[4], kSobel2, kSobel1);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(cm_texel_kernel, grid, block, 0, s, D->tmp[2], D->tmp[3], D->tmp[4], D->texels + (long long)i * px, px);
        e = filter(depth, D->tmp[3], kSobel1, kSobel2);
        if (e == hipSuccess) e = filter(depth, D->tmp[4], kSobel2, kSobel1);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(cm_mask_kernel, grid, block, 0, s, D->tmp[3], D->tmp[4], D->mtmp[0], px, D->cfg.discontinuity_threshold);
        hipLaunchKernelGGL(cm_dilate_kernel<false>, grid, block, 0, s, D->mtmp[0], D->mtmp[1], w, h, D->cfg.half_dilation);
        hipLaunchKernelGGL(cm_dilate_kernel<true>, grid, block, 0, s, D->mtmp[1], D->mask + (long long)i * px, w, h, D->cfg.half_dilation);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    e = cm_upload_extrinsics(D);
    if (e == hipSuccess) e = hipMemcpyAsync(D->extr0, D->extrinsics, sizeof(double) * 16 * (size_t)n, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(D->bits, 0, sizeof(unsigned) * (size_t)D->nv * D->words, s);
    if (e != hipSuccess) return e;

    VisibilitySource src;
    src.vertices = D->vertices; src.extrinsics = D->extr0; src.depth = D->depth; src.mask = D->mask; src.K = D->K;
    src.nv = D->nv; src.nvp = D->nvp; src.max_depth = D->cfg.max_depth; src.visibility_threshold = D->cfg.visibility_threshold;
    src.list = nullptr; src.bits = D->bits;
    const long long items = (long long)n * D->nvp;
    long long rows = 0;
    e = compact_count(D->compactor, src, items, s, &rows);
    if (e != hipSuccess) return e;
    DEV_RESET(D->list, (size_t)rows);
    src.list = D->list;
    e = compact_write(D->compactor, src, items, s);
    if (e != hipSuccess) return e;
    // camera c's list begins where its first tile does
    D->host_offsets.assign((size_t)n + 1, rows);
    const long long tiles_per_camera = D->nvp / kThreads;
    for (int c = 0; c < n && tiles_per_camera > 0 && e == hipSuccess; c++)
        e = hipMemcpyAsync(&D->host_offsets[(size_t)c], D->compactor.tile_offset.get() + c * tiles_per_camera, sizeof(long long),
                           hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    long long most = 0;
    for (int c = 0; c < n; c++) {
        counts[c] = D->host_offsets[(size_t)c + 1] - D->host_offsets[(size_t)c];
        most = std::max<long long>(most, counts[c]);
    }
    D->blocks = (int)std::min<long long>(std::max<long long>((most + kPairThreads - 1) / kPairThreads, 1), kColorMapMaxBlocks);
    DEV_RESET(D->partials, (size_t)n * D->blocks * kPairRow);
    e = hipMemcpyAsync(D->offsets, D->host_offsets.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && D->warp) e = color_map_warp_prepare(D);
    D->proxy_valid = false;
    return e;
}

// which: 0 gray, 1 dx, 2 dy (fp32), 3 mask (uint8)
hipError_t color_map_device_get_image(ColorMapDevice *D, int i, int which, void *out)
{
    const size_t px = (size_t)D->plane;
    if (which == 3) return hipMemcpy(out, D->mask + (size_t)i * px, px, hipMemcpyDeviceToHost);
    std::vector<float4> t(px);
    hipError_t e = hipMemcpy(t.data(), D->texels + (size_t)i * px, sizeof(float4) * px, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    float *o = (float *)out;
    for (size_t p = 0; p < px; p++) o[p] = which == 0 ? t[p].x : which == 1 ? t[p].y : t[p].z;
    return hipSuccess;
}

int64_t color_map_device_visible_count(const ColorMapDevice *D, int i)
{
    return D->host_offsets[(size_t)i + 1] - D->host_offsets[(size_t)i];
}

hipError_t color_map_device_get_visible(ColorMapDevice *D, int i, int32_t *out)
{
    const int64_t n = color_map_device_visible_count(D, i);
    if (n <= 0) return hipSuccess;
    return hipMemcpy(out, D->list + D->host_offsets[(size_t)i], sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost);
}

void color_map_device_get_extrinsics(const ColorMapDevice *D, double *out)
{
    std::memcpy(out, D->host_extr.data(), sizeof(double) * D->host_extr.size());
}

hipError_t color_map_device_set_extrinsics(ColorMapDevice *D, const double *in)
{
    std::memcpy(D->host_extr.data(), in, sizeof(double) * D->host_extr.size());
    D->proxy_valid = false;
    return hipSuccess;
}

static VertexPassArgs cm_vertex_args(ColorMapDevice *D, double *out)
{
    VertexPassArgs a;
    a.vertices = D->vertices; a.extrinsics = D->extrinsics; a.bits = D->bits; a.texels = D->texels; a.rgb = D->rgb; a.K = D->K;
    a.nv = D->nv; a.words = D->words; a.n_cameras = D->cfg.n_images; a.out = out;
    a.flow = D->flow; a.aw = D->aw; a.ah = D->ah; a.step = D->step;
    return a;
}

// the poses on the device and the proxies of them
hipError_t cm_refresh_proxy(ColorMapDevice *D)
{
    if (D->proxy_valid) return hipSuccess;
    hipError_t e = cm_upload_extrinsics(D);
    if (e == hipSuccess && D->warp) e = color_map_warp_upload_flow(D);
    if (e != hipSuccess) return e;
    if (D->nv > 0) {
        if (D->warp)
            hipLaunchKernelGGL((cm_vertex_kernel<false, true>), dim3(cm_blocks(D->nv)), dim3(kThreads), 0, D->stream, cm_vertex_args(D, D->proxy));
        else
            hipLaunchKernelGGL((cm_vertex_kernel<false, false>), dim3(cm_blocks(D->nv)), dim3(kThreads), 0, D->stream, cm_vertex_args(D, D->proxy));
        e = hipGetLastError();
    }
    // (the upload's source is host_extr: it must not change before the copy has run)
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    D->proxy_valid = e == hipSuccess;
    return e;
}

hipError_t color_map_device_get_proxy(ColorMapDevice *D, double *out)
{
    hipError_t e = cm_refresh_proxy(D);
    if (e != hipSuccess || D->nv == 0) return e;
    return hipMemcpy(out, D->proxy, sizeof(double) * (size_t)D->nv, hipMemcpyDeviceToHost);
}

// the 29 sums of every camera at the current poses: rows[n_images x kColorMapSums]
hipError_t color_map_device_sums(ColorMapDevice *D, double *rows)
{
    hipError_t e = cm_refresh_proxy(D);
    if (e != hipSuccess) return e;
    const int n = D->cfg.n_images;
    IterationArgs a;
    a.vertices = D->vertices; a.extrinsics = D->extrinsics; a.proxy = D->proxy; a.texels = D->texels; a.list = D->list;
    a.offsets = D->offsets; a.K = D->K; a.partials = D->partials; a.tickets = D->tickets; a.sums = D->sums;
    hipLaunchKernelGGL(cm_iteration_kernel, dim3((unsigned)D->blocks, (unsigned)n), dim3(kPairThreads), 0, D->stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    std::vector<double> host((size_t)n * kPairRow);
    e = hipMemcpyAsync(host.data(), D->sums, sizeof(double) * host.size(), hipMemcpyDeviceToHost, D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return e;
    for (int c = 0; c < n; c++) std::memcpy(rows + (size_t)c * kColorMapSums, host.data() + (size_t)c * kPairRow, sizeof(double) * kColorMapSums);
    return hipSuccess;
}

// one iteration: the sums, then per camera x = -JJ^-1 Jb and pose <- [Rz Ry Rx | t] pose on the host.  A camera with fewer
// than 6 accepted vertices, a singular JJ or a step that is not finite keeps its pose.  rr[n_images], count[n_images].
hipError_t color_map_device_step(ColorMapDevice *D, double *rr, int64_t *count)
{
    const int n = D->cfg.n_images;
    std::vector<double> rows((size_t)n * kColorMapSums);
    hipError_t e = color_map_device_sums(D, rows.data());
    if (e != hipSuccess) return e;
    for (int c = 0; c < n; c++) {
        const double *r = rows.data() + (size_t)c * kColorMapSums;
        rr[c] = r[27];
        count[c] = (int64_t)r[28];
        if (count[c] < 6) continue;
        double JJ[36], nb[6], x[6];
        int k = 0;
        for (int a = 0; a < 6; a++)
            for (int b = a; b < 6; b++) { JJ[a * 6 + b] = r[k]; JJ[b * 6 + a] = r[k]; k++; }
        for (int a = 0; a < 6; a++) nb[a] = -r[21 + a];
        const double det = solve6(JJ, nb, x);
        bool ok = det != 0.0 && std::isfinite(det);
        for (int a = 0; a < 6; a++) ok = ok && std::isfinite(x[a]);
        if (!ok) continue;
        double *P = D->host_extr.data() + 16 * (size_t)c;
        const Mat4 next = euler_zyx_to_mat4(x) * Mat4::from(P);
        std::memcpy(P, next.m, sizeof(next.m));
    }
    D->proxy_valid = false;
    return hipSuccess;
}

hipError_t color_map_device_get_colors(ColorMapDevice *D, double *out)
{
    hipError_t e = cm_upload_extrinsics(D);
    if (e == hipSuccess && D->warp) e = color_map_warp_upload_flow(D);
    if (e != hipSuccess) return e;
    if (D->nv == 0) return hipStreamSynchronize(D->stream);
    if (D->warp)
        hipLaunchKernelGGL((cm_vertex_kernel<true, true>), dim3(cm_blocks(D->nv)), dim3(kThreads), 0, D->stream, cm_vertex_args(D, D->colors));
    else
        hipLaunchKernelGGL((cm_vertex_kernel<true, false>), dim3(cm_blocks(D->nv)), dim3(kThreads), 0, D->stream, cm_vertex_args(D, D->colors));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, D->colors, sizeof(double) * 3 * (size_t)D->nv, hipMemcpyDeviceToHost, D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    return e;
}

}  // namespace visma
