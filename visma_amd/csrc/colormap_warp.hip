// colormap_warp.hip -- the NON-RIGID color map optimization (Zhou and Koltun 2014; Open3D's OptimizeImageCoorNonrigid,
// Core/ColorMap/ColorMapOptimization.cpp) on gfx950: besides its pose every image carries a bilinear warping field of
// anchor_w x anchor_h anchors, and an iteration refines both.  The device object, the images, the visibility and the
// compaction are colormap.hip's (colormap_device.h); the proxies and the colours are its vertex kernel's WARP instantiations.
//
//  field        anchor_h = number_of_vertical_anchors, step = double(h) / (anchor_h - 1), anchor_w = int(ceil(double(w) / step) + 1);
//               flow[(i + j anchor_w) 2 + {0, 1}] = {i step, j step}: the initial value and the regulariser's anchor.  The
//               fields live on the device (n x 2 aw ah doubles); host_flow is their copy.
//  visit        cm_warp_visit, ONE function for the keys and the rows: G, u, v as the rigid kernel; the cell (ii, jj) and p, q
//               from the doubles; (uu, vv) the field's shift; the margin test on it; gray, dx, dy there; the chain rule
//               through the field; C[14] and r.  A visit whose cell is out of range -- or whose u / step, v / step is not
//               finite or reaches 2^30, compared BEFORE the conversion to int -- is skipped (the reference indexes out of
//               bounds there).
//  keys         one lane per visit of the concatenated list: its cell, or `cells` for "rejected".
//  sort         by key within each camera, stable, one counting pass: a wave per tile of kWarpTile visits builds the tile's
//               histogram in LDS (bins = cells + 1 <= 8192: 32 KiB); one scan per camera over (bin, tile); a wave per tile
//               scatters its visits round by round (64 at a time, in list order) at base[key] + rank among the round's equal
//               keys.  A cell's visits end up in ascending vertex id: the order of every sum is defined.
//  reduce       one wave per (camera, cell).  In batches of 64 each lane computes one visit's row (C[14], -r, 1) into LDS;
//               then lane l owns accumulators l and l + 64 of the 121 -- each a product row[x] * row[y] -- and walks the
//               batch's visits in order.  The accumulators persist across batches: every sum is sequential in list order.
//               Rows go straight to cell_sums: no partial rows, no tickets, no atomics on floating point.
//  solve        on the host (colormap_solve.hpp): per camera a banded Cholesky with a border of six, up to 16 threads.
// (Reasoning: DESIGN.md 4.4c13.)
#include "colormap_device.h"
#include "colormap_solve.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace visma {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                         // the keys pass: the grid is capped and strides
constexpr int kScanThreads = 1024;
constexpr int kWarpTile = 1024;                          // visits per tile of the sort: 16 rounds of one wave
constexpr int kWarpRowStride = 17;                       // 16 doubles of a visit + 1: the lanes' rows start in different banks

struct WarpArgs {
    const double *vertices, *extrinsics, *proxy, *flow;
    const float4 *texels;
    const int32_t *list;
    const long long *offsets;        // n_cameras + 1
    CmCamera K;
    int aw, ah, cells, tiles;
    double step;
    int32_t *keys, *sorted;
    int *hist, *scan;                // n_cameras x bins x tiles
    double *cell_sums;
};

// One visit of camera `P` (its pose's first 12 entries) to vertex j -> its cell, or a.cells where it is skipped.
// ROW: row[0..13] = C, row[14] = -r, row[15] = 1.
template <bool ROW>
__device__ __forceinline__ int cm_warp_visit(const WarpArgs &a, const double *__restrict__ P, const double *__restrict__ flow,
                                             const float4 *__restrict__ img, int j, double *row)
{
    const CmCamera K = a.K;
    const double X = a.vertices[3 * (long long)j], Y = a.vertices[3 * (long long)j + 1], Z = a.vertices[3 * (long long)j + 2];
    const double G0 = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
    const double G1 = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
    const double G2 = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
    const double u = (K.fx * G0 + K.cx * G2) / G2, v = (K.fy * G1 + K.cy * G2) / G2;
    const double step = a.step;
    const double du = u / step, dv = v / step;
    // (a NaN fails; gfx950 saturates the conversion where x86-64 gives INT_MIN: the doubles are compared, not the ints)
    if (!(fabs(du) < 1073741824.0) || !(fabs(dv) < 1073741824.0)) return a.cells;
    const int ii = (int)du, jj = (int)dv;                // toward zero: u in (-step, 0) is cell 0 with p < 0
    if (ii < 0 || ii > a.aw - 2 || jj < 0 || jj > a.ah - 2) return a.cells;
    const double p = (u - ii * step) / step, q = (v - jj * step) / step;
    const CmWarpCell g = cm_warp_cell(flow, a.aw, ii, jj);
    double uu, vv;
    cm_warp_shift(g, p, q, &uu, &vv);
    if (!cm_inside(uu, vv, K)) return a.cells;
    const int cell = ii + jj * (a.aw - 1);
    if (!ROW) return cell;
    // FloatValueAt(uu, vv): the clamp is the reference's
    int ui = (int)uu, vi = (int)vv;
    ui = ui < K.w - 2 ? ui : K.w - 2; ui = ui > 0 ? ui : 0;
    vi = vi < K.h - 2 ? vi : K.h - 2; vi = vi > 0 ? vi : 0;
    const double pu = uu - (double)ui, pv = vv - (double)vi;
    const float4 *t = img + (long long)vi * K.w + ui;
    const float4 t00 = t[0], t10 = t[1], t01 = t[K.w], t11 = t[K.w + 1];
    const double qu = 1 - pu, qv = 1 - pv;
    const double gray = ((double)t00.x * qv + (double)t01.x * pv) * qu + ((double)t10.x * qv + (double)t11.x * pv) * pu;
    const double dIdfx = ((double)t00.y * qv + (double)t01.y * pv) * qu + ((double)t10.y * qv + (double)t11.y * pv) * pu;
    const double dIdfy = ((double)t00.z * qv + (double)t01.z * pv) * qu + ((double)t10.z * qv + (double)t11.z * pv) * pu;
    const double dfdx0 = ((g.x10 - g.x00) * (1 - q) + (g.x11 - g.x01) * q) / step;
    const double dfdx1 = ((g.y10 - g.y00) * (1 - q) + (g.y11 - g.y01) * q) / step;
    const double dfdy0 = ((g.x01 - g.x00) * (1 - p) + (g.x11 - g.x10) * p) / step;
    const double dfdy1 = ((g.y01 - g.y00) * (1 - p) + (g.y11 - g.y10) * p) / step;
    const double dIdx = dIdfx * dfdx0 + dIdfy * dfdx1, dIdy = dIdfx * dfdy0 + dIdfy * dfdy1;
    const double invz = 1. / G2;
    const double v0 = dIdx * K.fx * invz, v1 = dIdy * K.fy * invz;
    const double v2 = -(v0 * G0 + v1 * G1) * invz;
    row[0] = -G2 * v1 + G1 * v2;
    row[1] = G2 * v0 - G0 * v2;
    row[2] = -G1 * v0 + G0 * v1;
    row[3] = v0; row[4] = v1; row[5] = v2;
    row[6] = dIdfx * (1 - p) * (1 - q); row[7] = dIdfy * (1 - p) * (1 - q);
    row[8] = dIdfx * (1 - p) * q; row[9] = dIdfy * (1 - p) * q;
    row[10] = dIdfx * p * (1 - q); row[11] = dIdfy * p * (1 - q);
    row[12] = dIdfx * p * q; row[13] = dIdfy * p * q;
    row[14] = -(a.proxy[j] - gray);
    row[15] = 1.0;
    return cell;
}

// blockIdx.y: the camera; blockIdx.x strides over its list
__global__ __launch_bounds__(kThreads) void cm_warp_keys_kernel(WarpArgs a)
{
    const int cam = blockIdx.y;
    const double *P = a.extrinsics + 16 * cam;
    const double *flow = a.flow + (long long)cam * 2 * a.aw * a.ah;
    const long long begin = a.offsets[cam], end = a.offsets[cam + 1];
    for (long long at = begin + (long long)blockIdx.x * kThreads + threadIdx.x; at < end; at += (long long)gridDim.x * kThreads)
        a.keys[at] = cm_warp_visit<false>(a, P, flow, nullptr, a.list[at], nullptr);
}

// one wave per (tile, camera): the tile's histogram over bins = cells + 1, to hist[(cam bins + bin) tiles + tile]
__global__ __launch_bounds__(64) void cm_warp_hist_kernel(WarpArgs a)
{
    extern __shared__ int lds_bins[];
    const int cam = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x, bins = a.cells + 1;
    for (int b = lane; b < bins; b += 64) lds_bins[b] = 0;
    __syncthreads();
    const long long end = a.offsets[cam + 1];
    const long long first = a.offsets[cam] + (long long)tile * kWarpTile;
    for (int r = 0; r < kWarpTile / 64; r++) {
        const long long at = first + r * 64 + lane;
        if (at < end) atomicAdd(&lds_bins[a.keys[at]], 1);          // (integers: the order does not matter)
    }
    __syncthreads();
    int *out = a.hist + (long long)cam * bins * a.tiles + tile;
    for (int b = lane; b < bins; b += 64) out[(long long)b * a.tiles] = lds_bins[b];
}

// one workgroup per camera: the exclusive scan of its bins x tiles counts, chunk by chunk with a carry
__global__ __launch_bounds__(kScanThreads) void cm_warp_scan_kernel(WarpArgs a)
{
    __shared__ int buf[kScanThreads];
    __shared__ int carry;
    const long long n = (long long)(a.cells + 1) * a.tiles;
    const int *in = a.hist + (long long)blockIdx.x * n;
    int *out = a.scan + (long long)blockIdx.x * n;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long at = 0; at < n; at += kScanThreads) {
        const long long i = at + threadIdx.x;
        const int v = i < n ? in[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kScanThreads; o <<= 1) {                     // Hillis-Steele, inclusive
            const int add = (int)threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n) out[i] = carry + buf[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == kScanThreads - 1) carry += buf[threadIdx.x];
        __syncthreads();
    }
}

// one wave per (tile, camera): round by round in list order, a visit goes to base[key] + its rank among the round's equal keys
__global__ __launch_bounds__(64) void cm_warp_scatter_kernel(WarpArgs a)
{
    extern __shared__ int lds_bins[];
    const int cam = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x, bins = a.cells + 1;
    const int *scan = a.scan + (long long)cam * bins * a.tiles + tile;
    for (int b = lane; b < bins; b += 64) lds_bins[b] = scan[(long long)b * a.tiles];
    __syncthreads();
    const long long begin = a.offsets[cam], end = a.offsets[cam + 1];
    const long long first = begin + (long long)tile * kWarpTile;
    const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
    for (int r = 0; r < kWarpTile / 64; r++) {
        const long long at = first + r * 64 + lane;
        const bool active = at < end;
        const int key = active ? a.keys[at] : -1;
        int pos = 0;
        unsigned long long todo = __ballot(active);
        while (todo) {                                               // (uniform: every lane sees the same ballot)
            const int leader = __ffsll((long long)todo) - 1;
            const int kk = __shfl(key, leader, 64);
            const bool mine = active && key == kk;
            const unsigned long long m = __ballot(mine);
            const int base = lds_bins[kk];
            if (mine) pos = base + __popcll(m & below);
            if (lane == leader) lds_bins[kk] = base + __popcll(m);
            todo &= ~m;
        }
        if (active) a.sorted[begin + pos] = a.list[at];
        __syncthreads();
    }
}

// accumulator k of the 121 as a product row[x] * row[y]: the 105 upper entries of C C^T row by row, -r C, r r, 1
__device__ __forceinline__ void cm_warp_pair(int k, int *x, int *y)
{
    if (k >= 120) { *x = 15; *y = 15; return; }
    if (k == 119) { *x = 14; *y = 14; return; }
    if (k >= 105) { *x = 14; *y = k - 105; return; }
    int r = 0;
    while (k >= 14 - r) { k -= 14 - r; r++; }
    *x = r; *y = r + k;
}

// one wave per (cell, camera)
__global__ __launch_bounds__(64) void cm_warp_reduce_kernel(WarpArgs a)
{
    __shared__ double rows[64 * kWarpRowStride];
    const int cam = blockIdx.y, cell = blockIdx.x, lane = threadIdx.x;
    const int *scan = a.scan + (long long)cam * (a.cells + 1) * a.tiles;
    const long long begin = a.offsets[cam];
    const long long from = begin + scan[(long long)cell * a.tiles], to = begin + scan[(long long)(cell + 1) * a.tiles];
    const double *P = a.extrinsics + 16 * cam;
    const double *flow = a.flow + (long long)cam * 2 * a.aw * a.ah;
    const float4 *img = a.texels + (long long)cam * a.K.w * a.K.h;
    int x0, y0, x1, y1;
    cm_warp_pair(lane, &x0, &y0);
    cm_warp_pair(lane + 64 < kCmWarpRow ? lane + 64 : kCmWarpRow - 1, &x1, &y1);
    double acc0 = 0.0, acc1 = 0.0;
    for (long long at = from; at < to; at += 64) {
        double *mine = rows + lane * kWarpRowStride;
        if (at + lane < to) {
            double row[16];
            const int got = cm_warp_visit<true>(a, P, flow, img, a.sorted[at + lane], row);
            // (the key kernel ran this very function on these very inputs: got == cell.  Were it not, the visit adds nothing.)
#pragma unroll
            for (int k = 0; k < 16; k++) mine[k] = got == cell ? row[k] : 0.0;
        }
        __syncthreads();
        const int n = to - at < 64 ? (int)(to - at) : 64;
        for (int t = 0; t < n; t++) {
            const double *r = rows + t * kWarpRowStride;
            acc0 += r[x0] * r[y0];
            acc1 += r[x1] * r[y1];
        }
        __syncthreads();
    }
    double *out = a.cell_sums + ((long long)cam * a.cells + cell) * kCmWarpRow;
    out[lane] = acc0;
    if (lane + 64 < kCmWarpRow) out[lane + 64] = acc1;
}

}  // namespace

hipError_t color_map_warp_create(ColorMapDevice *D)
{
    D->warp = true;
    cm_warp_shape(D->cfg.w, D->cfg.h, D->cfg.anchors, &D->aw, &D->ah, &D->step);
    const size_t A = (size_t)D->aw * D->ah, n = (size_t)D->cfg.n_images;
    D->host_flow_init.resize(A * 2);
    for (int i = 0; i < D->aw; i++)
        for (int j = 0; j < D->ah; j++) {
            D->host_flow_init[((size_t)i + (size_t)j * D->aw) * 2] = i * D->step;
            D->host_flow_init[((size_t)i + (size_t)j * D->aw) * 2 + 1] = j * D->step;
        }
    D->host_flow.resize(n * A * 2);
    for (size_t c = 0; c < n; c++) std::memcpy(D->host_flow.data() + c * A * 2, D->host_flow_init.data(), sizeof(double) * A * 2);
    DEV_RESET(D->flow, n * A * 2);
    DEV_RESET(D->cell_sums, n * (size_t)(D->aw - 1) * (D->ah - 1) * kCmWarpRow);
    return hipSuccess;
}

// behind colormap.hip's prepare: the sort's buffers for the lists as they are now
hipError_t color_map_warp_prepare(ColorMapDevice *D)
{
    D->keys.release(); D->sorted.release(); D->hist.release(); D->hist_scan.release();   // (all four go before the first comes)
    const int n = D->cfg.n_images;
    long long most = 0;
    for (int c = 0; c < n; c++) most = std::max<long long>(most, D->host_offsets[(size_t)c + 1] - D->host_offsets[(size_t)c]);
    D->warp_rows = D->host_offsets[(size_t)n];
    D->warp_tiles = std::max<long long>((most + kWarpTile - 1) / kWarpTile, 1);
    const size_t bins = (size_t)(D->aw - 1) * (D->ah - 1) + 1;
    DEV_RESET(D->keys, (size_t)D->warp_rows);
    DEV_RESET(D->sorted, (size_t)D->warp_rows);
    DEV_RESET(D->hist, (size_t)n * bins * (size_t)D->warp_tiles);
    DEV_RESET(D->hist_scan, (size_t)n * bins * (size_t)D->warp_tiles);
    return hipSuccess;
}

hipError_t color_map_warp_upload_flow(ColorMapDevice *D)
{
    return hipMemcpyAsync(D->flow, D->host_flow.data(), sizeof(double) * D->host_flow.size(), hipMemcpyHostToDevice, D->stream);
}

hipError_t color_map_device_get_flow(const ColorMapDevice *D, double *out)
{
    if (!D->warp) return hipErrorInvalidValue;
    std::memcpy(out, D->host_flow.data(), sizeof(double) * D->host_flow.size());
    return hipSuccess;
}

hipError_t color_map_device_set_flow(ColorMapDevice *D, const double *in)
{
    if (!D->warp) return hipErrorInvalidValue;
    std::memcpy(D->host_flow.data(), in, sizeof(double) * D->host_flow.size());
    D->proxy_valid = false;
    return hipSuccess;
}

// keys, sort, reduce on the stream; the rows stay on the device
static hipError_t cm_warp_launch(ColorMapDevice *D)
{
    hipError_t e = cm_refresh_proxy(D);                  // (poses and fields on the device, the proxies of them)
    if (e != hipSuccess) return e;
    const int n = D->cfg.n_images;
    WarpArgs a;
    a.vertices = D->vertices; a.extrinsics = D->extrinsics; a.proxy = D->proxy; a.flow = D->flow; a.texels = D->texels;
    a.list = D->list; a.offsets = D->offsets; a.K = D->K; a.aw = D->aw; a.ah = D->ah; a.cells = (D->aw - 1) * (D->ah - 1);
    a.tiles = (int)D->warp_tiles; a.step = D->step; a.keys = D->keys; a.sorted = D->sorted; a.hist = D->hist; a.scan = D->hist_scan;
    a.cell_sums = D->cell_sums;
    const unsigned tiles = (unsigned)D->warp_tiles, cams = (unsigned)n;
    const size_t lds = sizeof(int) * (size_t)(a.cells + 1);
    const unsigned key_blocks = (unsigned)std::min<long long>((D->warp_tiles * kWarpTile + kThreads - 1) / kThreads, kMaxBlocks);
    hipLaunchKernelGGL(cm_warp_keys_kernel, dim3(key_blocks, cams), dim3(kThreads), 0, D->stream, a);
    hipLaunchKernelGGL(cm_warp_hist_kernel, dim3(tiles, cams), dim3(64), lds, D->stream, a);
    hipLaunchKernelGGL(cm_warp_scan_kernel, dim3(cams), dim3(kScanThreads), 0, D->stream, a);
    hipLaunchKernelGGL(cm_warp_scatter_kernel, dim3(tiles, cams), dim3(64), lds, D->stream, a);
    hipLaunchKernelGGL(cm_warp_reduce_kernel, dim3((unsigned)a.cells, cams), dim3(64), 0, D->stream, a);
    return hipGetLastError();
}

hipError_t color_map_device_cell_sums(ColorMapDevice *D, double *rows)
{
    if (!D->warp) return hipErrorInvalidValue;
    hipError_t e = cm_warp_launch(D);
    if (e != hipSuccess) return e;
    const size_t count = (size_t)D->cfg.n_images * (size_t)(D->aw - 1) * (D->ah - 1) * kCmWarpRow;
    e = hipMemcpyAsync(rows, D->cell_sums, sizeof(double) * count, hipMemcpyDeviceToHost, D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    return e;
}

// one iteration: the cell rows, then per camera the banded solve on the host, pose <- [Rz Ry Rx | t] pose and
// flow += x[6:].  A camera that keeps (colormap_solve.hpp) moves neither.
hipError_t color_map_device_step_non_rigid(ColorMapDevice *D, double *rr, double *rr_reg, int64_t *count)
{
    if (!D->warp) return hipErrorInvalidValue;
    const int n = D->cfg.n_images;
    const size_t A2 = (size_t)D->aw * D->ah * 2;
    std::vector<double> rows((size_t)n * (size_t)(D->aw - 1) * (D->ah - 1) * kCmWarpRow), x((size_t)n * (6 + A2));
    std::vector<char> moved((size_t)n);
    hipError_t e = color_map_device_cell_sums(D, rows.data());
    if (e != hipSuccess) return e;
    cm_warp_solve_all(n, kCmWarpMaxThreads, D->aw, D->ah, rows.data(), (double)D->nv, D->cfg.anchor_weight, D->host_flow.data(),
                      D->host_flow_init.data(), x.data(), rr, rr_reg, count, moved.data());
    for (int c = 0; c < n; c++) {
        if (!moved[(size_t)c]) continue;
        const double *xc = x.data() + (size_t)c * (6 + A2);
        double *P = D->host_extr.data() + 16 * (size_t)c;
        const Mat4 next = euler_zyx_to_mat4(xc) * Mat4::from(P);
        std::memcpy(P, next.m, sizeof(next.m));
        double *f = D->host_flow.data() + (size_t)c * A2;
        for (size_t d = 0; d < A2; d++) f[d] += xc[6 + d];
    }
    D->proxy_valid = false;
    return hipSuccess;
}

}  // namespace visma
