// cloud.hip -- open3d::PointCloud on the device (visma_icp_cloud_*): points and, optionally, normals and colours as n x 3 f64
// rows that stay resident between Transform, NormalizeNormals, PaintUniformColor, operator+=, GetMinBound / GetMaxBound,
// SelectDownSample, UniformDownSample, CropPointCloud, VoxelDownSample, EstimateNormals, the two OrientNormals*,
// ComputePointCloudMeanAndCovariance and ComputePointCloudMahalanobisDistance (Core/Geometry/PointCloud.cpp :47-198,
// DownSample.cpp :90-105, :222-254, EstimateNormals.cpp :158-204).  f64, one operation per rounding (the build's
// -ffp-contract=off), correctly rounded sqrt and division.  No floating-point atomics; one writer per output row.
//   rows_transform, rows_normalize  row_kernels.h, shared with trimesh.hip
//   cl_bounds_*             a reduction over (value, index) pairs: NaN values never enter, the smaller (larger) value wins and,
//                           among equal values (-0.0 == 0.0), the lower index: std::min_element's answer in any order of the
//                           reduction.  Point 0 is the exception the final step applies: its NaN is the result
//   InsideSource            CropPointCloud as compact.h's ordered compaction: the kept rows in their order
//   cl_gather, cl_every_k   SelectDownSample, UniformDownSample: one lane per output row
//   cl_first_finite         the index of the first point with three finite coordinates (an integer min): EstimateNormals'
//                           binning origin, which the host-array entry point reads from the host array
//   cl_cumulant_chunks ...  the nine cumulants: one lane per chunk of `chunk` consecutive points sums serially, one lane adds
//                           the chunk sums in chunk order, divides and forms mean and covariance
//   cl_mahalanobis          sqrt((p^T C^-1) p) per point, Eigen's order of the coefficient products
// The passes are streaming: grid-capped stride loops of 256 lanes (compact.h's shape).
#include "compact.h"
#include "dev_mem.h"
#include "kernels.h"
#include "row_kernels.h"

#include <math.h>

#include <algorithm>
#include <climits>
#include <memory>

namespace visma {

namespace {

__global__ __launch_bounds__(kThreads) void cl_fill(double *a, long long n, double x, double y, double z)
{
    ROW_LOOP(i, n) { a[3 * i] = x; a[3 * i + 1] = y; a[3 * i + 2] = z; }
}

// dst row i = src row idx[i]; every index has been checked on the host
__global__ __launch_bounds__(kThreads) void cl_gather(const double *src, const long long *idx, double *dst, long long rows)
{
    ROW_LOOP(i, rows) {
        const long long j = idx[i];
        dst[3 * i] = src[3 * j]; dst[3 * i + 1] = src[3 * j + 1]; dst[3 * i + 2] = src[3 * j + 2];
    }
}

// dst row i = src row i k; rows = ceil(n / k), so i k < n
__global__ __launch_bounds__(kThreads) void cl_every_k(const double *src, long long k, double *dst, long long rows)
{
    ROW_LOOP(i, rows) {
        const long long j = i * k;
        dst[3 * i] = src[3 * j]; dst[3 * i + 1] = src[3 * j + 1]; dst[3 * i + 2] = src[3 * j + 2];
    }
}

// DownSample.cpp:247-249: a NaN fails every comparison, in the point and in the bound
struct InsideSource {
    const double *p, *nrm, *col;
    double lo[3], hi[3];
    double *op, *onrm, *ocol;
    __device__ int count(long long i) const
    {
        const double *q = p + 3 * i;
        return q[0] >= lo[0] && q[0] <= hi[0] && q[1] >= lo[1] && q[1] <= hi[1] && q[2] >= lo[2] && q[2] <= hi[2];
    }
    __device__ void emit(long long i, long long row) const
    {
        for (int k = 0; k < 3; k++) op[3 * row + k] = p[3 * i + k];
        if (nrm) for (int k = 0; k < 3; k++) onrm[3 * row + k] = nrm[3 * i + k];
        if (col) for (int k = 0; k < 3; k++) ocol[3 * row + k] = col[3 * i + k];
    }
};

// ---- bounds: slots 0 .. 2 the minimum of x, y, z, slots 3 .. 5 the maximum; index < 0: no candidate yet ------------------
struct Extremes { double v[6]; int i[6]; };

__device__ __forceinline__ void ext_take(Extremes &e, int slot, double v, int i)
{
    if (i < 0) return;
    const bool better = slot < 3 ? v < e.v[slot] : v > e.v[slot];
    if (e.i[slot] < 0 || better || (v == e.v[slot] && i < e.i[slot])) { e.v[slot] = v; e.i[slot] = i; }
}

// the workgroup's extremes in thread 0
__device__ __forceinline__ void ext_reduce_block(Extremes &e)
{
    __shared__ double sv[kThreads / 64][6];
    __shared__ int si[kThreads / 64][6];
    for (int s = 0; s < 6; s++)
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_down(e.v[s], o, 64);
            const int oi = __shfl_down(e.i[s], o, 64);
            ext_take(e, s, ov, oi);
        }
    if ((threadIdx.x & 63) == 0)
        for (int s = 0; s < 6; s++) { sv[threadIdx.x >> 6][s] = e.v[s]; si[threadIdx.x >> 6][s] = e.i[s]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kThreads / 64; w++)
            for (int s = 0; s < 6; s++) ext_take(e, s, sv[w][s], si[w][s]);
}

__global__ __launch_bounds__(kThreads) void cl_bounds_partial(const double *p, long long n, double *part_v, int *part_i)
{
    Extremes e;
    for (int s = 0; s < 6; s++) { e.v[s] = 0.0; e.i[s] = -1; }
    ROW_LOOP(i, n)
        for (int a = 0; a < 3; a++) {
            const double v = p[3 * i + a];
            const int idx = isnan(v) ? -1 : (int)i;
            ext_take(e, a, v, idx);
            ext_take(e, 3 + a, v, idx);
        }
    ext_reduce_block(e);
    if (threadIdx.x == 0)
        for (int s = 0; s < 6; s++) { part_v[6 * blockIdx.x + s] = e.v[s]; part_i[6 * blockIdx.x + s] = e.i[s]; }
}

// ONE workgroup over the partial rows; std::min_element keeps its first element where nothing compares less: a NaN there
__global__ __launch_bounds__(kThreads) void cl_bounds_final(const double *part_v, const int *part_i, int parts, const double *p, double *out)
{
    Extremes e;
    for (int s = 0; s < 6; s++) { e.v[s] = 0.0; e.i[s] = -1; }
    for (int b = threadIdx.x; b < parts; b += kThreads)
        for (int s = 0; s < 6; s++) ext_take(e, s, part_v[6 * b + s], part_i[6 * b + s]);
    ext_reduce_block(e);
    if (threadIdx.x == 0)
        for (int s = 0; s < 6; s++) out[s] = isnan(p[s % 3]) ? p[s % 3] : e.v[s];
}

// *first = min(*first, the lowest index of a point with three finite coordinates)
__global__ __launch_bounds__(kThreads) void cl_first_finite(const double *p, long long n, int *first)
{
    int m = INT_MAX;
    ROW_LOOP(i, n)
        if (isfinite(p[3 * i]) && isfinite(p[3 * i + 1]) && isfinite(p[3 * i + 2])) m = min(m, (int)i);
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m != INT_MAX) atomicMin(first, m);
}

// ---- mean and covariance (PointCloud.cpp:151-178) ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cl_cumulant_chunks(const double *__restrict__ p, long long n, long long chunk, double *__restrict__ part)
{
    const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long lo = ch * chunk;
    if (lo >= n) return;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = lo; i < hi; i++) {
        const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        c[0] += x; c[1] += y; c[2] += z;
        c[3] += x * x; c[4] += x * y; c[5] += x * z;
        c[6] += y * y; c[7] += y * z; c[8] += z * z;
    }
    for (int k = 0; k < 9; k++) part[9 * ch + k] = c[k];
}

// out: mean (3), covariance (9, row-major)
__global__ __launch_bounds__(64) void cl_cumulant_combine(const double *__restrict__ part, long long nch, long long n, double *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long ch = 0; ch < nch; ch++)
        for (int k = 0; k < 9; k++) c[k] += part[9 * ch + k];
    for (int k = 0; k < 9; k++) c[k] /= (double)n;
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    out[3] = c[3] - c[0] * c[0];
    out[7] = c[6] - c[1] * c[1];
    out[11] = c[8] - c[2] * c[2];
    out[4] = out[6] = c[4] - c[0] * c[1];
    out[5] = out[9] = c[5] - c[0] * c[2];
    out[8] = out[10] = c[7] - c[1] * c[2];
}

// PointCloud.cpp:194-195.  Eigen evaluates p^T * C^-1 into a row first (r_j = (p_0 C_0j + p_1 C_1j) + p_2 C_2j), then its
// product with p; the three-term sums associate as the compiled reference's do (tests/golden/cloud.npz decides)
struct MahalanobisArgs { double mean[3], inv[9]; };
__global__ __launch_bounds__(kThreads) void cl_mahalanobis(const double *p, long long n, MahalanobisArgs a, double *out)
{
    ROW_LOOP(i, n) {
        const double x = p[3 * i] - a.mean[0], y = p[3 * i + 1] - a.mean[1], z = p[3 * i + 2] - a.mean[2];
        const double r0 = (x * a.inv[0] + y * a.inv[3]) + z * a.inv[6];
        const double r1 = (x * a.inv[1] + y * a.inv[4]) + z * a.inv[7];
        const double r2 = (x * a.inv[2] + y * a.inv[5]) + z * a.inv[8];
        out[i] = sqrt((r0 * x + r1 * y) + r2 * z);
    }
}

// ---- OrientNormals* (EstimateNormals.cpp:168-175, :188-202); norm() == 0.0 is sqrt((x x + y y) + z z) == 0.0 -------------------
__device__ __forceinline__ double cl_norm(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__global__ __launch_bounds__(kThreads) void cl_orient(const double *p, double *nrm, long long n, bool camera, double rx, double ry, double rz)
{
    ROW_LOOP(i, n) {
        double x = nrm[3 * i], y = nrm[3 * i + 1], z = nrm[3 * i + 2];
        double ox = rx, oy = ry, oz = rz;
        if (camera) { ox = rx - p[3 * i]; oy = ry - p[3 * i + 1]; oz = rz - p[3 * i + 2]; }
        if (cl_norm(x, y, z) == 0.0) {
            x = ox; y = oy; z = oz;
            if (camera) {
                if (cl_norm(x, y, z) == 0.0) {
                    x = 0.0; y = 0.0; z = 1.0;
                } else {                                     // normalize(): z = squaredNorm(); if (z > 0) /= sqrt(z)
                    const double n2 = (x * x + y * y) + z * z;
                    if (n2 > 0.0) {
                        const double len = sqrt(n2);
                        x = x / len; y = y / len; z = z / len;
                    }
                }
            }
        } else if ((x * ox + y * oy) + z * oz < 0.0) {
            x = x * -1.0; y = y * -1.0; z = z * -1.0;
        }
        nrm[3 * i] = x; nrm[3 * i + 1] = y; nrm[3 * i + 2] = z;
    }
}

}  // namespace

struct CloudDevice {
    int64_t n = 0;
    bool has_n = false, has_c = false;                     // the reference's HasNormals(), HasColors(): never set on no rows
    DeviceBuf<double> p, nrm, col;
    // what a call works in: grow-only
    Compactor comp;
    DeviceBuf<long long> sel;
    DeviceBuf<double> part_v, out;
    DeviceBuf<int> part_i, first;
};

namespace {

const double *normals_of(const CloudDevice *P) { return P->has_n ? P->nrm.get() : nullptr; }
const double *colors_of(const CloudDevice *P) { return P->has_c ? P->col.get() : nullptr; }

// an empty output cloud with room for `rows` rows of what S has
hipError_t make_like(const CloudDevice *S, int64_t rows, std::unique_ptr<CloudDevice> &O)
{
    O.reset(new CloudDevice);
    O->n = rows;
    O->has_n = S->has_n && rows > 0; O->has_c = S->has_c && rows > 0;
    if (rows > 0) {
        DEV_RESET(O->p, 3 * (size_t)rows);
        if (O->has_n) DEV_RESET(O->nrm, 3 * (size_t)rows);
        if (O->has_c) DEV_RESET(O->col, 3 * (size_t)rows);
    }
    return hipSuccess;
}

}  // namespace

void cloud_device_destroy(CloudDevice *P) { delete P; }

hipError_t cloud_device_create(const double *points, int64_t n, const double *normals, const double *colors, bool on_device,
                               hipStream_t stream, CloudDevice **out)
{
    *out = nullptr;
    std::unique_ptr<CloudDevice> P(new CloudDevice);
    P->n = n;
    P->has_n = normals != nullptr && n > 0; P->has_c = colors != nullptr && n > 0;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t bytes = sizeof(double) * 3 * (size_t)n;
    if (n > 0) {
        DEV_RESET(P->p, 3 * (size_t)n);
        VISMA_TRY(hipMemcpyAsync(P->p.get(), points, bytes, kind, stream));
        if (P->has_n) { DEV_RESET(P->nrm, 3 * (size_t)n); VISMA_TRY(hipMemcpyAsync(P->nrm.get(), normals, bytes, kind, stream)); }
        if (P->has_c) { DEV_RESET(P->col, 3 * (size_t)n); VISMA_TRY(hipMemcpyAsync(P->col.get(), colors, bytes, kind, stream)); }
    }
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = P.release();
    return hipSuccess;
}

void cloud_device_size(const CloudDevice *P, int64_t *n, int *flags)
{
    *n = P->n;
    *flags = (P->has_n ? kCloudNormals : 0) | (P->has_c ? kCloudColors : 0);
}

hipError_t cloud_device_get(CloudDevice *P, double *points, double *normals, double *colors, hipStream_t stream)
{
    const size_t bytes = sizeof(double) * 3 * (size_t)P->n;
    if (P->n > 0) {
        if (points) VISMA_TRY(hipMemcpyAsync(points, P->p.get(), bytes, hipMemcpyDeviceToHost, stream));
        if (normals && P->has_n) VISMA_TRY(hipMemcpyAsync(normals, P->nrm.get(), bytes, hipMemcpyDeviceToHost, stream));
        if (colors && P->has_c) VISMA_TRY(hipMemcpyAsync(colors, P->col.get(), bytes, hipMemcpyDeviceToHost, stream));
    }
    return hipStreamSynchronize(stream);
}

hipError_t cloud_device_transform(CloudDevice *P, const double T[16], hipStream_t stream)
{
    const Mat34 m(T);
    if (P->n > 0) rows_transform<<<capped_blocks(P->n), kThreads, 0, stream>>>(P->p.get(), P->n, m, 1.0);
    if (P->has_n) rows_transform<<<capped_blocks(P->n), kThreads, 0, stream>>>(P->nrm.get(), P->n, m, 0.0);
    VISMA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

hipError_t cloud_device_normalize_normals(CloudDevice *P, hipStream_t stream)
{
    if (P->has_n) rows_normalize<<<capped_blocks(P->n), kThreads, 0, stream>>>(P->nrm.get(), P->n, false);
    VISMA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

hipError_t cloud_device_paint_uniform_color(CloudDevice *P, const double rgb[3], hipStream_t stream)
{
    if (P->n == 0) return hipSuccess;
    DEV_RESERVE(P->col, 3 * (size_t)P->n);
    cl_fill<<<capped_blocks(P->n), kThreads, 0, stream>>>(P->col.get(), P->n, rgb[0], rgb[1], rgb[2]);
    VISMA_TRY(hipGetLastError());
    P->has_c = true;
    return hipStreamSynchronize(stream);
}

// PointCloud.cpp:89-115
hipError_t cloud_device_append(CloudDevice *P, const CloudDevice *other, hipStream_t stream)
{
    if (other->n == 0) return hipSuccess;                    // (not even the normals are cleared)
    const int64_t n0 = P->n, add = other->n, n1 = n0 + add;
    if (n1 > 0x7fffffff) return hipErrorInvalidValue;
    const bool keep_n = (n0 == 0 || P->has_n) && other->has_n, keep_c = (n0 == 0 || P->has_c) && other->has_c;
    const size_t b0 = sizeof(double) * 3 * (size_t)n0, b1 = sizeof(double) * 3 * (size_t)add;
    DeviceBuf<double> p, nrm, col;                           // new arrays: `other` may be P itself
    DEV_RESET(p, 3 * (size_t)n1);
    if (n0 > 0) VISMA_TRY(hipMemcpyAsync(p.get(), P->p.get(), b0, hipMemcpyDeviceToDevice, stream));
    VISMA_TRY(hipMemcpyAsync(p.get() + 3 * n0, other->p.get(), b1, hipMemcpyDeviceToDevice, stream));
    if (keep_n) {
        DEV_RESET(nrm, 3 * (size_t)n1);
        if (n0 > 0) VISMA_TRY(hipMemcpyAsync(nrm.get(), P->nrm.get(), b0, hipMemcpyDeviceToDevice, stream));
        VISMA_TRY(hipMemcpyAsync(nrm.get() + 3 * n0, other->nrm.get(), b1, hipMemcpyDeviceToDevice, stream));
    }
    if (keep_c) {
        DEV_RESET(col, 3 * (size_t)n1);
        if (n0 > 0) VISMA_TRY(hipMemcpyAsync(col.get(), P->col.get(), b0, hipMemcpyDeviceToDevice, stream));
        VISMA_TRY(hipMemcpyAsync(col.get() + 3 * n0, other->col.get(), b1, hipMemcpyDeviceToDevice, stream));
    }
    VISMA_TRY(hipStreamSynchronize(stream));
    P->p = std::move(p); P->nrm = std::move(nrm); P->col = std::move(col);
    P->n = n1; P->has_n = keep_n; P->has_c = keep_c;
    return hipSuccess;
}

hipError_t cloud_device_bounds(CloudDevice *P, double lo[3], double hi[3], hipStream_t stream)
{
    for (int k = 0; k < 3; k++) lo[k] = hi[k] = 0.0;       // PointCloud.cpp:49-51
    if (P->n == 0) return hipSuccess;
    const unsigned parts = capped_blocks(P->n);
    DEV_RESERVE(P->part_v, 6 * (size_t)parts);
    DEV_RESERVE(P->part_i, 6 * (size_t)parts);
    DEV_RESERVE(P->out, 12);
    cl_bounds_partial<<<parts, kThreads, 0, stream>>>(P->p.get(), P->n, P->part_v.get(), P->part_i.get());
    cl_bounds_final<<<1, kThreads, 0, stream>>>(P->part_v.get(), P->part_i.get(), (int)parts, P->p.get(), P->out.get());
    VISMA_TRY(hipGetLastError());
    double h[6];
    VISMA_TRY(hipMemcpyAsync(h, P->out.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < 3; k++) { lo[k] = h[k]; hi[k] = h[3 + k]; }
    return hipSuccess;
}

hipError_t cloud_device_select(CloudDevice *S, const int64_t *h_indices, int64_t n, hipStream_t stream, CloudDevice **out)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "the indices are uploaded as they are");
    *out = nullptr;
    for (int64_t i = 0; i < n; i++)
        if (h_indices[i] < 0 || h_indices[i] >= S->n) return hipErrorInvalidValue;   // (the reference reads out of bounds)
    std::unique_ptr<CloudDevice> O;
    VISMA_TRY(make_like(S, n, O));
    if (n > 0) {
        DEV_RESERVE(S->sel, (size_t)n);
        VISMA_TRY(hipMemcpyAsync(S->sel.get(), h_indices, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, stream));
        const unsigned g = capped_blocks(n);
        cl_gather<<<g, kThreads, 0, stream>>>(S->p.get(), S->sel.get(), O->p.get(), n);
        if (O->has_n) cl_gather<<<g, kThreads, 0, stream>>>(S->nrm.get(), S->sel.get(), O->nrm.get(), n);
        if (O->has_c) cl_gather<<<g, kThreads, 0, stream>>>(S->col.get(), S->sel.get(), O->col.get(), n);
        VISMA_TRY(hipGetLastError());
    }
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = O.release();
    return hipSuccess;
}

hipError_t cloud_device_uniform_down_sample(CloudDevice *S, int64_t every_k, hipStream_t stream, CloudDevice **out)
{
    *out = nullptr;
    const int64_t rows = every_k > 0 && S->n > 0 ? (S->n - 1) / every_k + 1 : 0;  // DownSample.cpp:225-232
    std::unique_ptr<CloudDevice> O;
    VISMA_TRY(make_like(S, rows, O));
    if (rows > 0) {
        const unsigned g = capped_blocks(rows);
        cl_every_k<<<g, kThreads, 0, stream>>>(S->p.get(), every_k, O->p.get(), rows);
        if (O->has_n) cl_every_k<<<g, kThreads, 0, stream>>>(S->nrm.get(), every_k, O->nrm.get(), rows);
        if (O->has_c) cl_every_k<<<g, kThreads, 0, stream>>>(S->col.get(), every_k, O->col.get(), rows);
        VISMA_TRY(hipGetLastError());
    }
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = O.release();
    return hipSuccess;
}

hipError_t cloud_device_crop(CloudDevice *S, const double lo[3], const double hi[3], hipStream_t stream, CloudDevice **out)
{
    *out = nullptr;
    std::unique_ptr<CloudDevice> O;
    const bool illegal = lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2];   // DownSample.cpp:239-243: an empty cloud
    long long rows = 0;
    InsideSource s{S->p.get(), normals_of(S), colors_of(S), {lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}, nullptr, nullptr, nullptr};
    if (!illegal) VISMA_TRY(compact_count(S->comp, s, S->n, stream, &rows));
    VISMA_TRY(make_like(S, rows, O));
    if (rows > 0) {
        s.op = O->p.get(); s.onrm = O->nrm.get(); s.ocol = O->col.get();
        VISMA_TRY(compact_write(S->comp, s, S->n, stream));
    }
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = O.release();
    return hipSuccess;
}

hipError_t cloud_device_voxel_down_sample(CloudDevice *S, double voxel, hipStream_t stream, CloudDevice **out)
{
    *out = nullptr;
    std::unique_ptr<CloudDevice> O(new CloudDevice);
    int64_t rows = 0;
    VISMA_TRY(voxel_down_sample_core(S->p.get(), normals_of(S), colors_of(S), S->n, voxel, O->p, &O->nrm, &O->col, &rows, stream));
    O->n = rows;
    O->has_n = S->has_n && rows > 0; O->has_c = S->has_c && rows > 0;
    VISMA_TRY(hipStreamSynchronize(stream));
    *out = O.release();
    return hipSuccess;
}

hipError_t cloud_device_estimate_normals(CloudDevice *P, int search_type, int knn, double radius, hipStream_t stream)
{
    if (P->n == 0) return hipSuccess;
    const long long n = P->n;
    DeviceBuf<double> fresh;
    DEV_RESET(fresh, 3 * (size_t)n);
    if (estimate_normals_trivial(search_type, knn, radius)) {
        cl_fill<<<capped_blocks(n), kThreads, 0, stream>>>(fresh.get(), n, 0.0, 0.0, 1.0);
        VISMA_TRY(hipGetLastError());
    } else {
        // nn_binning_origin's point: the first one with three finite coordinates, else the zeros
        double origin[3] = {0.0, 0.0, 0.0};
        int first = INT_MAX;
        DEV_RESERVE(P->first, 1);
        VISMA_TRY(hipMemcpyAsync(P->first.get(), &first, sizeof(int), hipMemcpyHostToDevice, stream));
        cl_first_finite<<<capped_blocks(n), kThreads, 0, stream>>>(P->p.get(), n, P->first.get());
        VISMA_TRY(hipGetLastError());
        VISMA_TRY(hipMemcpyAsync(&first, P->first.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        VISMA_TRY(hipStreamSynchronize(stream));
        if (first >= 0 && first < n) {
            VISMA_TRY(hipMemcpyAsync(origin, P->p.get() + 3 * (size_t)first, sizeof(origin), hipMemcpyDeviceToHost, stream));
            VISMA_TRY(hipStreamSynchronize(stream));
        }
        VISMA_TRY(estimate_normals_core(P->p.get(), n, normals_of(P), origin, search_type, knn, radius, fresh.get(), stream));
    }
    VISMA_TRY(hipStreamSynchronize(stream));
    P->nrm = std::move(fresh);
    P->has_n = true;
    return hipSuccess;
}

hipError_t cloud_device_orient_normals(CloudDevice *P, bool camera, const double ref[3], hipStream_t stream)
{
    if (P->n > 0) cl_orient<<<capped_blocks(P->n), kThreads, 0, stream>>>(P->p.get(), P->nrm.get(), P->n, camera, ref[0], ref[1], ref[2]);
    VISMA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

hipError_t cloud_device_mean_and_covariance(CloudDevice *P, int64_t chunk, double mean[3], double cov[9], hipStream_t stream)
{
    for (int k = 0; k < 3; k++) mean[k] = 0.0;               // PointCloud.cpp:147-150
    for (int k = 0; k < 9; k++) cov[k] = k % 4 == 0 ? 1.0 : 0.0;
    if (P->n == 0) return hipSuccess;
    const long long nch = (P->n + chunk - 1) / chunk;
    DEV_RESERVE(P->part_v, 9 * (size_t)nch);
    DEV_RESERVE(P->out, 12);
    cl_cumulant_chunks<<<(unsigned)((nch + 63) / 64), 64, 0, stream>>>(P->p.get(), P->n, chunk, P->part_v.get());
    cl_cumulant_combine<<<1, 64, 0, stream>>>(P->part_v.get(), nch, P->n, P->out.get());
    VISMA_TRY(hipGetLastError());
    double h[12];
    VISMA_TRY(hipMemcpyAsync(h, P->out.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < 3; k++) mean[k] = h[k];
    for (int k = 0; k < 9; k++) cov[k] = h[3 + k];
    return hipSuccess;
}

hipError_t cloud_device_mahalanobis(CloudDevice *P, const double mean[3], const double inv[9], double *out, hipStream_t stream)
{
    if (P->n == 0) return hipSuccess;
    MahalanobisArgs a;
    for (int k = 0; k < 3; k++) a.mean[k] = mean[k];
    for (int k = 0; k < 9; k++) a.inv[k] = inv[k];
    DeviceBuf<double> d;
    DEV_RESET(d, (size_t)P->n);
    cl_mahalanobis<<<capped_blocks(P->n), kThreads, 0, stream>>>(P->p.get(), P->n, a, d.get());
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(hipMemcpyAsync(out, d.get(), sizeof(double) * (size_t)P->n, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

}  // namespace visma
