// nn_grid.hip -- the radius-cell grid of ONE cloud for the neighbourhood features (normals.hip, color_gradient.hip, fpfh.hip;
// the search over it: nn_list.h): the cloud packed for binning, its bounding box, the plan, the counting sort of grid.hip, and
// for KNN searches the cell size tuned from the measured population of the 27 cells.
#include "nn_list.h"

#include <math.h>

#include <algorithm>

namespace visma {

namespace {

// Points, and normals where nrm3 is given, from whichever form the caller holds them in: n x 3 doubles, Pt64 or float4.
// The fp32 copy is used for BINNING only and is taken relative to a point of the cloud (subtracted in f64): its rounding
// error then scales with the cloud's extent, not with its distance from the origin -- a scan 100 m from the origin with
// a 5 mm radius would otherwise put neighbours one cell off (0.1 % slack between cell and radius).  Distances and sums
// use the caller's f64 coordinates, so the results do not depend on the shift.
__global__ void nn_pack_kernel(ColorGradientInput in, float4 *__restrict__ f4, Pt64 *__restrict__ p8, double *__restrict__ nrm3)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.n) return;
    double x, y, z;
    if (in.xyz) { x = in.xyz[3 * i]; y = in.xyz[3 * i + 1]; z = in.xyz[3 * i + 2]; }
    else if (in.xyz64) { const Pt64 p = in.xyz64[i]; x = p.x; y = p.y; z = p.z; }
    else { const float4 p = in.xyz32[i]; x = (double)p.x; y = (double)p.y; z = (double)p.z; }
    f4[i] = make_float4((float)(x - in.origin[0]), (float)(y - in.origin[1]), (float)(z - in.origin[2]), __uint_as_float((unsigned)i));
    p8[i] = Pt64{x, y, z, (unsigned long long)i};
    if (!nrm3) return;                                            // (none, or n x 3 doubles already: read in place)
    if (in.nrm64) { const Pt64 p = in.nrm64[i]; x = p.x; y = p.y; z = p.z; }
    else { const float4 p = in.nrm32[i]; x = (double)p.x; y = (double)p.y; z = (double)p.z; }
    nrm3[3 * i] = x; nrm3[3 * i + 1] = y; nrm3[3 * i + 2] = z;
}

// n27[0] += the points in the 27 cells around every 64th point (cell order), n27[1] += those sampled.  Integer atomics:
// the sums do not depend on the order, nor does the cell size tuned from them.
__global__ __launch_bounds__(256) void nn_sample27_kernel(NnGridView v, long long n, unsigned long long *n27)
{
    const long long t = ((long long)blockIdx.x * 256 + threadIdx.x) * 64;
    if (t >= n) return;
    const NnQuery q = nn_query(v, t);
    const GridParams g = v.g;
    unsigned long long tot = 0;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++) {
            const int z = q.cz + dz, y = q.cy + dy;
            if (z < 0 || z >= g.dim[2] || y < 0 || y >= g.dim[1]) continue;
            const int x0 = max(q.cx - 1, 0), x1 = min(q.cx + 1, g.dim[0] - 1);      // (x0 <= x1: cx is a cell of the grid)
            const long long row = ((long long)z * g.dim[1] + y) * g.dim[0];
            tot += v.start[row + x1 + 1] - v.start[row + x0];
        }
    atomicAdd(n27, tot);
    atomicAdd(n27 + 1, 1ull);
}

}  // namespace

void nn_binning_origin(const double *h_xyz, int64_t n, double origin[3])
{
    for (int64_t i = 0; i < n; i++)
        if (std::isfinite(h_xyz[3 * i]) && std::isfinite(h_xyz[3 * i + 1]) && std::isfinite(h_xyz[3 * i + 2])) {
            origin[0] = h_xyz[3 * i]; origin[1] = h_xyz[3 * i + 1]; origin[2] = h_xyz[3 * i + 2];
            return;
        }
}

hipError_t NnGrid::alloc(int64_t n_points)
{
    n = n_points;
    VISMA_TRY(bufs.alloc(&f4, (size_t)n));
    VISMA_TRY(bufs.alloc(&sorted, (size_t)n + kSortedSlack));
    VISMA_TRY(bufs.alloc(&p8, (size_t)n));
    VISMA_TRY(bufs.alloc(&sorted64, (size_t)n));
    VISMA_TRY(bufs.alloc(&box, 8));
    VISMA_TRY(bufs.alloc(&cell_of, 2 * (size_t)n));   // (cell, rank in the cell)
    VISMA_TRY(bufs.alloc(&n27, 2));
    return hipSuccess;
}

hipError_t NnGrid::build(const ColorGradientInput &in, double *d_nrm3, double radius, int knn_cap, hipStream_t stream)
{
    hipLaunchKernelGGL(nn_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, f4, p8, d_nrm3);
    VISMA_TRY(hipGetLastError());
    VISMA_TRY(launch_grid_bbox(f4, n, box, stream));
    unsigned h_box[6];
    VISMA_TRY(hipMemcpyAsync(h_box, box, sizeof(h_box), hipMemcpyDeviceToHost, stream));
    VISMA_TRY(hipStreamSynchronize(stream));
    float mn[3], mx[3];
    grid_decode_bbox(h_box, mn, mx);
    double diag = 0.0;
    for (int k = 0; k < 3; k++) diag += ((double)mx[k] - mn[k]) * ((double)mx[k] - mn[k]);
    diag = std::sqrt(diag);
    // KNN: a first guess of the distance to the knn-th neighbour on a surface; refined below
    double cell = knn_cap > 0 ? 0.6 * diag * std::sqrt((double)knn_cap / (double)n) : radius;
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = 1.0;
    unsigned *count = nullptr, *start = nullptr, *bsum = nullptr;
    int64_t cell_cap = 0;
    for (int attempt = 0;; attempt++) {
        const int64_t max_cells = std::min<int64_t>(kGridMaxCells, std::max<int64_t>(4096, 8 * n));
        const GridParams g = grid_plan(mn, mx, cell, max_cells);
        if (g.ncell + 1 > cell_cap) {
            VISMA_TRY(bufs.alloc(&count, (size_t)g.ncell + 1));
            VISMA_TRY(bufs.alloc(&start, (size_t)g.ncell + 9));
            VISMA_TRY(bufs.alloc(&bsum, (size_t)grid_scan_blocks(g.ncell) + 1));
            cell_cap = g.ncell + 1;
        }
        VISMA_TRY(launch_grid_build(f4, n, g, cell_of, count, bsum, start, sorted, stream, p8, sorted64));
        view.sorted = sorted; view.sorted64 = sorted64; view.start = start; view.g = g; view.pts = p8;
        if (knn_cap <= 0 || attempt >= 3) break;
        // KNN: aim at 2.5 knn points in the 27 cells (one ring is then enough for most points)
        VISMA_TRY(hipMemsetAsync(n27, 0, 2 * sizeof(unsigned long long), stream));
        hipLaunchKernelGGL(nn_sample27_kernel, dim3((unsigned)(((n + 63) / 64 + 255) / 256)), dim3(256), 0, stream, view,
                           (long long)n, n27);
        VISMA_TRY(hipGetLastError());
        unsigned long long h27[2];
        VISMA_TRY(hipMemcpyAsync(h27, n27, sizeof(h27), hipMemcpyDeviceToHost, stream));
        VISMA_TRY(hipStreamSynchronize(stream));
        const double mean27 = h27[1] ? (double)h27[0] / h27[1] : 0.0, want = 2.5 * knn_cap;
        if (mean27 >= 0.6 * want && mean27 <= 2.5 * want) break;
        const double f = mean27 > 0.0 ? std::sqrt(want / mean27) : 2.0;      // surface scaling; rings cover the rest
        const double next = cell * std::min(std::max(f, 0.25), 4.0);
        if (g.h > (float)(cell * 1.01) && next < cell) break;              // the cell cap already enlarged the cells
        cell = next;
    }
    return hipSuccess;
}

}  // namespace visma
