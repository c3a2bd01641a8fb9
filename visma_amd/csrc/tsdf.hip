// tsdf.hip -- TSDF integration (Open3D's UniformTSDFVolume: Integrate, ExtractPointCloud, ExtractVoxelPointCloud;
// CreateDepthToCameraDistanceMultiplierFloatImage; CreatePointCloudFromDepthImage / FromRGBDImage) on gfx950.
//
// The volume keeps the reference's voxel order x R^2 + y R + z: a COLUMN (x, y) is R contiguous floats.  tsdf and weight are
// one array each; colour is kept in planes (three for RGB8; ONE for Gray32, whose three channels undergo the same
// operations on the same values and are equal bit for bit) and interleaved by the getter.
//
//  multiplier   sqrtf(xx^2 + yy^2 + 1), xx = ((float)j - (float)cx) * (1.0f / (float)fx): built once per intrinsic and kept.
//  integrate    one lane per column, neighbouring lanes on neighbouring columns (a wave covers 64 R contiguous floats; at
//               R = 16 that is 4 KiB, and a lane's column is four 16-byte vectors).  The lane forms the camera-space point
//               of its column at z = 0 and advances it by fp32 additions of extrinsic_f(:, 2) * voxel_length_f: that
//               serial chain is the reference's arithmetic and is kept.  It walks z in 16-byte vectors -- scalar steps
//               up to the first 16-byte boundary of its column (R odd: columns are not aligned) and behind the last
//               whole vector -- and stores a vector only where a voxel of it changed: a frame changes the voxels in its
//               frustum within the truncation band, the rest of the volume is read once and not written.  Every voxel has
//               one writer; there are no atomics.  Everything is fp32, contraction off (the build's -ffp-contract=off),
//               `/` and sqrtf correctly rounded (hipcc's default).
//  extract      count, scan, write over tiles of 256 consecutive voxels (the same three kernels, instantiated for the
//               surface points -- up to three per voxel, one per axis -- and for the voxel cloud): a tile's count, an
//               exclusive scan of the tile counts by one workgroup, then every tile scans its voxels' counts in LDS and
//               writes its rows at its offset.  The output order is the voxel order, then the axis: x, y, z, axis
//               lexicographic, the reference's.  Points, normals and colours are computed in the write pass, in f64 with
//               the fp32 weights promoted as the reference promotes them.
//  from depth   the same three kernels over the strided pixels in row-major order.
//  scalable     ScalableTSDFVolume: units of R^3 voxels in a pool of slots (tsdf, weight, colour planes of capacity x R^3).
//               touched_kernel finds the unit boxes of a frame's strided pixels in f64 (none for a pixel whose point is not
//               finite or whose unit index lies beyond +-2^30), the host (tsdf_units.h) removes duplicates and
//               opens every new unit (the pool grows by allocate, copy, free; slots never move) BEFORE the integrate kernel
//               runs over the list of touched units -- the same kernel, a uniform volume being a list of one.  Extraction
//               walks the units in lexicographic order of their index and reads a +1 neighbour or a corner of GetTSDFAt in
//               the unit next door through a sorted key array (UnitList::find); a missing unit reads weight 0, tsdf 0.
//  mesh         ExtractTriangleMesh: marching cubes, the 256 cases computed from a rule (mc_table.h).  cube_kernel writes a
//               16-bit record per voxel (the case of the cube it is the base of), then two ordered compactions: the vertices
//               (item = voxel, up to three edges; decided from the records of the cubes around an edge; positions and
//               colours in f64 in the reference's order of operations) and the triangles (item = cube; a vertex index is the
//               vertex pass's tile offset + a second 16-bit record).  Both volume kinds behind one corner fetch.
// (Reasoning: DESIGN.md 4.4c11.)
#include "kernels.h"
#include "compact.h"
#include "tsdf_units.h"
#include "mc_table.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <array>
#include <map>
#include <set>
#include <vector>

namespace visma {

namespace {

__global__ __launch_bounds__(kThreads) void multiplier_kernel(float *out, int w, int h, float cx, float cy, float inv_fx, float inv_fy)
{
    const long long n = (long long)w * h;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const int y = (int)(i / w), x = (int)(i - (long long)y * w);
        const float xx = ((float)x - cx) * inv_fx, yy = ((float)y - cy) * inv_fy;
        out[i] = sqrtf(xx * xx + yy * yy + 1.0f);
    }
}

// a uniform volume, or one unit of a scalable one: where its R^3 voxels start in the arrays (slot * R^3) and its origin
struct TsdfUnit { int slot; float ox, oy, oz; };

struct IntegrateArgs {
    float *tsdf, *weight, *c0, *c1, *c2;                 // slots x R^3 each; c1, c2 only for RGB8
    const TsdfUnit *units;                               // the units this frame integrates into
    int n_units;
    int R;
    const float *depth, *mult, *gray;
    const uint8_t *rgb;
    int w, h;
    float fx, fy, cx, cy;
    float e[12];                                         // extrinsic_f, rows 0 .. 2
    float es[3];                                         // extrinsic_f(:, 2) * voxel_length_f
    float vl, half, trunc, trunc_inv, safe_w, safe_h;
};

// one voxel: the reference's loop body.  Returns whether the voxel was integrated.
template <int CT>
__device__ inline bool integrate_voxel(const IntegrateArgs &a, float px, float py, float pz, float &t, float &wt, float &c0, float &c1, float &c2)
{
    if (!(pz > 0.0f)) return false;
    const float u_f = px * a.fx / pz + a.cx + 0.5f;
    const float v_f = py * a.fy / pz + a.cy + 0.5f;
    if (!(u_f >= 0.0001f && u_f < a.safe_w && v_f >= 0.0001f && v_f < a.safe_h)) return false;
    const int u = (int)u_f, v = (int)v_f;
    const long long at = (long long)v * a.w + u;
    const float d = a.depth[at];
    if (!(d > 0.0f)) return false;
    const float sdf = (d - pz) * a.mult[at];
    if (!(sdf > -a.trunc)) return false;
    const float s = sdf * a.trunc_inv;
    const float ts = s < 1.0f ? s : 1.0f;                // std::min(1.0f, s)
    const float w1 = wt + 1.0f;
    t = (t * wt + ts) / w1;
    if (CT == kTsdfColorRgb8) {
        const uint8_t *rgb = a.rgb + 3 * at;
        c0 = (c0 * wt + (float)rgb[0]) / w1;
        c1 = (c1 * wt + (float)rgb[1]) / w1;
        c2 = (c2 * wt + (float)rgb[2]) / w1;
    } else if (CT == kTsdfColorGray32) {
        c0 = (c0 * wt + a.gray[at]) / w1;
    }
    wt = w1;
    return true;
}

template <int CT>
__global__ __launch_bounds__(kThreads) void integrate_kernel(IntegrateArgs a)
{
    const int R = a.R;
    const long long columns = (long long)R * R, items = columns * a.n_units;
    for (long long item = (long long)blockIdx.x * kThreads + threadIdx.x; item < items; item += (long long)gridDim.x * kThreads) {
        const TsdfUnit unit = a.units[item / columns];
        const long long col = item % columns;
        const int x = (int)(col / R), y = (int)(col - (long long)x * R);
        const float X = a.half + a.vl * (float)x + unit.ox, Y = a.half + a.vl * (float)y + unit.oy, Z = a.half + unit.oz;
        float px = a.e[0] * X + a.e[1] * Y + a.e[2] * Z + a.e[3];
        float py = a.e[4] * X + a.e[5] * Y + a.e[6] * Z + a.e[7];
        float pz = a.e[8] * X + a.e[9] * Y + a.e[10] * Z + a.e[11];
        const long long base = ((long long)unit.slot * columns + col) * R;   // the column's first voxel; the arrays are 16-byte aligned
        int z = 0;
        const int head = std::min(R, (int)((4 - (base & 3)) & 3));
        auto scalar_steps = [&](int end) {
            for (; z < end; z++) {
                const long long i = base + z;
                float t = a.tsdf[i], wt = a.weight[i], c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
                if (CT != kTsdfColorNone) c0 = a.c0[i];
                if (CT == kTsdfColorRgb8) { c1 = a.c1[i]; c2 = a.c2[i]; }
                if (integrate_voxel<CT>(a, px, py, pz, t, wt, c0, c1, c2)) {
                    a.tsdf[i] = t; a.weight[i] = wt;
                    if (CT != kTsdfColorNone) a.c0[i] = c0;
                    if (CT == kTsdfColorRgb8) { a.c1[i] = c1; a.c2[i] = c2; }
                }
                px += a.es[0]; py += a.es[1]; pz += a.es[2];
            }
        };
        scalar_steps(head);
        for (; z + 4 <= R; z += 4) {
            const long long i = base + z;                // a multiple of 4
            float4 t = *reinterpret_cast<const float4 *>(a.tsdf + i), wt = *reinterpret_cast<const float4 *>(a.weight + i);
            float4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0}, c2 = {0, 0, 0, 0};
            if (CT != kTsdfColorNone) c0 = *reinterpret_cast<const float4 *>(a.c0 + i);
            if (CT == kTsdfColorRgb8) { c1 = *reinterpret_cast<const float4 *>(a.c1 + i); c2 = *reinterpret_cast<const float4 *>(a.c2 + i); }
            bool any = integrate_voxel<CT>(a, px, py, pz, t.x, wt.x, c0.x, c1.x, c2.x);
            px += a.es[0]; py += a.es[1]; pz += a.es[2];
            any |= integrate_voxel<CT>(a, px, py, pz, t.y, wt.y, c0.y, c1.y, c2.y);
            px += a.es[0]; py += a.es[1]; pz += a.es[2];
            any |= integrate_voxel<CT>(a, px, py, pz, t.z, wt.z, c0.z, c1.z, c2.z);
            px += a.es[0]; py += a.es[1]; pz += a.es[2];
            any |= integrate_voxel<CT>(a, px, py, pz, t.w, wt.w, c0.w, c1.w, c2.w);
            px += a.es[0]; py += a.es[1]; pz += a.es[2];
            if (any) {
                *reinterpret_cast<float4 *>(a.tsdf + i) = t; *reinterpret_cast<float4 *>(a.weight + i) = wt;
                if (CT != kTsdfColorNone) *reinterpret_cast<float4 *>(a.c0 + i) = c0;
                if (CT == kTsdfColorRgb8) { *reinterpret_cast<float4 *>(a.c1 + i) = c1; *reinterpret_cast<float4 *>(a.c2 + i) = c2; }
            }
        }
        scalar_steps(R);
    }
}


__device__ inline bool voxel_valid(float w, float f) { return w != 0.0f && f < 0.98f && f >= -0.98f; }

// The units of an extraction in ITS order (a uniform volume: one; a scalable one: lexicographic by index), on the device:
// keys 3 ints per unit (the index), slots, origins 3 doubles per unit (index * unit length, formed on the host in f64)
struct UnitList {
    const int *keys, *slots;
    const double *origins;
    int n;
    // the position of unit (kx, ky, kz) in the sorted keys, or -1: the index -> slot map of the neighbour lookups
    __device__ int find(int kx, int ky, int kz) const
    {
        int lo = 0, hi = n - 1;
        while (lo <= hi) {
            const int mid = (lo + hi) >> 1;
            const int *k = keys + 3 * mid;
            const int c = k[0] != kx ? (k[0] < kx ? -1 : 1) : k[1] != ky ? (k[1] < ky ? -1 : 1) : k[2] != kz ? (k[2] < kz ? -1 : 1) : 0;
            if (c == 0) return mid;
            if (c < 0) lo = mid + 1; else hi = mid - 1;
        }
        return -1;
    }
};

// UniformTSDFVolume::ExtractVoxelPointCloud of every unit: item = (unit in list order, voxel)
struct VoxelCloudSource {
    const float *tsdf, *weight;
    const double *zs;                                    // half + k additions of voxel_length, k = 0 .. R - 1 (formed on the host)
    UnitList units;
    int R;
    double vl, half;                                     // the unit's own voxel length
    double *points, *colors;
    __device__ long long voxel(long long i) const { const long long R3 = (long long)R * R * R; return units.slots[i / R3] * R3 + i % R3; }
    __device__ int count(long long i) const { const long long v = voxel(i); return voxel_valid(weight[v], tsdf[v]) ? 1 : 0; }
    __device__ void emit(long long item, long long row) const
    {
        const long long R3 = (long long)R * R * R, i = item % R3;
        const double *o = units.origins + 3 * (item / R3);
        const double ox = o[0], oy = o[1], oz = o[2];
        const long long v = voxel(item);
        const int z = (int)(i % R), y = (int)((i / R) % R), x = (int)(i / ((long long)R * R));
        points[3 * row] = half + vl * x + ox;
        points[3 * row + 1] = half + vl * y + oy;
        points[3 * row + 2] = zs[z] + oz;
        const double c = ((double)tsdf[v] + 1.0) * 0.5;
        colors[3 * row] = c; colors[3 * row + 1] = c; colors[3 * row + 2] = c;
    }
};

// UniformTSDFVolume::ExtractPointCloud: item = voxel, up to three rows (one per axis)
struct SurfaceSource {
    const float *tsdf, *weight, *c0, *c1, *c2;
    int R, color_type;
    double vl, half, ox, oy, oz;
    double *points, *normals, *colors;

    __device__ long long stride(int axis) const { return axis == 0 ? (long long)R * R : axis == 1 ? R : 1; }
    // bit `axis` set: the edge from voxel i to its +1 neighbour along `axis` carries a point
    __device__ int mask(long long i) const
    {
        const int z = (int)(i % R), y = (int)((i / R) % R), x = (int)(i / ((long long)R * R));
        if (x < 1 || y < 1 || z < 1 || x > R - 2 || y > R - 2 || z > R - 2) return 0;
        const float f0 = tsdf[i];
        if (!voxel_valid(weight[i], f0)) return 0;
        const int at[3] = {x, y, z};
        int m = 0;
        for (int a = 0; a < 3; a++) {
            if (at[a] + 1 >= R - 1) continue;
            const long long j = i + stride(a);
            const float f1 = tsdf[j];
            if (voxel_valid(weight[j], f1) && f0 * f1 < 0.0f) m |= 1 << a;
        }
        return m;
    }
    __device__ int count(long long i) const { return __popc((unsigned)mask(i)); }

    // UniformTSDFVolume::GetTSDFAt (indices clamped into the volume: an extracted point never leaves it)
    __device__ double tsdf_at(double px, double py, double pz) const
    {
        const double gx = px / vl - 0.5, gy = py / vl - 0.5, gz = pz / vl - 0.5;
        const double fx = floor(gx), fy = floor(gy), fz = floor(gz);
        const double r0 = gx - fx, r1 = gy - fy, r2 = gz - fz;
        auto clampi = [this](double f) { const int v = (int)f; return v < 0 ? 0 : v > R - 2 ? R - 2 : v; };
        const int x = clampi(fx), y = clampi(fy), z = clampi(fz);
        const float *t = tsdf + ((long long)x * R + y) * R + z;
        const long long sx = (long long)R * R, sy = R;
        return (1 - r0) * ((1 - r1) * ((1 - r2) * t[0] + r2 * t[1]) + r1 * ((1 - r2) * t[sy] + r2 * t[sy + 1])) +
               r0 * ((1 - r1) * ((1 - r2) * t[sx] + r2 * t[sx + 1]) + r1 * ((1 - r2) * t[sx + sy] + r2 * t[sx + sy + 1]));
    }

    __device__ void emit(long long i, long long row) const
    {
        const int z = (int)(i % R), y = (int)((i / R) % R), x = (int)(i / ((long long)R * R));
        const int m = mask(i);
        const float f0 = tsdf[i];
        const double p0[3] = {half + vl * x, half + vl * y, half + vl * z};
        const double gap = 0.99 * vl;
        for (int a = 0; a < 3; a++) {
            if (!(m & (1 << a))) continue;
            const long long j = i + stride(a);
            const float f1 = tsdf[j];
            const float r0 = fabsf(f0), r1 = fabsf(f1);
            const float rs = r0 + r1;
            double p[3] = {p0[0], p0[1], p0[2]};
            const double p1 = p0[a] + vl;
            p[a] = (p0[a] * r1 + p1 * r0) / rs;
            points[3 * row] = p[0] + ox; points[3 * row + 1] = p[1] + oy; points[3 * row + 2] = p[2] + oz;
            if (color_type == kTsdfColorRgb8) {
                colors[3 * row] = (double)((c0[i] * r1 + c0[j] * r0) / rs / 255.0f);
                colors[3 * row + 1] = (double)((c1[i] * r1 + c1[j] * r0) / rs / 255.0f);
                colors[3 * row + 2] = (double)((c2[i] * r1 + c2[j] * r0) / rs / 255.0f);
            } else if (color_type == kTsdfColorGray32) {
                const double g = (double)((c0[i] * r1 + c0[j] * r0) / rs);
                colors[3 * row] = g; colors[3 * row + 1] = g; colors[3 * row + 2] = g;
            }
            // GetNormalAt
            double n[3];
            for (int k = 0; k < 3; k++) {
                double lo[3] = {p[0], p[1], p[2]}, hi[3] = {p[0], p[1], p[2]};
                lo[k] -= gap; hi[k] += gap;
                n[k] = tsdf_at(hi[0], hi[1], hi[2]) - tsdf_at(lo[0], lo[1], lo[2]);
            }
            const double zz = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];       // Eigen's normalized(): (x^2 + y^2) + z^2
            if (zz > 0.0) { const double s = sqrt(zz); n[0] /= s; n[1] /= s; n[2] /= s; }
            normals[3 * row] = n[0]; normals[3 * row + 1] = n[1]; normals[3 * row + 2] = n[2];
            row++;
        }
    }
};

// ScalableTSDFVolume::ExtractPointCloud: item = (unit in lexicographic order, voxel), up to three rows.  A +1 neighbour or
// a corner of GetTSDFAt beyond the unit is looked up in the unit next door; a missing unit reads weight 0, tsdf 0.
struct ScalableSurfaceSource {
    const float *tsdf, *weight, *c0, *c1, *c2;
    UnitList units;
    int R, color_type;
    double vl, half, ul;                                 // the volume's voxel length, half of it, the unit length
    double *points, *normals, *colors;

    // the memory position of voxel (x, y, z) of the unit at list position u, each coordinate in [0, 2 R): beyond R - 1 it is
    // the neighbouring unit's; -1 where that unit does not exist
    __device__ long long at(int u, int x, int y, int z) const
    {
        const long long R3 = (long long)R * R * R;
        int slot = units.slots[u];
        if (x >= R || y >= R || z >= R) {
            const int *k = units.keys + 3 * u;
            const int v = units.find(k[0] + (x >= R), k[1] + (y >= R), k[2] + (z >= R));
            if (v < 0) return -1;
            slot = units.slots[v];
            if (x >= R) x -= R;
            if (y >= R) y -= R;
            if (z >= R) z -= R;
        }
        return slot * R3 + ((long long)x * R + y) * R + z;
    }
    __device__ int mask(long long item) const
    {
        const long long R3 = (long long)R * R * R, i = item % R3;
        const int u = (int)(item / R3);
        const int z = (int)(i % R), y = (int)((i / R) % R), x = (int)(i / ((long long)R * R));
        const long long v0 = at(u, x, y, z);
        const float f0 = tsdf[v0];
        if (!voxel_valid(weight[v0], f0)) return 0;
        int m = 0;
        for (int a = 0; a < 3; a++) {
            const long long v1 = at(u, x + (a == 0), y + (a == 1), z + (a == 2));
            if (v1 < 0) continue;
            const float f1 = tsdf[v1];
            if (voxel_valid(weight[v1], f1) && f0 * f1 < 0.0f) m |= 1 << a;
        }
        return m;
    }
    __device__ int count(long long item) const { return __popc((unsigned)mask(item)); }

    // ScalableTSDFVolume::GetTSDFAt
    __device__ double tsdf_at(double px, double py, double pz) const
    {
        const double lx = px - 0.5 * vl, ly = py - 0.5 * vl, lz = pz - 0.5 * vl;
        const double ux = floor(lx / ul), uy = floor(ly / ul), uz = floor(lz / ul);
        const int u = units.find((int)ux, (int)uy, (int)uz);
        if (u < 0) return 0.0;
        const double gx = (lx - ux * ul) / vl, gy = (ly - uy * ul) / vl, gz = (lz - uz * ul) / vl;
        auto clampi = [this](double f) { const int v = (int)floor(f); return v < 0 ? 0 : v > R - 1 ? R - 1 : v; };
        const int x = clampi(gx), y = clampi(gy), z = clampi(gz);
        const double r0 = gx - x, r1 = gy - y, r2 = gz - z;
        float f[2][2][2];
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++)
                for (int c = 0; c < 2; c++) {
                    const long long v = at(u, x + a, y + b, z + c);
                    f[a][b][c] = v < 0 ? 0.0f : tsdf[v];
                }
        return (1 - r0) * ((1 - r1) * ((1 - r2) * f[0][0][0] + r2 * f[0][0][1]) + r1 * ((1 - r2) * f[0][1][0] + r2 * f[0][1][1])) +
               r0 * ((1 - r1) * ((1 - r2) * f[1][0][0] + r2 * f[1][0][1]) + r1 * ((1 - r2) * f[1][1][0] + r2 * f[1][1][1]));
    }

    __device__ void emit(long long item, long long row) const
    {
        const long long R3 = (long long)R * R * R, i = item % R3;
        const int u = (int)(item / R3);
        const int z = (int)(i % R), y = (int)((i / R) % R), x = (int)(i / ((long long)R * R));
        const int *k = units.keys + 3 * u;
        const int m = mask(item);
        const long long v0 = at(u, x, y, z);
        const float f0 = tsdf[v0];
        const double p0[3] = {half + vl * x + (double)k[0] * ul, half + vl * y + (double)k[1] * ul, half + vl * z + (double)k[2] * ul};
        const double gap = 0.99 * vl;
        for (int a = 0; a < 3; a++) {
            if (!(m & (1 << a))) continue;
            const long long v1 = at(u, x + (a == 0), y + (a == 1), z + (a == 2));
            const float f1 = tsdf[v1];
            const float r0 = fabsf(f0), r1 = fabsf(f1);
            const float rs = r0 + r1;
            double p[3] = {p0[0], p0[1], p0[2]};
            const double p1 = p0[a] + vl;
            p[a] = (p0[a] * r1 + p1 * r0) / rs;
            points[3 * row] = p[0]; points[3 * row + 1] = p[1]; points[3 * row + 2] = p[2];
            if (color_type == kTsdfColorRgb8) {
                colors[3 * row] = (double)((c0[v0] * r1 + c0[v1] * r0) / rs / 255.0f);
                colors[3 * row + 1] = (double)((c1[v0] * r1 + c1[v1] * r0) / rs / 255.0f);
                colors[3 * row + 2] = (double)((c2[v0] * r1 + c2[v1] * r0) / rs / 255.0f);
            } else if (color_type == kTsdfColorGray32) {
                const double g = (double)((c0[v0] * r1 + c0[v1] * r0) / rs);
                colors[3 * row] = g; colors[3 * row + 1] = g; colors[3 * row + 2] = g;
            }
            double n[3];
            for (int q = 0; q < 3; q++) {
                double lo[3] = {p[0], p[1], p[2]}, hi[3] = {p[0], p[1], p[2]};
                lo[q] -= gap; hi[q] += gap;
                n[q] = tsdf_at(hi[0], hi[1], hi[2]) - tsdf_at(lo[0], lo[1], lo[2]);
            }
            const double zz = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
            if (zz > 0.0) { const double sq = sqrt(zz); n[0] /= sq; n[1] /= sq; n[2] /= sq; }
            normals[3 * row] = n[0]; normals[3 * row + 1] = n[1]; normals[3 * row + 2] = n[2];
            row++;
        }
    }
};

// ---- ExtractTriangleMesh: marching cubes (the case rule: mc_table.h; the semantics: visma_icp.h) ----
// An item is a voxel in extraction order (unit in list order, then x R^2 + y R + z): the base of a cube and the lower end of
// up to three vertex edges.  Three passes share two 16-bit records per item:
//   cube_rec   cube_kernel: the cube's case (bits 0 .. 7), bit 8: the cube is valid, bit 9: the voxel's own weight is != 0
//   vert_rec   the vertex pass's write: which of the voxel's +x, +y, +z edges carry a vertex (bits 0 .. 2) and the row of its
//              first vertex within its tile of 256 items (bits 3 .. 12; at most 255 * 3)
// so the vertex of an edge is tile_offset[item / 256] + (vert_rec >> 3) + the set mask bits below its axis: no hash.
// The two grids are the corner fetch: where the neighbour of a voxel is, and its global index.
struct UniformGrid {
    int R;
    static constexpr bool kOrigin = true;
    __device__ void split(long long item, int &u, int &x, int &y, int &z) const
    {
        u = 0; z = (int)(item % R); y = (int)((item / R) % R); x = (int)(item / ((long long)R * R));
    }
    // the item at (x, y, z), each in [-1, R], or -1 beyond the volume
    __device__ long long item_at(int, int x, int y, int z) const
    {
        if ((unsigned)x >= (unsigned)R || (unsigned)y >= (unsigned)R || (unsigned)z >= (unsigned)R) return -1;
        return ((long long)x * R + y) * R + z;
    }
    __device__ long long voxel(long long item) const { return item; }
    __device__ void index(int, int x, int y, int z, double g[3]) const { g[0] = (double)x; g[1] = (double)y; g[2] = (double)z; }
};

struct ScalableGrid {
    UnitList units;
    int R;
    static constexpr bool kOrigin = false;
    __device__ void split(long long item, int &u, int &x, int &y, int &z) const
    {
        const long long R3 = (long long)R * R * R, i = item % R3;
        u = (int)(item / R3); z = (int)(i % R); y = (int)((i / R) % R); x = (int)(i / ((long long)R * R));
    }
    // ... of the unit at list position u; beyond the unit it is the neighbouring unit's, -1 where that does not exist
    __device__ long long item_at(int u, int x, int y, int z) const
    {
        const int dx = x < 0 ? -1 : x >= R ? 1 : 0, dy = y < 0 ? -1 : y >= R ? 1 : 0, dz = z < 0 ? -1 : z >= R ? 1 : 0;
        if (dx | dy | dz) {
            const int *k = units.keys + 3 * u;
            u = units.find(k[0] + dx, k[1] + dy, k[2] + dz);
            if (u < 0) return -1;
            x -= dx * R; y -= dy * R; z -= dz * R;
        }
        return (long long)u * R * R * R + ((long long)x * R + y) * R + z;
    }
    __device__ long long voxel(long long item) const
    {
        const long long R3 = (long long)R * R * R;
        return units.slots[item / R3] * R3 + item % R3;
    }
    // the global voxel index
    __device__ void index(int u, int x, int y, int z, double g[3]) const
    {
        const int *k = units.keys + 3 * u;
        g[0] = (double)((long long)k[0] * R + x); g[1] = (double)((long long)k[1] * R + y); g[2] = (double)((long long)k[2] * R + z);
    }
};

constexpr unsigned kCubeValid = 0x100, kCubeOwnWeight = 0x200;

template <class Grid>
struct MeshArgs {
    Grid g;
    const float *tsdf, *weight, *c0, *c1, *c2;
    int color_type;
    double vl, half, ox, oy, oz;
    uint16_t *cube_rec, *vert_rec;
    const McCase *table;
    const long long *vert_tile_offset;                   // the vertex pass's tile offsets
    double *vertices, *colors;
    int *triangles;
};

// the cube of every item: most voxels have weight 0 and are decided by that one load
template <class Grid>
__global__ __launch_bounds__(kThreads) void cube_kernel(MeshArgs<Grid> a, long long n)
{
    for (long long item = (long long)blockIdx.x * kThreads + threadIdx.x; item < n; item += (long long)gridDim.x * kThreads) {
        const long long v0 = a.g.voxel(item);
        unsigned rec = 0;
        if (a.weight[v0] != 0.0f) {
            int u, x, y, z;
            a.g.split(item, u, x, y, z);
            unsigned cs = a.tsdf[v0] < 0.0f ? 1u : 0u;
            bool valid = true;
            for (int i = 1; i < 8 && valid; i++) {
                const long long j = a.g.item_at(u, x + (i & 1), y + ((i >> 1) & 1), z + (i >> 2));
                if (j < 0) { valid = false; break; }
                const long long v = a.g.voxel(j);
                if (a.weight[v] == 0.0f) { valid = false; break; }
                if (a.tsdf[v] < 0.0f) cs |= 1u << i;
            }
            rec = kCubeOwnWeight | (valid ? (kCubeValid | cs) : 0u);
        }
        a.cube_rec[item] = (uint16_t)rec;
    }
}

// the vertices: item = voxel, up to three rows (its +x, +y, +z edges)
template <class Grid>
struct MeshVertexSource {
    MeshArgs<Grid> a;
    // bit `axis`: the two ends differ in sign in a valid cube around the edge (any valid cube holds both ends' signs)
    __device__ int mask(long long item) const
    {
        const unsigned own = a.cube_rec[item];
        if (!(own & kCubeOwnWeight)) return 0;
        int u, x, y, z;
        a.g.split(item, u, x, y, z);
        // the cubes at (x - i, y - j, z - k), i, j, k in {0, 1}; the one at (-1, -1, -1) holds none of the three edges
        unsigned rec[2][2][2];
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 2; j++)
                for (int k = 0; k < 2; k++) {
                    rec[i][j][k] = 0;
                    if (i + j + k == 0) { rec[0][0][0] = own; continue; }
                    if (i + j + k == 3) continue;
                    const long long c = a.g.item_at(u, x - i, y - j, z - k);
                    if (c >= 0) rec[i][j][k] = a.cube_rec[c];
                }
        int m = 0;
        for (int axis = 0; axis < 3; axis++) {
            bool cut = false;
            for (int i = 0; i < 2; i++)
                for (int j = 0; j < 2; j++)
                    for (int k = 0; k < 2; k++) {
                        const int d[3] = {i, j, k};
                        if (d[axis]) continue;
                        const unsigned r = rec[i][j][k];
                        if (!(r & kCubeValid)) continue;
                        const int lo = i | (j << 1) | (k << 2);                // this voxel as a corner of that cube
                        cut = cut || (((r >> lo) ^ (r >> (lo | (1 << axis)))) & 1u);
                    }
            if (cut) m |= 1 << axis;
        }
        return m;
    }
    __device__ int count(long long item) const { return __popc((unsigned)mask(item)); }

    // f64, in the reference's order of operations (contraction is off for the whole build)
    __device__ void emit(long long item, long long row) const
    {
        const int m = mask(item);
        a.vert_rec[item] = (uint16_t)((unsigned)m | ((unsigned)(row - a.vert_tile_offset[item / kThreads]) << 3));
        int u, x, y, z;
        a.g.split(item, u, x, y, z);
        const long long v0 = a.g.voxel(item);
        const double f0 = fabs((double)a.tsdf[v0]);
        double g[3];
        a.g.index(u, x, y, z, g);
        const double p0[3] = {a.half + a.vl * g[0], a.half + a.vl * g[1], a.half + a.vl * g[2]};
        for (int axis = 0; axis < 3; axis++) {
            if (!(m & (1 << axis))) continue;
            const long long v1 = a.g.voxel(a.g.item_at(u, x + (axis == 0), y + (axis == 1), z + (axis == 2)));
            const double f1 = fabs((double)a.tsdf[v1]);
            double p[3] = {p0[0], p0[1], p0[2]};
            p[axis] += f0 * a.vl / (f0 + f1);
            if (Grid::kOrigin) { p[0] = p[0] + a.ox; p[1] = p[1] + a.oy; p[2] = p[2] + a.oz; }
            a.vertices[3 * row] = p[0]; a.vertices[3 * row + 1] = p[1]; a.vertices[3 * row + 2] = p[2];
            if (a.color_type == kTsdfColorRgb8) {
                const float *plane[3] = {a.c0, a.c1, a.c2};
                for (int c = 0; c < 3; c++) {
                    const double k0 = (double)plane[c][v0] / 255.0, k1 = (double)plane[c][v1] / 255.0;
                    a.colors[3 * row + c] = (f1 * k0 + f0 * k1) / (f0 + f1);
                }
            } else if (a.color_type == kTsdfColorGray32) {
                const double k0 = (double)a.c0[v0], k1 = (double)a.c0[v1];
                const double gray = (f1 * k0 + f0 * k1) / (f0 + f1);
                a.colors[3 * row] = gray; a.colors[3 * row + 1] = gray; a.colors[3 * row + 2] = gray;
            }
            row++;
        }
    }
};

// the triangles: item = cube, the rows of its case
template <class Grid>
struct MeshTriangleSource {
    MeshArgs<Grid> a;
    __device__ int count(long long item) const
    {
        const unsigned r = a.cube_rec[item];
        return (r & kCubeValid) ? a.table[r & 0xffu].n : 0;
    }
    __device__ void emit(long long item, long long row) const
    {
        const McCase cs = a.table[a.cube_rec[item] & 0xffu];
        int u, x, y, z;
        a.g.split(item, u, x, y, z);
        long long corner[8];                             // (every corner of a valid cube exists)
        for (int i = 0; i < 8; i++) corner[i] = i ? a.g.item_at(u, x + (i & 1), y + ((i >> 1) & 1), z + (i >> 2)) : item;
        for (int t = 0; t < 3 * (int)cs.n; t++) {
            const int e = cs.edge[t], axis = e >> 2;
            const long long lower = corner[mc_edge_lower(e)];
            const unsigned vr = a.vert_rec[lower];
            a.triangles[3 * row + t] = (int)(a.vert_tile_offset[lower / kThreads] + (long long)(vr >> 3) + __popc(vr & ((1u << axis) - 1u)));
        }
    }
};

// CreatePointCloudFromFloatDepthImage / CreatePointCloudFromRGBDImageT: item = strided pixel, row-major
struct DepthSource {
    const float *depth, *gray;
    const uint8_t *rgb;
    int w, sw, stride, color_type;                       // sw: strided pixels per row
    double fx, fy, cx, cy;
    double pose[12];
    double *points, *colors;
    __device__ long long pixel(long long i) const { return (i / sw) * stride * (long long)w + (i % sw) * stride; }
    __device__ int count(long long i) const { return depth[pixel(i)] > 0.0f ? 1 : 0; }
    __device__ void point(long long i, double p[3]) const
    {
        const long long at = pixel(i);
        const int v = (int)(at / w), u = (int)(at % w);
        const double z = (double)depth[at];
        const double x = (u - cx) * z / fx, y = (v - cy) * z / fy;
        for (int r = 0; r < 3; r++) p[r] = pose[4 * r] * x + pose[4 * r + 1] * y + pose[4 * r + 2] * z + pose[4 * r + 3];
    }
    __device__ void emit(long long i, long long row) const
    {
        const long long at = pixel(i);
        point(i, points + 3 * row);
        if (color_type == kTsdfColorRgb8) {
            for (int c = 0; c < 3; c++) colors[3 * row + c] = (double)rgb[3 * at + c] / 255.0;
        } else if (color_type == kTsdfColorGray32) {
            const double g = (double)gray[at];
            colors[3 * row] = g; colors[3 * row + 1] = g; colors[3 * row + 2] = g;
        }
    }
};

// ScalableTSDFVolume::Integrate's touched units: per strided pixel with a depth, LocateVolumeUnit(point - sdf_trunc) and
// LocateVolumeUnit(point + sdf_trunc) in f64 -- a TouchedBox.  The host expands the boxes into unit keys and removes the
// duplicates (tsdf_units.h).  A pixel without a depth, with a point that is not finite (a depth of inf, or of 1e38 times a
// pose) or with an index beyond +-2^30 has valid = 0.  The comparisons are made on the f64 floors and are false for a NaN,
// so no value is converted to int that an int cannot hold.
__global__ __launch_bounds__(kThreads) void touched_kernel(DepthSource s, long long n, double trunc, double ul, TouchedBox *boxes)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        TouchedBox b = {{0, 0, 0}, {0, 0, 0}, 0};
        if (s.count(i)) {
            double p[3];
            s.point(i, p);
            bool ok = true;
            for (int a = 0; a < 3; a++) {
                const double lo = floor((p[a] - trunc) / ul), hi = floor((p[a] + trunc) / ul);
                ok = ok && isfinite(p[a]) && fabs(lo) <= (double)kTsdfUnitIndexLimit && fabs(hi) <= (double)kTsdfUnitIndexLimit;
                if (ok) { b.lo[a] = (int32_t)lo; b.hi[a] = (int32_t)hi; }
            }
            b.valid = ok ? 1 : 0;
        }
        boxes[i] = b;
    }
}

}  // namespace

struct TsdfDevice {
    TsdfConfig cfg;
    hipStream_t stream = nullptr;
    size_t R3 = 0;                                       // voxels of a unit
    size_t capacity = 0;                                 // units the pool holds (a uniform volume: one)
    DeviceBuf<float> tsdf, weight, color[3];              // capacity x R3 each; the planes beyond planes() stay empty
    DeviceBuf<double> zs;
    // unit index -> slot, in lexicographic order of the index; slots are handed out in opening order and never move
    std::map<std::array<int, 3>, int> slot_of;
    // the last frame: depth, colour, the multiplier image of the last intrinsic, the touched boxes, the unit list
    DeviceBuf<float> depth, gray, mult;
    DeviceBuf<uint8_t> rgb;
    DeviceBuf<TouchedBox> bounds;
    DeviceBuf<TsdfUnit> unit_list;
    int mult_w = 0, mult_h = 0;
    double mult_k[4] = {0, 0, 0, 0};
    Compactor comp;
    // an extraction's unit list on the device
    DeviceBuf<int> x_keys, x_slots;
    DeviceBuf<double> x_origins;
    // the last extractions: [0] surface points, [1] voxel cloud
    DeviceBuf<double> out_points[2], out_normals, out_colors[2];
    long long rows[2] = {-1, -1};
    // ExtractTriangleMesh: the second compaction (comp keeps the vertex pass's tile offsets for the triangle pass), the two
    // records per item (4 transient bytes per voxel, grow-only), the case table, and the last mesh
    bool integrated = false;                             // a frame went in since the creation or the last Reset()
    Compactor comp_tri;
    DeviceBuf<uint16_t> cube_rec, vert_rec;
    DeviceBuf<McCase> mc_cases;
    DeviceBuf<double> mesh_vertices, mesh_colors;
    DeviceBuf<int> mesh_triangles;
    long long mesh_nv = -1, mesh_nt = -1;
    int planes() const { return cfg.color_type == kTsdfColorRgb8 ? 3 : cfg.color_type == kTsdfColorGray32 ? 1 : 0; }
    double unit_length() const { return cfg.length; }
    double unit_voxel_length() const { return cfg.length / (double)cfg.resolution; }
};

namespace {

// the pool at `units` units: new arrays, the old contents copied, the rest zero; they take the old ones' place only when
// every one of them exists and is filled -- a failed allocation or copy leaves the volume as it was
hipError_t pool_resize(TsdfDevice *D, size_t units)
{
    DeviceBuf<float> fresh[5], *old[5] = {&D->tsdf, &D->weight, &D->color[0], &D->color[1], &D->color[2]};
    const int arrays = 2 + D->planes();
    const size_t bytes = sizeof(float) * D->R3 * units, keep = sizeof(float) * D->R3 * std::min(units, D->capacity);
    for (int a = 0; a < arrays; a++) DEV_RESET(fresh[a], D->R3 * units);
    hipError_t e = hipSuccess;
    for (int a = 0; a < arrays && e == hipSuccess; a++) {
        e = hipMemsetAsync(fresh[a], 0, bytes, D->stream);
        if (e == hipSuccess && keep && *old[a]) e = hipMemcpyAsync(fresh[a], *old[a], keep, hipMemcpyDeviceToDevice, D->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    for (int a = 0; a < arrays; a++) *old[a] = std::move(fresh[a]);
    D->capacity = units;
    return hipSuccess;
}

// the units of an extraction, in the map's (lexicographic) order, on the device
hipError_t upload_unit_list(TsdfDevice *D, UnitList *out)
{
    const size_t n = D->cfg.scalable ? D->slot_of.size() : 1;
    std::vector<int> keys(3 * n, 0), slots(n, 0);
    std::vector<double> origins(3 * n);
    if (D->cfg.scalable) {
        size_t u = 0;
        for (const auto &kv : D->slot_of) {
            for (int a = 0; a < 3; a++) { keys[3 * u + a] = kv.first[a]; origins[3 * u + a] = (double)kv.first[a] * D->unit_length(); }
            slots[u++] = kv.second;
        }
    } else {
        for (int a = 0; a < 3; a++) origins[a] = D->cfg.origin[a];
    }
    DEV_RESERVE(D->x_keys, 3 * n);
    DEV_RESERVE(D->x_slots, n);
    DEV_RESERVE(D->x_origins, 3 * n);
    if (n) {
        VISMA_TRY(hipMemcpyAsync(D->x_keys, keys.data(), sizeof(int) * 3 * n, hipMemcpyHostToDevice, D->stream));
        VISMA_TRY(hipMemcpyAsync(D->x_slots, slots.data(), sizeof(int) * n, hipMemcpyHostToDevice, D->stream));
        VISMA_TRY(hipMemcpyAsync(D->x_origins, origins.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, D->stream));
        VISMA_TRY(hipStreamSynchronize(D->stream));           // (the vectors are this function's)
    }
    out->keys = D->x_keys; out->slots = D->x_slots; out->origins = D->x_origins; out->n = (int)n;
    return hipSuccess;
}

}  // namespace

void tsdf_device_destroy(TsdfDevice *D) { delete D; }

// Reset(): a uniform volume's voxels to zero; a scalable volume forgets its units (a slot is zeroed when it is handed out)
hipError_t tsdf_device_reset(TsdfDevice *D)
{
    D->rows[0] = D->rows[1] = -1;
    D->mesh_nv = D->mesh_nt = -1;
    D->integrated = false;
    D->slot_of.clear();
    const size_t bytes = sizeof(float) * D->R3 * D->capacity;
    VISMA_TRY(hipMemsetAsync(D->tsdf, 0, bytes, D->stream));
    VISMA_TRY(hipMemsetAsync(D->weight, 0, bytes, D->stream));
    for (int c = 0; c < D->planes(); c++) VISMA_TRY(hipMemsetAsync(D->color[c], 0, bytes, D->stream));
    return hipStreamSynchronize(D->stream);
}

hipError_t tsdf_device_create(const TsdfConfig &cfg, hipStream_t stream, TsdfDevice **out)
{
    *out = nullptr;
    TsdfDevice *D = new TsdfDevice;
    D->cfg = cfg; D->stream = stream;
    const int R = cfg.resolution;
    D->R3 = (size_t)R * R * R;
    hipError_t e = pool_resize(D, cfg.scalable ? (size_t)std::max(cfg.initial_units, 1) : 1);
    if (e == hipSuccess) e = (hipError_t)D->zs.reset((size_t)R);
    if (e == hipSuccess) {
        // ExtractVoxelPointCloud's pt(2): half_voxel_length, then += voxel_length_ per voxel, in f64
        std::vector<double> zs((size_t)R);
        const double vl = D->unit_voxel_length();
        double z = vl * 0.5;
        for (int k = 0; k < R; k++, z += vl) zs[(size_t)k] = z;
        e = hipMemcpy(D->zs, zs.data(), sizeof(double) * (size_t)R, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { tsdf_device_destroy(D); (void)hipGetLastError(); return e; }
    *out = D;
    return hipSuccess;
}

// CreateDepthToCameraDistanceMultiplierFloatImage (ImageFactory.cpp): the one copy, for a volume's frames and for
// visma_icp_image_distance_multiplier
hipError_t launch_tsdf_multiplier(float *out, int w, int h, double fx, double fy, double cx, double cy, hipStream_t stream)
{
    if (w <= 0 || h <= 0) return hipSuccess;
    multiplier_kernel<<<capped_blocks((long long)w * h), kThreads, 0, stream>>>(out, w, h, (float)cx, (float)cy, 1.0f / (float)fx, 1.0f / (float)fy);
    return hipGetLastError();
}

hipError_t tsdf_device_integrate(TsdfDevice *D, const TsdfFrame &f, const double pose[16])
{
    const TsdfConfig &c = D->cfg;
    const size_t n = (size_t)f.w * f.h;
    const hipMemcpyKind kind = f.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    DEV_RESERVE(D->depth, n);
    VISMA_TRY(hipMemcpyAsync(D->depth, f.depth, sizeof(float) * n, kind, D->stream));
    if (c.color_type == kTsdfColorRgb8) {
        DEV_RESERVE(D->rgb, 3 * n);
        VISMA_TRY(hipMemcpyAsync(D->rgb, f.color, 3 * n, kind, D->stream));
    } else if (c.color_type == kTsdfColorGray32) {
        DEV_RESERVE(D->gray, n);
        VISMA_TRY(hipMemcpyAsync(D->gray, f.color, sizeof(float) * n, kind, D->stream));
    }
    // the units of this frame: the one of a uniform volume, or the touched ones, every one of them open before any kernel
    // of the integration starts
    std::vector<TsdfUnit> list;
    if (!c.scalable) {
        list.push_back({0, (float)c.origin[0], (float)c.origin[1], (float)c.origin[2]});
    } else {
        const long long sw = ((long long)f.w - 1) / c.stride + 1, sh = ((long long)f.h - 1) / c.stride + 1, items = sw * sh;
        DepthSource s;
        s.depth = D->depth; s.gray = nullptr; s.rgb = nullptr;
        s.w = f.w; s.sw = (int)sw; s.stride = c.stride; s.color_type = kTsdfColorNone;
        s.fx = f.fx; s.fy = f.fy; s.cx = f.cx; s.cy = f.cy;
        for (int i = 0; i < 12; i++) s.pose[i] = pose[i];
        s.points = nullptr; s.colors = nullptr;
        DEV_RESERVE(D->bounds, (size_t)items);
        touched_kernel<<<capped_blocks(items), kThreads, 0, D->stream>>>(s, items, c.sdf_trunc, D->unit_length(), D->bounds);
        VISMA_TRY(hipGetLastError());
        std::vector<TouchedBox> b((size_t)items);
        VISMA_TRY(hipMemcpyAsync(b.data(), D->bounds, sizeof(TouchedBox) * b.size(), hipMemcpyDeviceToHost, D->stream));
        VISMA_TRY(hipStreamSynchronize(D->stream));
        const std::set<std::array<int, 3>> touched = expand_touched_boxes(b.data(), b.size());
        if (touched.empty()) return hipSuccess;          // nothing is launched with an empty list
        size_t next = D->slot_of.size();
        std::vector<std::array<int, 3>> opened;
        for (const auto &k : touched)
            if (!D->slot_of.count(k)) opened.push_back(k);
        const size_t need = next + opened.size();
        if (need > D->capacity) {
            const hipError_t e = pool_resize(D, std::max(need, 2 * D->capacity));
            if (e != hipSuccess) return e;               // (no unit was opened: the volume is as it was)
        }
        if (!opened.empty()) {                           // the slots handed out are zeroed: a Reset() leaves old voxels in them
            const size_t at = D->R3 * next, bytes = sizeof(float) * D->R3 * opened.size();
            VISMA_TRY(hipMemsetAsync(D->tsdf + at, 0, bytes, D->stream));
            VISMA_TRY(hipMemsetAsync(D->weight + at, 0, bytes, D->stream));
            for (int p = 0; p < D->planes(); p++) VISMA_TRY(hipMemsetAsync(D->color[p] + at, 0, bytes, D->stream));
        }
        for (const auto &k : opened) D->slot_of[k] = (int)next++;
        for (const auto &k : touched)
            list.push_back({D->slot_of[k], (float)((double)k[0] * D->unit_length()), (float)((double)k[1] * D->unit_length()),
                            (float)((double)k[2] * D->unit_length())});
    }
    DEV_RESERVE(D->unit_list, list.size());
    VISMA_TRY(hipMemcpyAsync(D->unit_list, list.data(), sizeof(TsdfUnit) * list.size(), hipMemcpyHostToDevice, D->stream));
    const float fx = (float)f.fx, fy = (float)f.fy, cx = (float)f.cx, cy = (float)f.cy;
    const double k[4] = {f.fx, f.fy, f.cx, f.cy};
    if (!D->mult || D->mult_w != f.w || D->mult_h != f.h || std::memcmp(k, D->mult_k, sizeof(k)) != 0) {
        D->mult_w = 0;
        DEV_RESERVE(D->mult, n);
        VISMA_TRY(launch_tsdf_multiplier(D->mult, f.w, f.h, f.fx, f.fy, f.cx, f.cy, D->stream));
        D->mult_w = f.w; D->mult_h = f.h;
        std::memcpy(D->mult_k, k, sizeof(k));
    }
    IntegrateArgs a;
    a.tsdf = D->tsdf; a.weight = D->weight; a.c0 = D->color[0]; a.c1 = D->color[1]; a.c2 = D->color[2];
    a.units = D->unit_list; a.n_units = (int)list.size();
    a.R = c.resolution;
    a.depth = D->depth; a.mult = D->mult; a.gray = D->gray; a.rgb = D->rgb;
    a.w = f.w; a.h = f.h;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.vl = (float)D->unit_voxel_length();
    a.half = a.vl * 0.5f;
    a.trunc = (float)c.sdf_trunc;
    a.trunc_inv = 1.0f / a.trunc;
    for (int i = 0; i < 12; i++) a.e[i] = (float)f.extrinsic[i];
    for (int r = 0; r < 3; r++) a.es[r] = a.e[4 * r + 2] * a.vl;
    a.safe_w = (float)f.w - 0.0001f; a.safe_h = (float)f.h - 0.0001f;
    const unsigned blocks = capped_blocks((long long)c.resolution * c.resolution * (long long)list.size());
    if (c.color_type == kTsdfColorRgb8) integrate_kernel<kTsdfColorRgb8><<<blocks, kThreads, 0, D->stream>>>(a);
    else if (c.color_type == kTsdfColorGray32) integrate_kernel<kTsdfColorGray32><<<blocks, kThreads, 0, D->stream>>>(a);
    else integrate_kernel<kTsdfColorNone><<<blocks, kThreads, 0, D->stream>>>(a);
    VISMA_TRY(hipGetLastError());
    D->rows[0] = D->rows[1] = -1;
    D->mesh_nv = D->mesh_nt = -1;
    D->integrated = true;
    return hipStreamSynchronize(D->stream);
}

hipError_t tsdf_device_extract(TsdfDevice *D, int voxel_cloud, int64_t *n)
{
    const TsdfConfig &c = D->cfg;
    const int which = voxel_cloud ? 1 : 0;
    D->rows[which] = -1;
    *n = 0;
    long long rows = 0;
    UnitList units;
    VISMA_TRY(upload_unit_list(D, &units));
    const long long items = (long long)D->R3 * units.n;
    if (voxel_cloud) {
        const double vl = D->unit_voxel_length();
        VoxelCloudSource s = {D->tsdf, D->weight, D->zs, units, c.resolution, vl, vl * 0.5, nullptr, nullptr};
        VISMA_TRY(compact_count(D->comp, s, items, D->stream, &rows));
        DEV_RESERVE(D->out_points[1], 3 * (size_t)rows);
        DEV_RESERVE(D->out_colors[1], 3 * (size_t)rows);
        s.points = D->out_points[1]; s.colors = D->out_colors[1];
        if (rows > 0) VISMA_TRY(compact_write(D->comp, s, items, D->stream));
    } else {
        auto outputs = [&]() -> hipError_t {
            DEV_RESERVE(D->out_points[0], 3 * (size_t)rows);
            DEV_RESERVE(D->out_normals, 3 * (size_t)rows);
            DEV_RESERVE(D->out_colors[0], 3 * (size_t)rows);
            return hipSuccess;
        };
        if (c.scalable) {
            ScalableSurfaceSource s = {D->tsdf, D->weight, D->color[0], D->color[1], D->color[2], units, c.resolution, c.color_type,
                                       c.voxel_length, c.voxel_length * 0.5, D->unit_length(), nullptr, nullptr, nullptr};
            VISMA_TRY(compact_count(D->comp, s, items, D->stream, &rows));
            VISMA_TRY(outputs());
            s.points = D->out_points[0]; s.normals = D->out_normals; s.colors = D->out_colors[0];
            if (rows > 0) VISMA_TRY(compact_write(D->comp, s, items, D->stream));
        } else {
            const double vl = D->unit_voxel_length();
            SurfaceSource s = {D->tsdf, D->weight, D->color[0], D->color[1], D->color[2], c.resolution, c.color_type, vl, vl * 0.5,
                               c.origin[0], c.origin[1], c.origin[2], nullptr, nullptr, nullptr};
            VISMA_TRY(compact_count(D->comp, s, items, D->stream, &rows));
            VISMA_TRY(outputs());
            s.points = D->out_points[0]; s.normals = D->out_normals; s.colors = D->out_colors[0];
            if (rows > 0) VISMA_TRY(compact_write(D->comp, s, items, D->stream));
        }
    }
    VISMA_TRY(hipStreamSynchronize(D->stream));
    D->rows[which] = rows;
    *n = (int64_t)rows;
    return hipSuccess;
}

hipError_t tsdf_device_get_extract(TsdfDevice *D, int voxel_cloud, double *points, double *normals, double *colors)
{
    const int which = voxel_cloud ? 1 : 0;
    const long long rows = D->rows[which];
    if (rows <= 0) return hipSuccess;
    const size_t bytes = sizeof(double) * 3 * (size_t)rows;
    if (points) VISMA_TRY(hipMemcpy(points, D->out_points[which], bytes, hipMemcpyDeviceToHost));
    if (normals && !voxel_cloud) VISMA_TRY(hipMemcpy(normals, D->out_normals, bytes, hipMemcpyDeviceToHost));
    if (colors && (voxel_cloud || D->planes() > 0)) VISMA_TRY(hipMemcpy(colors, D->out_colors[which], bytes, hipMemcpyDeviceToHost));
    return hipSuccess;
}

namespace {

template <class Grid>
hipError_t extract_mesh(TsdfDevice *D, MeshArgs<Grid> a, long long items, long long *nv, long long *nt)
{
    cube_kernel<Grid><<<capped_blocks(items), kThreads, 0, D->stream>>>(a, items);
    VISMA_TRY(hipGetLastError());
    MeshVertexSource<Grid> vs = {a};
    VISMA_TRY(compact_count(D->comp, vs, items, D->stream, nv));
    if (*nv > 0x7fffffffLL) return hipErrorInvalidValue;
    if (*nv == 0) return hipSuccess;                     // no vertex, no triangle
    DEV_RESERVE(D->mesh_vertices, 3 * (size_t)*nv);
    if (D->planes() > 0) DEV_RESERVE(D->mesh_colors, 3 * (size_t)*nv);
    vs.a.vertices = D->mesh_vertices.get(); vs.a.colors = D->mesh_colors.get();
    vs.a.vert_tile_offset = D->comp.tile_offset.get();
    VISMA_TRY(compact_write(D->comp, vs, items, D->stream));
    MeshTriangleSource<Grid> ts = {vs.a};
    VISMA_TRY(compact_count(D->comp_tri, ts, items, D->stream, nt));
    if (*nt > 0x7fffffffLL) return hipErrorInvalidValue;
    if (*nt == 0) return hipSuccess;
    DEV_RESERVE(D->mesh_triangles, 3 * (size_t)*nt);
    ts.a.triangles = D->mesh_triangles.get();
    return compact_write(D->comp_tri, ts, items, D->stream);
}

}  // namespace

hipError_t tsdf_device_extract_mesh(TsdfDevice *D, int64_t *nv, int64_t *nt)
{
    const TsdfConfig &c = D->cfg;
    D->mesh_nv = D->mesh_nt = -1;
    *nv = *nt = 0;
    long long n_vertices = 0, n_triangles = 0;
    // nothing is launched over a volume without a cube or without a frame
    const bool empty = !D->integrated || (c.scalable ? D->slot_of.empty() : c.resolution < 2);
    if (!empty) {
        UnitList units;
        VISMA_TRY(upload_unit_list(D, &units));
        const long long items = (long long)D->R3 * units.n;
        DEV_RESERVE(D->cube_rec, (size_t)items);
        DEV_RESERVE(D->vert_rec, (size_t)items);
        if (!D->mc_cases) {
            const McTable &t = mc_table();
            for (const McCase &cs : t.c)
                if (cs.n > kMcMaxTriangles) return hipErrorUnknown;          // (the rule gave more than a row holds: never)
            DEV_RESERVE(D->mc_cases, 256);
            const hipError_t e = hipMemcpyAsync(D->mc_cases.get(), t.c, sizeof(t.c), hipMemcpyHostToDevice, D->stream);   // (a static table)
            if (e != hipSuccess) { D->mc_cases.release(); return e; }
        }
        hipError_t e;
        if (c.scalable) {
            MeshArgs<ScalableGrid> a = {{units, c.resolution}, D->tsdf, D->weight, D->color[0], D->color[1], D->color[2], c.color_type,
                                        c.voxel_length, c.voxel_length * 0.5, 0.0, 0.0, 0.0, D->cube_rec.get(), D->vert_rec.get(),
                                        D->mc_cases.get(), nullptr, nullptr, nullptr, nullptr};
            e = extract_mesh(D, a, items, &n_vertices, &n_triangles);
        } else {
            const double vl = D->unit_voxel_length();
            MeshArgs<UniformGrid> a = {{c.resolution}, D->tsdf, D->weight, D->color[0], D->color[1], D->color[2], c.color_type,
                                       vl, vl * 0.5, c.origin[0], c.origin[1], c.origin[2], D->cube_rec.get(), D->vert_rec.get(),
                                       D->mc_cases.get(), nullptr, nullptr, nullptr, nullptr};
            e = extract_mesh(D, a, items, &n_vertices, &n_triangles);
        }
        if (e != hipSuccess) { (void)hipStreamSynchronize(D->stream); return e; }
        VISMA_TRY(hipStreamSynchronize(D->stream));
    }
    D->mesh_nv = n_vertices; D->mesh_nt = n_triangles;
    *nv = (int64_t)n_vertices; *nt = (int64_t)n_triangles;
    return hipSuccess;
}

hipError_t tsdf_device_get_mesh(TsdfDevice *D, double *vertices, double *colors, int32_t *triangles)
{
    if (D->mesh_nv > 0) {
        const size_t bytes = sizeof(double) * 3 * (size_t)D->mesh_nv;
        if (vertices) VISMA_TRY(hipMemcpy(vertices, D->mesh_vertices.get(), bytes, hipMemcpyDeviceToHost));
        if (colors && D->planes() > 0) VISMA_TRY(hipMemcpy(colors, D->mesh_colors.get(), bytes, hipMemcpyDeviceToHost));
    }
    if (D->mesh_nt > 0 && triangles)
        VISMA_TRY(hipMemcpy(triangles, D->mesh_triangles.get(), sizeof(int32_t) * 3 * (size_t)D->mesh_nt, hipMemcpyDeviceToHost));
    return hipSuccess;
}

bool tsdf_device_mesh_view(const TsdfDevice *D, TsdfMeshView *view)
{
    if (D->mesh_nv < 0) return false;
    view->vertices = D->mesh_vertices.get();
    view->colors = D->planes() > 0 ? D->mesh_colors.get() : nullptr;
    view->triangles = D->mesh_triangles.get();
    view->nv = D->mesh_nv; view->nt = D->mesh_nt;
    return true;
}

bool tsdf_device_cloud_view(const TsdfDevice *D, int voxel_cloud, TsdfCloudView *view)
{
    const int which = voxel_cloud ? 1 : 0;
    if (D->rows[which] < 0) return false;
    view->n = D->rows[which];
    view->points = D->out_points[which].get();
    view->normals = voxel_cloud ? nullptr : D->out_normals.get();
    view->colors = (voxel_cloud || D->planes() > 0) ? D->out_colors[which].get() : nullptr;
    return true;
}

void tsdf_device_get_units(const TsdfDevice *D, std::vector<int32_t> *keys)
{
    keys->clear();
    for (const auto &kv : D->slot_of)
        for (int a = 0; a < 3; a++) keys->push_back(kv.first[a]);
}

hipError_t tsdf_device_get_volume(TsdfDevice *D, const int32_t *unit, float *tsdf, float *weight, float *color)
{
    size_t slot = 0;
    if (D->cfg.scalable) {
        if (!unit) return hipErrorInvalidValue;
        const auto it = D->slot_of.find({unit[0], unit[1], unit[2]});
        if (it == D->slot_of.end()) return hipErrorInvalidValue;
        slot = (size_t)it->second;
    }
    const size_t at = slot * D->R3, bytes = sizeof(float) * D->R3;
    if (tsdf) VISMA_TRY(hipMemcpy(tsdf, D->tsdf + at, bytes, hipMemcpyDeviceToHost));
    if (weight) VISMA_TRY(hipMemcpy(weight, D->weight + at, bytes, hipMemcpyDeviceToHost));
    if (color && D->planes() > 0) {
        // plane by plane in pieces of 4 M voxels (16 MB on the host whatever the resolution), interleaved as the reference
        // keeps the colour; Gray32: the one plane, three times
        const size_t piece = (size_t)1 << 22;
        std::vector<float> buf(std::min(piece, D->R3));
        for (size_t v0 = 0; v0 < D->R3; v0 += piece) {
            const size_t m = std::min(piece, D->R3 - v0);
            for (int c = 0; c < 3; c++) {
                if (c < D->planes()) VISMA_TRY(hipMemcpy(buf.data(), D->color[c] + at + v0, sizeof(float) * m, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < m; i++) color[3 * (v0 + i) + (size_t)c] = buf[i];
            }
        }
    }
    return hipSuccess;
}

hipError_t point_cloud_from_depth_device(const TsdfFrame &f, const double pose[16], int color_type, int stride, double *points,
                                         double *colors, int64_t *n, hipStream_t stream, CloudDevice **cloud)
{
    *n = 0;
    if (cloud) *cloud = nullptr;
    const hipMemcpyKind kind = f.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t px = (size_t)f.w * f.h;
    const long long sw = ((long long)f.w - 1) / stride + 1, sh = ((long long)f.h - 1) / stride + 1, items = sw * sh;
    DeviceBuf<float> d_depth, d_gray;
    DeviceBuf<uint8_t> d_rgb;
    DeviceBuf<double> d_points, d_colors;
    Compactor comp;
    // (a return with work in flight is safe: the buffers' hipFree waits for the device before the caller has its arrays back)
    DEV_RESET(d_depth, px);
    VISMA_TRY(hipMemcpyAsync(d_depth, f.depth, sizeof(float) * px, kind, stream));
    if (color_type == kTsdfColorRgb8) {
        DEV_RESET(d_rgb, 3 * px);
        VISMA_TRY(hipMemcpyAsync(d_rgb, f.color, 3 * px, kind, stream));
    } else if (color_type == kTsdfColorGray32) {
        DEV_RESET(d_gray, px);
        VISMA_TRY(hipMemcpyAsync(d_gray, f.color, sizeof(float) * px, kind, stream));
    }
    DepthSource s;
    s.depth = d_depth; s.gray = d_gray; s.rgb = d_rgb;
    s.w = f.w; s.sw = (int)sw; s.stride = stride; s.color_type = color_type;
    s.fx = f.fx; s.fy = f.fy; s.cx = f.cx; s.cy = f.cy;
    for (int i = 0; i < 12; i++) s.pose[i] = pose[i];
    s.points = nullptr; s.colors = nullptr;
    long long rows = 0;
    VISMA_TRY(compact_count(comp, s, items, stream, &rows));
    *n = (int64_t)rows;
    if (rows == 0 && cloud) return cloud_device_create(nullptr, 0, nullptr, nullptr, true, stream, cloud);
    if (rows == 0 || (!points && !cloud)) return hipSuccess;
    const size_t bytes = sizeof(double) * 3 * (size_t)rows;
    DEV_RESET(d_points, 3 * (size_t)rows);
    if (color_type != kTsdfColorNone) DEV_RESET(d_colors, 3 * (size_t)rows);
    s.points = d_points; s.colors = d_colors;
    VISMA_TRY(compact_write(comp, s, items, stream));
    if (cloud) return cloud_device_create(d_points, (int64_t)rows, nullptr, d_colors ? d_colors.get() : nullptr, true, stream, cloud);   // device to device
    VISMA_TRY(hipMemcpyAsync(points, d_points, bytes, hipMemcpyDeviceToHost, stream));
    if (colors && d_colors) VISMA_TRY(hipMemcpyAsync(colors, d_colors, bytes, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

}  // namespace visma
