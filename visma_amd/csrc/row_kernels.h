// row_kernels.h -- the two kernels over n x 3 f64 rows that the resident TriangleMesh (trimesh.hip) and the resident
// PointCloud (cloud.hip) share: Transform and NormalizeNormals.  One copy of the text; each including file gets its own
// compiled copy (unnamed namespace), as with compact.h, whose launch shape (grid-capped stride loops of kThreads lanes)
// they have.
#pragma once

#include "compact.h"

namespace visma {

namespace {

#define ROW_LOOP(i, n) \
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < (n); i += (long long)gridDim.x * kThreads)

// Eigen's normalize() (Dot.h: z = squaredNorm(); if (z > 0) derived() /= sqrt(z)); nan_rule: then TriangleMesh.h's rule on x
// (a NaN there makes the row (0, 0, 1)), which PointCloud.h's NormalizeNormals does not have
__global__ __launch_bounds__(kThreads) void rows_normalize(double *a, long long n, bool nan_rule)
{
    ROW_LOOP(i, n) {
        double x = a[3 * i], y = a[3 * i + 1], z = a[3 * i + 2];
        const double n2 = (x * x + y * y) + z * z;
        if (n2 > 0.0) {
            const double len = sqrt(n2);
            x = x / len; y = y / len; z = z / len;
        }
        if (nan_rule && isnan(x)) { x = 0.0; y = 0.0; z = 1.0; }
        a[3 * i] = x; a[3 * i + 1] = y; a[3 * i + 2] = z;
    }
}

// ---- Transform: a row is ((T_i0 x + T_i1 y) + T_i2 z) + T_i3 w, w = 1 for points and 0 for normals ---------------------
struct Mat34 {
    double m[12];
    explicit Mat34(const double T[16]) { for (int i = 0; i < 12; i++) m[i] = T[i]; }   // (the fourth row is not read)
};
__global__ __launch_bounds__(kThreads) void rows_transform(double *a, long long n, Mat34 T, double w)
{
    ROW_LOOP(i, n) {
        const double x = a[3 * i], y = a[3 * i + 1], z = a[3 * i + 2];
        for (int r = 0; r < 3; r++)
            a[3 * i + r] = ((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3] * w;
    }
}

}  // namespace

}  // namespace visma
