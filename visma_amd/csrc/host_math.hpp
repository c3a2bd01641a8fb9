// host_math.hpp -- the tiny f64 solves of the ICP loop.  Every function is
// host+device: the synchronous API solves on the host, the asynchronous
// on-device loop (icp_loop.hip) runs the very same code in a one-thread kernel.
//
// The reference does these with Eigen (umeyama / JacobiSVD / LDLT).  Eigen is
// not a dependency of this library (there is none on the target image), so the
// few fixed-size operations needed are written out here:
//   kabsch_from_stats   Eigen/src/Geometry/Umeyama.h:118-159 evaluated from the
//                       reduced moments instead of from gathered 3xK matrices
//   gn_from_stats       O3D/Core/Utility/Eigen.cpp:35-56,88-106 (6x6 solve with
//                       the |det| < 1e-6 guard) + :58-68 (Euler ZYX) or the
//                       exponential map of core/rodrigues.h:143-182
// All matrices row-major.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "so3.h"

namespace visma {

struct Mat4 {
    double m[16];
    VISMA_HD static Mat4 identity()
    {
        Mat4 r;
        for (int i = 0; i < 16; i++) r.m[i] = 0.0;
        r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.0;
        return r;
    }
    VISMA_HD static Mat4 from(const double *p)
    {
        Mat4 r;
        for (int i = 0; i < 16; i++) r.m[i] = p[i];
        return r;
    }
    VISMA_HD double &operator()(int i, int j) { return m[i * 4 + j]; }
    VISMA_HD double operator()(int i, int j) const { return m[i * 4 + j]; }
};

VISMA_HD Mat4 operator*(const Mat4 &a, const Mat4 &b)
{
    Mat4 r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += a(i, k) * b(k, j);
            r(i, j) = s;
        }
    return r;
}

// x' = x - c  ==>  [R | t]  <->  [R | R c + t - c]
VISMA_HD Mat4 to_centred(const Mat4 &T, const double c[3])
{
    Mat4 r = T;
    for (int i = 0; i < 3; i++)
        r(i, 3) = T(i, 0) * c[0] + T(i, 1) * c[1] + T(i, 2) * c[2] + T(i, 3) - c[i];
    return r;
}

VISMA_HD Mat4 from_centred(const Mat4 &Tc, const double c[3])
{
    Mat4 r = Tc;
    for (int i = 0; i < 3; i++)
        r(i, 3) = Tc(i, 3) - (Tc(i, 0) * c[0] + Tc(i, 1) * c[1] + Tc(i, 2) * c[2]) + c[i];
    return r;
}

VISMA_HD double det3(const double A[9])
{
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) +
           A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// Singular value decomposition of a 3x3 by one-sided Jacobi rotations on the
// columns (A V = U S); singular values sorted descending, U completed to a
// full orthonormal basis when A is rank deficient.
VISMA_HD void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

struct Svd3 {
    double U[9], s[3], V[9];
};

// Written so that every array index is a compile-time constant after unrolling: on the GPU
// (one-thread epilogue of the batched device loop) the first version indexed G / W / the sort
// permutation dynamically, which put them in scratch memory -- 720 B of private segment and
// most of the 8 us the solve took.  Same operations in the same order as before.
VISMA_HD Svd3 svd3(const double A[9])
{
    double G[3][3], W[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = A[i * 3 + j];
    // Convergence: every column pair orthogonal to 2 ulp (|g| <= 4.4e-16 sqrt(ab)).
    // A tighter bound only burns sweeps (each rotation is a chain of dependent f64
    // div/sqrt) without changing R.
    bool any = false;
    auto rotate = [&](const int p, const int q) {
        double a = 0, b = 0, g = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            a += G[r][p] * G[r][p];
            b += G[r][q] * G[r][q];
            g += G[r][p] * G[r][q];
        }
        if (g == 0.0 || g * g <= 1.9e-31 * (a * b)) return;
        any = true;
        const double zeta = (b - a) / (2.0 * g);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double gp = G[r][p], gq = G[r][q];
            G[r][p] = c * gp - s * gq;
            G[r][q] = s * gp + c * gq;
            const double wp = W[r][p], wq = W[r][q];
            W[r][p] = c * wp - s * wq;
            W[r][q] = s * wp + c * wq;
        }
    };
    for (int sweep = 0; sweep < 30; sweep++) {
        any = false;
        rotate(0, 1);
        rotate(0, 2);
        rotate(1, 2);
        if (!any) break;
    }
    double n[3];
#pragma unroll
    for (int j = 0; j < 3; j++) n[j] = sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]);
    // columns by descending norm: the same three comparisons as a sort of an index permutation
    // (a, b) = (0,1), (0,2), (1,2), carried out on the columns themselves
    auto order = [&](const int a, const int b) {
        if (n[b] > n[a]) {
            const double t = n[a]; n[a] = n[b]; n[b] = t;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double tg = G[r][a]; G[r][a] = G[r][b]; G[r][b] = tg;
                const double tw = W[r][a]; W[r][a] = W[r][b]; W[r][b] = tw;
            }
        }
    };
    order(0, 1);
    order(0, 2);
    order(1, 2);
    Svd3 out;
    double u[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        out.s[j] = n[j];
#pragma unroll
        for (int r = 0; r < 3; r++) out.V[r * 3 + j] = W[r][j];
        if (n[j] > 1e-300 && n[j] > 1e-15 * n[0]) {
#pragma unroll
            for (int r = 0; r < 3; r++) u[j][r] = G[r][j] / n[j];
            rank = j + 1;
        }
    }
    if (rank == 0) {
        // zero matrix: no rotation is needed; U = V = I, which is also what the
        // reference's JacobiSVD returns (so the update is a pure translation)
#pragma unroll
        for (int i = 0; i < 9; i++) out.U[i] = out.V[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return out;
    }
    if (rank == 1) {
        // the axis along which u0 is smallest (first one on ties), crossed with u0
        int m = 0;
        double mv = fabs(u[0][0]);
        if (fabs(u[0][1]) < mv) { m = 1; mv = fabs(u[0][1]); }
        if (fabs(u[0][2]) < mv) { m = 2; }
        const double e[3] = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
        cross3(u[0], e, u[1]);
        const double l = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
#pragma unroll
        for (int r = 0; r < 3; r++) u[1][r] /= l;
        rank = 2;
    }
    if (rank == 2) cross3(u[0], u[1], u[2]);
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int r = 0; r < 3; r++) out.U[r * 3 + j] = u[j][r];
    return out;
}

// projectSO3 (core/rodrigues.h:229-237) and SO3Type::fitToSO3 (core/se3.h:58-61): U V^T of the SVD,
// the orthogonal factor nearest to A (no determinant fix, like the reference: a reflection stays one).
VISMA_HD void project_so3(const double A[9], double R[9])
{
    const Svd3 d = svd3(A);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            R[i * 3 + j] = d.U[i * 3] * d.V[j * 3] + d.U[i * 3 + 1] * d.V[j * 3 + 1] + d.U[i * 3 + 2] * d.V[j * 3 + 2];
}

// The rotation nearest to A -- the orthogonal polar factor Q of A = Q H -- by Newton's iteration
// X <- (X + X^-T) / 2 from X0 = A / |A|_F (Higham, "Computing the polar decomposition -- with applications", 1986):
// the singular vectors of X never change, every singular value s goes to (s + 1/s) / 2 -> 1 quadratically, and
// det X keeps its sign.  For det A > 0 that Q is exactly Umeyama's U S V^T (Umeyama.h:118-159: S = I when
// det U det V > 0), with tr(Q^T A) the sum of A's singular values -- WITHOUT the one-sided Jacobi sweeps of svd3,
// whose ~18 rotations are a chain of dependent f64 divisions and square roots: 9 us in one GPU thread (the solve
// launch between every two search launches of a batch: 18 % of config 3's GPU time until round 5) against ~1 us
// here (one division per step, 8-13 steps).  Only +, -, x, / in a fixed order: host and device agree bit for bit.
// Returns false -- the caller then takes the SVD path -- for det A <= 0 (a reflection is nearest: Umeyama flips the
// smallest singular direction, which only the SVD names), for a matrix too close to singular for the inverse to be
// trusted, and for non-finite input.  "Too close": the first step inverts X0, and a Newton step from an X0 with singular
// values s1 >= s2 >= s3 loses ~2e-17 / (s3 / s1) of the singular VECTORS for good (measured: |Q - U V^T| = 2e-12 at
// s3 / s1 = 1e-5, 6e-11 at 3e-7 -- walls and floors seen at an angle land there).  The SVD path is good to
// 1e-16 at any conditioning, so the Newton path is taken only from det X0 >= 1e-3 (|X0|_F = 1: s3 / s1 >~ 2e-3, error
// <~ 1e-14) and everything thinner -- nearly planar, planar, collinear sets, a handful of pairs -- goes to svd3.
VISMA_HD bool polar_rotation3(const double A[9], double Q[9])
{
    double f2 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) f2 += A[i] * A[i];
    if (!(f2 > 0.0) || !(f2 < 1e300)) return false;
    const double inv_f = 1.0 / sqrt(f2);
    double X[9];
#pragma unroll
    for (int i = 0; i < 9; i++) X[i] = A[i] * inv_f;
    for (int it = 0; it < 64; it++) {
        // cofactors: C = det(X) X^-T
        double C[9];
        C[0] = X[4] * X[8] - X[5] * X[7];
        C[1] = X[5] * X[6] - X[3] * X[8];
        C[2] = X[3] * X[7] - X[4] * X[6];
        C[3] = X[2] * X[7] - X[1] * X[8];
        C[4] = X[0] * X[8] - X[2] * X[6];
        C[5] = X[1] * X[6] - X[0] * X[7];
        C[6] = X[1] * X[5] - X[2] * X[4];
        C[7] = X[2] * X[3] - X[0] * X[5];
        C[8] = X[0] * X[4] - X[1] * X[3];
        const double det = X[0] * C[0] + X[1] * C[1] + X[2] * C[2];
        // (|X0|_F = 1: det X0 = s1 s2 s3 <= 3^-3/2; later iterates have every s >= 1)
        if (!(det > (it == 0 ? 1e-3 : 0.5))) return false;
        const double inv = 1.0 / det;
        double d2 = 0.0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const double xn = 0.5 * (X[i] + C[i] * inv);
            const double d = xn - X[i];
            d2 += d * d;
            X[i] = xn;
        }
        // quadratic convergence: a step below 1e-8 leaves an error of ~1e-16 -- one more step then changes nothing
        // above rounding
        if (d2 < 1e-16) {
#pragma unroll
            for (int i = 0; i < 9; i++) Q[i] = X[i];
            return true;
        }
    }
    return false;
}

struct NormalEq {
    double K, r2;
    double JTJ[36];
    double JTr[6];
    double M[9];  // sum q p^T
};

VISMA_HD NormalEq unpack_stats(const double *st)
{
    NormalEq e;
    e.K = st[0];
    e.r2 = st[1];
    int o = 2;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) {
            e.JTJ[a * 6 + b] = st[o];
            e.JTJ[b * 6 + a] = st[o];
            ++o;
        }
    for (int a = 0; a < 6; a++) e.JTr[a] = st[o++];
    for (int a = 0; a < 9; a++) e.M[a] = st[o++];
    return e;
}

// R = U S V^T of Umeyama (Umeyama.h:139-152) for the cross-covariance sigma, and sum_i s_i S_i (:155-158), returned:
// through the polar factor when det sigma > 0 and sigma is well conditioned (every registration of a real surface), else
// through the SVD
VISMA_HD double umeyama_rotation(const double sigma[9], double R[9])
{
    double strace;
    if (polar_rotation3(sigma, R)) {
        strace = 0.0;                                        // tr(R^T sigma) = s1 + s2 + s3
        for (int i = 0; i < 9; i++) strace += R[i] * sigma[i];
    } else {
        const Svd3 d = svd3(sigma);
        double S[3] = {1.0, 1.0, 1.0};
        if (det3(d.U) * det3(d.V) < 0.0) S[2] = -1.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                R[i * 3 + j] = d.U[i * 3] * S[0] * d.V[j * 3] + d.U[i * 3 + 1] * S[1] * d.V[j * 3 + 1] +
                               d.U[i * 3 + 2] * S[2] * d.V[j * 3 + 2];
        strace = d.s[0] * S[0] + d.s[1] * S[1] + d.s[2] * S[2];
    }
    return strace;
}

// Closed-form least-squares rigid (optionally similarity) update for the
// fixed correspondence set, from the moments.
VISMA_HD Mat4 kabsch_from_stats(const double *st, bool with_scaling)
{
    const NormalEq e = unpack_stats(st);
    if (!(e.K > 0.0)) return Mat4::identity();
    // the cross block of J^T J is hat(sum p); J^T r's tail is sum p - sum q
    const double P[3] = {e.JTJ[2 * 6 + 4], e.JTJ[0 * 6 + 5], e.JTJ[1 * 6 + 3]};
    const double Q[3] = {P[0] - e.JTr[3], P[1] - e.JTr[4], P[2] - e.JTr[5]};
    const double inv = 1.0 / e.K;
    double pm[3], qm[3], sigma[9];
    for (int a = 0; a < 3; a++) { pm[a] = P[a] * inv; qm[a] = Q[a] * inv; }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) sigma[a * 3 + b] = e.M[a * 3 + b] * inv - qm[a] * pm[b];
    double R[9];
    const double strace = umeyama_rotation(sigma, R);
    double c = 1.0;
    if (with_scaling) {
        // tr(sum(|p|^2 I - p p^T)) = 2 sum |p|^2
        const double sum_p2 = 0.5 * (e.JTJ[0] + e.JTJ[7] + e.JTJ[14]);
        const double var = sum_p2 * inv - (pm[0] * pm[0] + pm[1] * pm[1] + pm[2] * pm[2]);
        c = strace / var;
    }
    Mat4 T = Mat4::identity();
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T(i, j) = c * R[i * 3 + j];
        T(i, 3) = qm[i] - c * (R[i * 3] * pm[0] + R[i * 3 + 1] * pm[1] + R[i * 3 + 2] * pm[2]);
    }
    return T;
}

// Solve A x = b (6x6, partial pivoting); returns det(A).
VISMA_HD double solve6(const double A[36], const double b[6], double x[6])
{
    double M[6][7];
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < 6; j++) M[i][j] = A[i * 6 + j];
        M[i][6] = b[i];
    }
    double det = 1.0;
    for (int c = 0; c < 6; c++) {
        int piv = c;
        for (int r = c + 1; r < 6; r++)
            if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
        if (M[piv][c] == 0.0) {
            for (int i = 0; i < 6; i++) x[i] = 0.0;
            return 0.0;
        }
        if (piv != c) {
            for (int j = 0; j < 7; j++) { const double t = M[c][j]; M[c][j] = M[piv][j]; M[piv][j] = t; }
            det = -det;
        }
        det *= M[c][c];
        for (int r = c + 1; r < 6; r++) {
            const double f = M[r][c] / M[c][c];
            for (int j = c; j < 7; j++) M[r][j] -= f * M[c][j];
        }
    }
    for (int r = 5; r >= 0; r--) {
        double s = M[r][6];
        for (int j = r + 1; j < 6; j++) s -= M[r][j] * x[j];
        x[r] = s / M[r][r];
    }
    return det;
}

VISMA_HD Mat4 euler_zyx_to_mat4(const double x[6])
{
    const double ca = cos(x[0]), sa = sin(x[0]);
    const double cb = cos(x[1]), sb = sin(x[1]);
    const double cg = cos(x[2]), sg = sin(x[2]);
    Mat4 T = Mat4::identity();
    // Rz(g) * Ry(b) * Rx(a), written out
    T(0, 0) = cg * cb; T(0, 1) = cg * sb * sa - sg * ca; T(0, 2) = cg * sb * ca + sg * sa;
    T(1, 0) = sg * cb; T(1, 1) = sg * sb * sa + cg * ca; T(1, 2) = sg * sb * ca - cg * sa;
    T(2, 0) = -sb;     T(2, 1) = cb * sa;                T(2, 2) = cb * ca;
    T(0, 3) = x[3]; T(1, 3) = x[4]; T(2, 3) = x[5];
    return T;
}

// One Gauss-Newton step on J^T J x = -J^T r.  ok=false (Identity) when the
// determinant guard rejects the system.
VISMA_HD Mat4 gn_from_stats(const double *st, bool expmap, bool *ok)
{
    const NormalEq e = unpack_stats(st);
    *ok = false;
    if (!(e.K > 0.0)) return Mat4::identity();
    double nb[6], x[6];
    for (int i = 0; i < 6; i++) nb[i] = -e.JTr[i];
    const double det = solve6(e.JTJ, nb, x);
    if (fabs(det) < 1e-6 || isnan(det) || isinf(det)) return Mat4::identity();
    *ok = true;
    if (!expmap) return euler_zyx_to_mat4(x);
    double R[9];
    rodrigues(x, R);
    Mat4 T = Mat4::identity();
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T(i, j) = R[i * 3 + j];
        T(i, 3) = x[3 + i];
    }
    return T;
}

// ---- 4 degrees of freedom: rotation about a fixed unit axis `a` (target frame) + a 3-D translation ----------------------
// (the orientation constrained ICP of the VISMA paper: gravity-aligned scans, yaw only).  DESIGN.md 4.5b.

// R = c I + s [a]x + (1 - c) a a^T: the rotation by the angle with cosine c and sine s about the unit axis a
VISMA_HD void axis_rotation3(const double a[3], double c, double s, double R[9])
{
    const double v = 1.0 - c;
    R[0] = c + v * a[0] * a[0];        R[1] = v * a[0] * a[1] - s * a[2]; R[2] = v * a[0] * a[2] + s * a[1];
    R[3] = v * a[1] * a[0] + s * a[2]; R[4] = c + v * a[1] * a[1];        R[5] = v * a[1] * a[2] - s * a[0];
    R[6] = v * a[2] * a[0] - s * a[1]; R[7] = v * a[2] * a[1] + s * a[0]; R[8] = c + v * a[2] * a[2];
}

// Point-to-point, closed form: the exact least-squares minimiser over rotations about `a` plus a translation for the
// fixed correspondence set (the constrained analogue of Umeyama).  With sigma = sum q p^T / K - qm pm^T (as
// kabsch_from_stats forms it), sum |R p + t - q|^2 is smallest where tr(R^T sigma) = cos A + sin B + a^T sigma a is
// largest: A = tr sigma - a^T sigma a, B = a . vee(sigma - sigma^T), so (cos, sin) = (A, B) / hypot(A, B).  No atan2 /
// sin / cos -- only +, -, x, /, sqrt in a fixed order: host and device agree bit for bit (the build has
// -ffp-contract=off).  A (near-)zero or non-finite hypot (every pair on a line parallel to `a`, K = 0): no rotation.
VISMA_HD Mat4 kabsch_axis_from_stats(const double *st, const double a[3])
{
    const NormalEq e = unpack_stats(st);
    if (!(e.K > 0.0)) return Mat4::identity();
    const double P[3] = {e.JTJ[2 * 6 + 4], e.JTJ[0 * 6 + 5], e.JTJ[1 * 6 + 3]};
    const double Q[3] = {P[0] - e.JTr[3], P[1] - e.JTr[4], P[2] - e.JTr[5]};
    const double inv = 1.0 / e.K;
    double pm[3], qm[3], sigma[9];
    for (int i = 0; i < 3; i++) { pm[i] = P[i] * inv; qm[i] = Q[i] * inv; }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) sigma[i * 3 + j] = e.M[i * 3 + j] * inv - qm[i] * pm[j];
    double asa = 0.0, m2 = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            asa += a[i] * sigma[i * 3 + j] * a[j];
            const double mk = e.M[i * 3 + j] * inv;
            m2 += mk * mk;
        }
    const double A = (sigma[0] + sigma[4] + sigma[8]) - asa;
    const double B = a[0] * (sigma[7] - sigma[5]) + a[1] * (sigma[2] - sigma[6]) + a[2] * (sigma[3] - sigma[1]);
    const double h2 = A * A + B * B;
    double c = 1.0, s = 0.0;
    // (h below 1e-12 of the moments sigma is formed from -- the level of their summation's rounding: the data do not
    //  determine the angle, e.g. every pair on a line parallel to a)
    if (h2 > 1e-24 * m2 && h2 > 0.0 && h2 < 1e300) {
        const double h = sqrt(h2);
        c = A / h;
        s = B / h;
    }
    double R[9];
    axis_rotation3(a, c, s, R);
    Mat4 T = Mat4::identity();
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T(i, j) = R[i * 3 + j];
        T(i, 3) = qm[i] - (R[i * 3] * pm[0] + R[i * 3 + 1] * pm[1] + R[i * 3 + 2] * pm[2]);
    }
    return T;
}

// Solve A x = b (4x4, partial pivoting, the steps of solve6); returns det(A).
VISMA_HD double solve4(const double A[16], const double b[4], double x[4])
{
    double M[4][5];
    for (int i = 0; i < 4; i++) {
        for (int j = 0; j < 4; j++) M[i][j] = A[i * 4 + j];
        M[i][4] = b[i];
    }
    double det = 1.0;
    for (int c = 0; c < 4; c++) {
        int piv = c;
        for (int r = c + 1; r < 4; r++)
            if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
        if (M[piv][c] == 0.0) {
            for (int i = 0; i < 4; i++) x[i] = 0.0;
            return 0.0;
        }
        if (piv != c) {
            for (int j = 0; j < 5; j++) { const double t = M[c][j]; M[c][j] = M[piv][j]; M[piv][j] = t; }
            det = -det;
        }
        det *= M[c][c];
        for (int r = c + 1; r < 4; r++) {
            const double f = M[r][c] / M[c][c];
            for (int j = c; j < 5; j++) M[r][j] -= f * M[c][j];
        }
    }
    for (int r = 3; r >= 0; r--) {
        double s = M[r][4];
        for (int j = r + 1; j < 4; j++) s -= M[r][j] * x[j];
        x[r] = s / M[r][r];
    }
    return det;
}

// Point-to-plane: one Gauss-Newton step on (angle about a, translation).  The 6-DoF Jacobian row [p x n, n] restricted
// by P = [[a, 0], [0, I3]] (6x4): H = P^T (J^T J) P, g = P^T (J^T r), H y = -g; the |det| < 1e-6 guard of gn_from_stats
// (Eigen.cpp:35-56) on the 4x4 system.  The update is the exact rotation by y0 about a (the Euler map of y0 a is a
// rotation about a only for a coordinate axis) and the translation y1..3.
VISMA_HD Mat4 gn_axis_from_stats(const double *st, const double a[3], bool *ok)
{
    const NormalEq e = unpack_stats(st);
    *ok = false;
    if (!(e.K > 0.0)) return Mat4::identity();
    double H[16], g[4], y[4];
    double Ja[6];                                       // (J^T J) column block times a: rows 0..5
    for (int i = 0; i < 6; i++) Ja[i] = e.JTJ[i * 6] * a[0] + e.JTJ[i * 6 + 1] * a[1] + e.JTJ[i * 6 + 2] * a[2];
    H[0] = a[0] * Ja[0] + a[1] * Ja[1] + a[2] * Ja[2];
    for (int j = 0; j < 3; j++) {
        H[1 + j] = Ja[3 + j];
        H[(1 + j) * 4] = Ja[3 + j];
        for (int k = 0; k < 3; k++) H[(1 + j) * 4 + 1 + k] = e.JTJ[(3 + j) * 6 + 3 + k];
    }
    g[0] = -(a[0] * e.JTr[0] + a[1] * e.JTr[1] + a[2] * e.JTr[2]);
    for (int j = 0; j < 3; j++) g[1 + j] = -e.JTr[3 + j];
    const double det = solve4(H, g, y);
    if (fabs(det) < 1e-6 || isnan(det) || isinf(det)) return Mat4::identity();
    *ok = true;
    double R[9];
    axis_rotation3(a, cos(y[0]), sin(y[0]), R);
    Mat4 T = Mat4::identity();
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T(i, j) = R[i * 3 + j];
        T(i, 3) = y[1 + i];
    }
    return T;
}

// The unit axis of a caller's vector: false for a zero, near-zero or non-finite one
inline bool normalise_axis(const double in[3], double out[3])
{
    const double n2 = in[0] * in[0] + in[1] * in[1] + in[2] * in[2];
    if (!(n2 > 1e-24) || !(n2 < 1e300)) return false;
    const double n = sqrt(n2);
    for (int i = 0; i < 3; i++) out[i] = in[i] / n;
    return true;
}

// ---- fast global registration (Zhou, Park, Koltun, ECCV 2016; O3D/Core/Registration/FastGlobalRegistration.cpp) -----------
// Host only: everything after the feature matching works on a few thousand correspondences.  DESIGN.md 4.4c7.

struct FgrOption {                                     // FastGlobalRegistration.h:44-50
    double division_factor = 1.4, max_corr_dist = 0.025, tuple_scale = 0.95;
    int use_absolute_scale = 0, decrease_mu = 1, iteration_number = 64, maximum_tuple_count = 1000;
};

// Philox4x32-10 (Salmon et al., SC'11), the generator of mesh.hip's sampling kernel, on the host (and in ransac.hip)
VISMA_HD void philox4x32_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

VISMA_HD double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// NormalizePointCloud (:189-240) on copies: cloud k minus its mean, both divided by scale_global
struct FgrNormalized {
    std::vector<double> xyz[2];
    double mean[2][3];
    double scale_global, scale_start;
};

inline FgrNormalized fgr_normalize(const double *c0, int64_t n0, const double *c1, int64_t n1, bool use_absolute_scale)
{
    FgrNormalized N;
    const double *in[2] = {c0, c1};
    const int64_t cnt[2] = {n0, n1};
    double scale = 0.0;
    for (int k = 0; k < 2; k++) {
        double m[3] = {0.0, 0.0, 0.0}, max_scale = 0.0;
        for (int64_t i = 0; i < cnt[k]; i++)
            for (int a = 0; a < 3; a++) m[a] = m[a] + in[k][3 * i + a];
        for (int a = 0; a < 3; a++) N.mean[k][a] = m[a] = m[a] / (double)(int)cnt[k];
        N.xyz[k].resize((size_t)(3 * cnt[k]));
        for (int64_t i = 0; i < cnt[k]; i++) {
            double *p = &N.xyz[k][(size_t)(3 * i)];
            for (int a = 0; a < 3; a++) p[a] = in[k][3 * i + a] - m[a];
            const double len = norm3(p[0], p[1], p[2]);
            if (len > max_scale) max_scale = len;
        }
        if (max_scale > scale) scale = max_scale;
    }
    N.scale_global = use_absolute_scale ? 1.0 : scale;
    N.scale_start = use_absolute_scale ? scale : 1.0;
    for (int k = 0; k < 2; k++)
        for (double &v : N.xyz[k]) v /= N.scale_global;
    return N;
}

// STEP 2 of AdvancedMatching (:98-123) from both full nearest-neighbour maps: (i, j) with nn_i_of_j[j] == i and
// nn_j_of_i[i] == j, ascending i.  (The reference asks for nn_j_of_i only where some j hits i; a kept pair's i is hit by its
// own j, so the full map gives the same list.)
inline void fgr_cross_check(const int32_t *nn_i_of_j, int64_t nj, const int32_t *nn_j_of_i, int64_t ni, std::vector<int32_t> &ci,
                            std::vector<int32_t> &cj)
{
    ci.clear(); cj.clear();
    for (int64_t i = 0; i < ni; i++) {
        const int32_t j = nn_j_of_i[i];
        if (j < 0 || j >= nj || nn_i_of_j[j] != (int32_t)i) continue;
        ci.push_back((int32_t)i);
        cj.push_back(j);
    }
}

// STEP 3 (:126-174): trial t draws three indices into the cross-checked list -- from `triples` (3 per trial, taken modulo
// ncorr) or words 0..2 of Philox4x32-10 at counter (t, 0), key `seed`, modulo ncorr --; all three edge ratios strictly
// inside (scale, 1 / scale) pushes the three pairs.  Returns the trials drawn.
inline int64_t fgr_tuple_test(const double *pi, const double *pj, const std::vector<int32_t> &ci, const std::vector<int32_t> &cj,
                              double scale, int maximum_tuple_count, uint64_t seed, const int32_t *triples, int64_t n_triples,
                              std::vector<int32_t> &oi, std::vector<int32_t> &oj)
{
    oi.clear(); oj.clear();
    const int64_t ncorr = (int64_t)ci.size();
    int64_t trials = ncorr * 100;
    if (triples) trials = n_triples < trials ? n_triples : trials;
    int64_t cnt = 0, t = 0;
    for (; t < trials; t++) {
        int64_t r[3];
        if (triples) {
            for (int k = 0; k < 3; k++) r[k] = (((int64_t)triples[3 * t + k] % ncorr) + ncorr) % ncorr;
        } else {
            uint32_t w[4];
            philox4x32_host((uint32_t)t, (uint32_t)((uint64_t)t >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
            for (int k = 0; k < 3; k++) r[k] = (int64_t)(w[k] % (uint64_t)ncorr);
        }
        double li[3], lj[3];
        for (int k = 0; k < 3; k++) {
            const double *a = pi + 3 * (int64_t)ci[(size_t)r[k]], *b = pi + 3 * (int64_t)ci[(size_t)r[(k + 1) % 3]];
            li[k] = norm3(a[0] - b[0], a[1] - b[1], a[2] - b[2]);
            const double *c = pj + 3 * (int64_t)cj[(size_t)r[k]], *d = pj + 3 * (int64_t)cj[(size_t)r[(k + 1) % 3]];
            lj[k] = norm3(c[0] - d[0], c[1] - d[1], c[2] - d[2]);
        }
        if ((li[0] * scale < lj[0]) && (lj[0] < li[0] / scale) && (li[1] * scale < lj[1]) && (lj[1] < li[1] / scale) &&
            (li[2] * scale < lj[2]) && (lj[2] < li[2] / scale)) {
            for (int k = 0; k < 3; k++) { oi.push_back(ci[(size_t)r[k]]); oj.push_back(cj[(size_t)r[k]]); }
            cnt++;
        }
        if (cnt >= maximum_tuple_count) { t++; break; }
    }
    return t;
}

// OptimizePairwiseRegistration (:242-325): the graduated Geman-McClure Gauss-Newton loop over pairs (i0[c], i1[c]) of the
// clouds p0, p1; returns trans with trans * p1 ~ p0.  Fewer than 10 pairs: the identity.
inline Mat4 fgr_optimize(const double *p0, const double *p1, const int32_t *i0, const int32_t *i1, int64_t K, const FgrOption &o,
                         double par)
{
    Mat4 trans = Mat4::identity();
    if (K < 10) return trans;
    std::vector<double> q((size_t)(3 * K));                   // the moved copies of p1's points, per pair
    for (int64_t c = 0; c < K; c++)
        for (int a = 0; a < 3; a++) q[(size_t)(3 * c + a)] = p1[3 * (int64_t)i1[c] + a];
    for (int itr = 0; itr < o.iteration_number; itr++) {
        double JTJ[36], JTr[6];
        for (double &v : JTJ) v = 0.0;
        for (double &v : JTr) v = 0.0;
        for (int64_t c = 0; c < K; c++) {
            const double *p = p0 + 3 * (int64_t)i0[c], *qq = &q[(size_t)(3 * c)];
            const double rpq[3] = {p[0] - qq[0], p[1] - qq[1], p[2] - qq[2]};
            const double temp = par / ((rpq[0] * rpq[0] + rpq[1] * rpq[1] + rpq[2] * rpq[2]) + par);
            const double s = temp * temp;
            // the three rows (:282-307): J and its three non-zero entries
            const int idx[3][3] = {{1, 2, 3}, {2, 0, 4}, {0, 1, 5}};
            const double val[3][3] = {{-qq[2], qq[1], -1.0}, {-qq[0], qq[2], -1.0}, {-qq[1], qq[0], -1.0}};
            for (int row = 0; row < 3; row++) {
                const double r = rpq[row];
                for (int a = 0; a < 3; a++) {
                    for (int b = 0; b < 3; b++) JTJ[idx[row][a] * 6 + idx[row][b]] += val[row][a] * val[row][b] * s;
                    JTr[idx[row][a]] += val[row][a] * r * s;
                }
            }
        }
        // SolveLinearSystem(-JTJ, JTr) (Eigen.cpp:35-56): zeros where the determinant guard rejects
        double A[36], x[6];
        for (int k = 0; k < 36; k++) A[k] = -JTJ[k];
        const double det = solve6(A, JTr, x);
        if (fabs(det) < 1e-6 || isnan(det) || isinf(det))
            for (double &v : x) v = 0.0;
        const Mat4 delta = euler_zyx_to_mat4(x);
        trans = delta * trans;
        for (int64_t c = 0; c < K; c++) {                      // PointCloud::Transform(delta)
            double *qq = &q[(size_t)(3 * c)];
            double n[3];
            for (int a = 0; a < 3; a++) n[a] = delta(a, 0) * qq[0] + delta(a, 1) * qq[1] + delta(a, 2) * qq[2] + delta(a, 3) * 1.0;
            qq[0] = n[0]; qq[1] = n[1]; qq[2] = n[2];
        }
        if (o.decrease_mu && itr % 4 == 0 && par > o.max_corr_dist) par /= o.division_factor;
    }
    return trans;
}

// GetTransformationOriginalScale(...).inverse() (:329-342, :373-374): source to target in the callers' frame
inline Mat4 fgr_map_back(const Mat4 &t, const FgrNormalized &N)
{
    double R[9], tt[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i * 3 + j] = t(i, j);
        tt[i] = (-t(i, 0) * N.mean[1][0] + -t(i, 1) * N.mean[1][1] + -t(i, 2) * N.mean[1][2]) + t(i, 3) * N.scale_global + N.mean[0][i];
    }
    // the inverse of [R tt; 0 1] for a general R: adjugate over determinant
    const double det = det3(R);
    double Ri[9];
    Ri[0] = (R[4] * R[8] - R[5] * R[7]) / det; Ri[1] = (R[2] * R[7] - R[1] * R[8]) / det; Ri[2] = (R[1] * R[5] - R[2] * R[4]) / det;
    Ri[3] = (R[5] * R[6] - R[3] * R[8]) / det; Ri[4] = (R[0] * R[8] - R[2] * R[6]) / det; Ri[5] = (R[2] * R[3] - R[0] * R[5]) / det;
    Ri[6] = (R[3] * R[7] - R[4] * R[6]) / det; Ri[7] = (R[1] * R[6] - R[0] * R[7]) / det; Ri[8] = (R[0] * R[4] - R[1] * R[3]) / det;
    Mat4 out = Mat4::identity();
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out(i, j) = Ri[i * 3 + j];
        out(i, 3) = -(Ri[i * 3] * tt[0] + Ri[i * 3 + 1] * tt[1] + Ri[i * 3 + 2] * tt[2]);
    }
    return out;
}

}  // namespace visma
