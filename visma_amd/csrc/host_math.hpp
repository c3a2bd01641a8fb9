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

// ---- multiway registration (Choi, Zhou, Koltun, CVPR 2015; O3D/Core/Registration/GlobalOptimization.cpp) ------------------
// Host only: 6 unknowns per node, tens or hundreds of nodes.  DESIGN.md 4.4c9.

// The information matrix sum G^T G, G = [-hat(q) | I], from the ten sums of information.hip
// s = {K, sum x, y, z, sum xx, yy, zz, xy, xz, yz}; row-major 6 x 6.  (No identity terms: visma_icp.h.)
inline void information_from_sums(const double s[10], double out[36])
{
    for (int i = 0; i < 36; i++) out[i] = 0.0;
    const double K = s[0], X = s[1], Y = s[2], Z = s[3], xx = s[4], yy = s[5], zz = s[6], xy = s[7], xz = s[8], yz = s[9];
    out[0] = yy + zz; out[1] = -xy;     out[2] = -xz;
    out[6] = -xy;     out[7] = xx + zz; out[8] = -yz;
    out[12] = -xz;    out[13] = -yz;    out[14] = xx + yy;
    // the upper right block is sum hat(q)^T = -hat(sum q), the lower left its transpose
    out[4] = -Z; out[5] = Y; out[9] = Z; out[11] = -X; out[15] = -Y; out[16] = X;
    out[24] = -Z; out[30] = Y; out[19] = Z; out[31] = -X; out[20] = -Y; out[26] = X;
    out[21] = out[28] = out[35] = K;
}

// the inverse of a general 4 x 4 by cofactors (what Eigen's fixed-size inverse() evaluates)
inline Mat4 inverse4(const Mat4 &A)
{
    const double *m = A.m;
    double inv[16];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    Mat4 r;
    for (int i = 0; i < 16; i++) r.m[i] = inv[i] / det;
    return r;
}

// TransformMatrix4dToVector6d (Eigen.cpp:70-86)
inline void mat4_to_vec6(const Mat4 &T, double out[6])
{
    const double sy = sqrt(T(0, 0) * T(0, 0) + T(1, 0) * T(1, 0));
    if (!(sy < 1e-6)) {
        out[0] = atan2(T(2, 1), T(2, 2));
        out[1] = atan2(-T(2, 0), sy);
        out[2] = atan2(T(1, 0), T(0, 0));
    } else {
        out[0] = atan2(-T(1, 2), T(1, 1));
        out[1] = atan2(-T(2, 0), sy);
        out[2] = 0.0;
    }
    out[3] = T(0, 3); out[4] = T(1, 3); out[5] = T(2, 3);
}

struct PgEdge {                                        // PoseGraphEdge (PoseGraph.h:52-86)
    int source = -1, target = -1;
    Mat4 X = Mat4::identity();
    double info[36];
    int uncertain = 0;
    double confidence = 1.0;
};
struct PgOption {                                      // GlobalOptimizationOption, clamped as its constructor clamps
    double max_corr_dist = 0.075, edge_prune_threshold = 0.25, preference_loop_closure = 1.0;
    int reference_node = -1;
};
struct PgCriteria {                                    // GlobalOptimizationConvergenceCriteria, likewise
    int max_iteration = 100;
    double min_relative_increment = 1e-6, min_relative_residual_increment = 1e-6, min_right_term = 1e-6, min_residual = 1e-6;
    int max_iteration_lm = 20;
    double upper_scale_factor = 2.0 / 3.0, lower_scale_factor = 1.0 / 3.0;
};
struct PoseGraphData {
    std::vector<Mat4> nodes;
    std::vector<PgEdge> edges;
};

// GetLinearized6DVector (:71-79)
inline void pg_linearized6(const Mat4 &M, double o[6])
{
    o[0] = (-M(1, 2) + M(2, 1)) / 2.0;
    o[1] = (-M(2, 0) + M(0, 2)) / 2.0;
    o[2] = (-M(0, 1) + M(1, 0)) / 2.0;
    o[3] = M(0, 3); o[4] = M(1, 3); o[5] = M(2, 3);
}

// ValidatePoseGraph (:372-402)
inline bool pg_validate(const PoseGraphData &g)
{
    const int n_nodes = (int)g.nodes.size();
    for (int i = 0; i < n_nodes - 1; i++) {
        bool valid = false;
        for (const PgEdge &t : g.edges)
            if (t.source == i && t.target - t.source == 1) valid = true;
        if (!valid) return false;
    }
    for (const PgEdge &t : g.edges)
        if (!(t.source >= 0 && t.source < n_nodes && t.target >= 0 && t.target < n_nodes)) return false;
    return true;
}

// ComputeZeta (:161-172): 6 per edge, the linearised X^-1 Tt^-1 Ts
inline void pg_zeta(const PoseGraphData &g, std::vector<double> &zeta)
{
    zeta.assign(g.edges.size() * 6, 0.0);
    for (size_t e = 0; e < g.edges.size(); e++) {
        const PgEdge &t = g.edges[e];
        const Mat4 A = inverse4(t.X) * inverse4(g.nodes[(size_t)t.target]);
        pg_linearized6(A * g.nodes[(size_t)t.source], &zeta[e * 6]);
    }
}

// ComputeLinearSystem (:187-229): H (6n x 6n, row-major) and b (6n)
inline void pg_linear_system(const PoseGraphData &g, const std::vector<double> &zeta, std::vector<double> &H, std::vector<double> &b)
{
    const int n = (int)g.nodes.size() * 6;
    H.assign((size_t)n * n, 0.0);
    b.assign((size_t)n, 0.0);
    for (size_t ei = 0; ei < g.edges.size(); ei++) {
        const PgEdge &t = g.edges[ei];
        const double *e = &zeta[ei * 6];
        const Mat4 A = inverse4(t.X) * inverse4(g.nodes[(size_t)t.target]);
        const Mat4 &Ts = g.nodes[(size_t)t.source];
        // GetJacobian (:101-118): column i of Js is the linearised A Op_i Ts; Jt's the same with -Op_i, its exact negative
        double Js[36], Jt[36];
        static const int op_at[6][2] = {{6, 9}, {2, 8}, {1, 4}, {3, 3}, {7, 7}, {11, 11}};     // the entries -1 / +1 (or the 1)
        for (int i = 0; i < 6; i++) {
            Mat4 Op;
            for (double &v : Op.m) v = 0.0;
            if (i < 3) { Op.m[op_at[i][0]] = i == 1 ? 1.0 : -1.0; Op.m[op_at[i][1]] = i == 1 ? -1.0 : 1.0; }
            else Op.m[op_at[i][0]] = 1.0;
            double col[6];
            pg_linearized6((A * Op) * Ts, col);
            for (int r = 0; r < 6; r++) { Js[r * 6 + i] = col[r]; Jt[r * 6 + i] = -col[r]; }
        }
        double JsTI[36], JtTI[36], eTI[6];
        for (int r = 0; r < 6; r++) {
            for (int c = 0; c < 6; c++) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < 6; k++) { s1 += Js[k * 6 + r] * t.info[k * 6 + c]; s2 += Jt[k * 6 + r] * t.info[k * 6 + c]; }
                JsTI[r * 6 + c] = s1; JtTI[r * 6 + c] = s2;
            }
            double s = 0.0;
            for (int k = 0; k < 6; k++) s += e[k] * t.info[k * 6 + r];
            eTI[r] = s;
        }
        const double l = t.confidence;
        const int ii = t.source * 6, jj = t.target * 6;
        for (int r = 0; r < 6; r++) {
            for (int c = 0; c < 6; c++) {
                double ss = 0.0, st = 0.0, ts = 0.0, tt = 0.0;
                for (int k = 0; k < 6; k++) {
                    ss += l * JsTI[r * 6 + k] * Js[k * 6 + c]; st += l * JsTI[r * 6 + k] * Jt[k * 6 + c];
                    ts += l * JtTI[r * 6 + k] * Js[k * 6 + c]; tt += l * JtTI[r * 6 + k] * Jt[k * 6 + c];
                }
                H[(size_t)(ii + r) * n + ii + c] += ss; H[(size_t)(ii + r) * n + jj + c] += st;
                H[(size_t)(jj + r) * n + ii + c] += ts; H[(size_t)(jj + r) * n + jj + c] += tt;
            }
            double bs = 0.0, bt = 0.0;
            for (int k = 0; k < 6; k++) { bs += l * eTI[k] * Js[k * 6 + r]; bt += l * eTI[k] * Jt[k * 6 + r]; }
            b[(size_t)(ii + r)] -= bs; b[(size_t)(jj + r)] -= bt;
        }
    }
}

// A x = b by the dense L D L^T with diagonal pivoting that Eigen's LDLT<MatrixXd, Lower> runs (LDLT.h:291-400, :558-600): the
// largest remaining diagonal entry first, no cut-off on a pivot other than exactly zero (whose row of the solve gives 0).
// Gauss-Newton hands it the singular H of a graph without a fixed node, as the reference does.
inline void ldlt_solve(std::vector<double> A, int n, const double *b, double *x)
{
    std::vector<int> tr((size_t)n);
    std::vector<double> temp((size_t)n);
    auto a = [&](int i, int j) -> double & { return A[(size_t)i * n + j]; };
    for (int k = 0; k < n; k++) {
        int p = k;
        for (int i = k + 1; i < n; i++)
            if (fabs(a(i, i)) > fabs(a(p, p))) p = i;
        tr[(size_t)k] = p;
        if (p != k) {                                        // the transposition on the lower triangle
            for (int j = 0; j < k; j++) { const double v = a(k, j); a(k, j) = a(p, j); a(p, j) = v; }
            for (int i = p + 1; i < n; i++) { const double v = a(i, k); a(i, k) = a(i, p); a(i, p) = v; }
            { const double v = a(k, k); a(k, k) = a(p, p); a(p, p) = v; }
            for (int i = k + 1; i < p; i++) { const double v = a(i, k); a(i, k) = a(p, i); a(p, i) = v; }
        }
        if (k > 0) {
            for (int j = 0; j < k; j++) temp[(size_t)j] = a(j, j) * a(k, j);
            double s = 0.0;
            for (int j = 0; j < k; j++) s += a(k, j) * temp[(size_t)j];
            a(k, k) -= s;
            for (int i = k + 1; i < n; i++) {
                double u = 0.0;
                for (int j = 0; j < k; j++) u += a(i, j) * temp[(size_t)j];
                a(i, k) -= u;
            }
        }
        const double akk = a(k, k);
        const bool valid = fabs(akk) > 0.0;
        if (k == 0 && !valid) {                              // the whole diagonal is zero
            for (int j = 0; j < n; j++) tr[(size_t)j] = j;
            break;
        }
        if (valid)
            for (int i = k + 1; i < n; i++) a(i, k) /= akk;
    }
    for (int i = 0; i < n; i++) x[i] = b[i];
    for (int k = 0; k < n; k++) { const double v = x[k]; x[k] = x[tr[(size_t)k]]; x[tr[(size_t)k]] = v; }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++) x[i] -= a(i, j) * x[j];
    const double tol = 1.0 / 1.7976931348623157e308;
    for (int i = 0; i < n; i++) x[i] = fabs(a(i, i)) > tol ? x[i] / a(i, i) : 0.0;
    for (int i = n - 1; i >= 0; i--)
        for (int j = i + 1; j < n; j++) x[i] -= a(j, i) * x[j];
    for (int k = n - 1; k >= 0; k--) { const double v = x[k]; x[k] = x[tr[(size_t)k]]; x[tr[(size_t)k]] = v; }
}

// ComputeLineProcessWeight (:329-350): information(5, 5) read as the number of correspondences
inline double pg_line_process_weight(const PoseGraphData &g, const PgOption &o)
{
    if (g.edges.empty()) return 0.0;
    double avg = 0.0;
    for (const PgEdge &t : g.edges) avg += t.info[35];
    avg /= (double)(int)g.edges.size();
    return o.preference_loop_closure * pow(o.max_corr_dist, 2) * avg;
}

inline double pg_quadratic(const double *e, const double *info)
{
    double r = 0.0;
    for (int a = 0; a < 6; a++) {
        double s = 0.0;
        for (int c = 0; c < 6; c++) s += info[a * 6 + c] * e[c];
        r += e[a] * s;
    }
    return r;
}

// UpdateConfidence (:122-141)
inline int pg_update_confidence(PoseGraphData &g, const std::vector<double> &zeta, double w, const PgOption &o)
{
    int valid = 0;
    for (size_t e = 0; e < g.edges.size(); e++) {
        const double temp = w / (w + pg_quadratic(&zeta[e * 6], g.edges[e].info));
        g.edges[e].confidence = temp * temp;
        if (temp * temp > o.edge_prune_threshold) valid++;
    }
    return valid;
}

// ComputeResidual (:144-158)
inline double pg_residual(const PoseGraphData &g, const std::vector<double> &zeta, double w)
{
    double residual = 0.0;
    for (size_t e = 0; e < g.edges.size(); e++) {
        const double l = g.edges[e].confidence;
        residual += l * pg_quadratic(&zeta[e * 6], g.edges[e].info) + w * pow(sqrt(l) - 1, 2.0);
    }
    return residual;
}

inline void pg_pose_vector(const PoseGraphData &g, std::vector<double> &x)
{
    x.resize(g.nodes.size() * 6);
    for (size_t i = 0; i < g.nodes.size(); i++) mat4_to_vec6(g.nodes[i], &x[i * 6]);
}

inline PoseGraphData pg_updated(const PoseGraphData &g, const std::vector<double> &delta)
{
    PoseGraphData r = g;
    for (size_t i = 0; i < r.nodes.size(); i++) r.nodes[i] = euler_zyx_to_mat4(&delta[i * 6]) * r.nodes[i];
    return r;
}

inline double pg_norm(const std::vector<double> &v)
{
    double s = 0.0;
    for (double e : v) s += e * e;
    return sqrt(s);
}
inline double pg_max_coeff(const std::vector<double> &v)
{
    double m = v[0];
    for (double e : v) m = e > m ? e : m;
    return m;
}
inline bool pg_check_increment(const std::vector<double> &delta, const std::vector<double> &x, const PgCriteria &c)
{
    return pg_norm(delta) < c.min_relative_increment * (pg_norm(x) + c.min_relative_increment);
}

// GlobalOptimizationGaussNewton::OptimizePoseGraph (:432-514) and GlobalOptimizationLevenbergMarquardt's (:516-639): the
// reference's tests in the reference's order
inline void pg_optimize(PoseGraphData &g, int method, const PgCriteria &c, const PgOption &o)
{
    const int n = (int)g.nodes.size() * 6;
    if (n == 0) return;
    const double w = pg_line_process_weight(g, o);
    std::vector<double> zeta, zeta_new, H, b, x, delta((size_t)n), HL;
    pg_zeta(g, zeta);
    double current_residual = pg_residual(g, zeta, w), new_residual;
    pg_update_confidence(g, zeta, w, o);
    pg_pose_vector(g, x);
    pg_linear_system(g, zeta, H, b);
    auto right_term = [&]() { return pg_max_coeff(b) < c.min_right_term; };                   // maxCoeff, not its absolute value
    auto residual_increment = [&]() { return current_residual - new_residual < c.min_relative_residual_increment * current_residual; };
    auto accept = [&](PoseGraphData &next) {
        current_residual = new_residual;
        zeta = zeta_new;
        g = next;
        pg_pose_vector(g, x);
        pg_update_confidence(g, zeta, w, o);
        pg_linear_system(g, zeta, H, b);
    };
    bool stop = false;
    if (method == 0) {
        if (right_term()) return;
        for (int iter = 0; !stop; iter++) {
            ldlt_solve(H, n, b.data(), delta.data());
            stop = stop || pg_check_increment(delta, x, c);
            if (stop) break;
            PoseGraphData next = pg_updated(g, delta);
            pg_zeta(next, zeta_new);
            new_residual = pg_residual(g, zeta_new, w);
            stop = stop || residual_increment();
            if (stop) break;
            accept(next);
            stop = stop || right_term();
            if (stop) break;
            stop = stop || current_residual < c.min_residual || iter >= c.max_iteration;
        }
        return;
    }
    double hmax = H[0];
    for (int i = 1; i < n; i++) hmax = H[(size_t)i * n + i] > hmax ? H[(size_t)i * n + i] : hmax;
    const double tau = 1e-5;
    double current_lambda = tau * hmax, ni = 2.0, rho = 0.0;
    stop = stop || right_term();
    if (stop) return;
    for (int iter = 0; !stop; iter++) {
        int lm_count = 0;
        do {
            HL = H;
            for (int i = 0; i < n; i++) HL[(size_t)i * n + i] += current_lambda * 1.0;
            ldlt_solve(HL, n, b.data(), delta.data());           // (dense throughout: the reference's sparse Cholesky is an implementation detail)
            stop = stop || pg_check_increment(delta, x, c);
            if (!stop) {
                PoseGraphData next = pg_updated(g, delta);
                pg_zeta(next, zeta_new);
                new_residual = pg_residual(g, zeta_new, w);
                double dot = 0.0;
                for (int i = 0; i < n; i++) dot += delta[(size_t)i] * (current_lambda * delta[(size_t)i] + b[(size_t)i]);
                rho = (current_residual - new_residual) / (dot + 1e-3);
                if (rho > 0) {
                    stop = stop || residual_increment();
                    if (stop) break;
                    double alpha = 1. - pow((2 * rho - 1), 3);
                    alpha = alpha < c.upper_scale_factor ? alpha : c.upper_scale_factor;
                    const double scale = c.lower_scale_factor > alpha ? c.lower_scale_factor : alpha;
                    current_lambda *= scale;
                    ni = 2;
                    accept(next);
                    stop = stop || right_term();
                    if (stop) break;
                } else {
                    current_lambda *= ni;
                    ni *= 2;
                }
            }
            lm_count++;
            stop = stop || lm_count >= c.max_iteration_lm;
        } while (!((rho > 0) || stop));
        stop = stop || current_residual < c.min_residual || iter >= c.max_iteration;
    }
}

// GlobalOptimization (:641-662): validation, the first optimisation, CreatePoseGraphWithoutInvalidEdges (:406-430), the
// second optimisation, CompensateReferencePoseGraphNode (:352-370).  false: an invalid graph, returned untouched.
inline bool pg_global_optimization(PoseGraphData &g, int method, const PgCriteria &c, const PgOption &o)
{
    if (!pg_validate(g)) return false;
    PoseGraphData pre = g;
    pg_optimize(pre, method, c, o);
    PoseGraphData pruned;
    pruned.nodes = pre.nodes;
    for (const PgEdge &t : pre.edges)
        if (!t.uncertain || t.confidence > o.edge_prune_threshold) pruned.edges.push_back(t);
    pg_optimize(pruned, method, c, o);
    const int n_nodes = (int)pruned.nodes.size();
    if (o.reference_node >= 0 && o.reference_node < n_nodes) {
        const Mat4 comp = g.nodes[(size_t)o.reference_node] * inverse4(pruned.nodes[(size_t)o.reference_node]);
        for (Mat4 &p : pruned.nodes) p = comp * p;
    }
    g = pruned;
    return true;
}

}  // namespace visma
