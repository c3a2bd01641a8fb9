// colormap_solve.hpp -- the host half of the NON-RIGID color map optimization (colormap_warp.hip): one camera's
// system assembled from its cell rows, the regulariser, and the solve.  Host only, no device, no library: the sanitized
// driver tests/cpp/colormap_solve_driver.cpp includes it as it is.
//
//  unknowns   the reference's order: 6 of the pose, then 2 per anchor, anchor (i, j) at 6 + (i + j * anchor_w) * 2.
//  cell row   kCmWarpRow = 121 doubles of cell (ii, jj) (index ii + jj * (anchor_w - 1)): the 105 upper entries of C C^T row
//             by row (C[0..5] the pose's, C[6..13] the anchors (ii, jj), (ii, jj + 1), (ii + 1, jj), (ii + 1, jj + 1), x then
//             y each), the 14 of -r C, rr, count.
//  structure  a cell couples anchors at most anchor_w + 1 apart: the anchor block is banded with half-bandwidth
//             2 * anchor_w + 3, the pose a border of six.  The band is factored by Cholesky (L L^T, lower band kept row by
//             row); the border goes through its 6 x 6 Schur complement S = D - B^T A^-1 B with solve6.  No dense
//             (6 + 2 A)^2 matrix exists.
//  keep       a camera keeps its pose and its flow (x = 0, the function returns false) with fewer than 6 accepted visits,
//             with a pivot of the band, or a determinant of S, that is not positive and finite, or with a step that is not finite.
//  order      cells ascending, within a cell the row's entries ascending: nothing depends on a thread count
//             (cm_warp_solve_all gives every camera to exactly one thread).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "host_math.hpp"

namespace visma {

constexpr int kCmWarpRow = 121;                          // 105 + 14 + rr + count
constexpr int kCmWarpMaxAnchors = 8192;                  // anchor_w * anchor_h: a workgroup's histogram of cells fits LDS
constexpr int kCmWarpMaxThreads = 16;

// anchor_h = number_of_vertical_anchors, anchor_step = double(h) / (anchor_h - 1), anchor_w = int(ceil(double(w) / step) + 1)
inline void cm_warp_shape(int w, int h, int anchors, int *aw, int *ah, double *step)
{
    *ah = anchors;
    *step = (double)h / (double)(anchors - 1);
    const double c = std::ceil((double)w / *step) + 1.0;
    *aw = c < 1073741824.0 ? (int)c : 1073741824;
}

// the unknown (6 based) of C[6 + k] in cell (ii, jj)
inline int cm_warp_unknown(int k, int ii, int jj, int aw)
{
    const int corner = k >> 1;                           // 0: (ii, jj), 1: (ii, jj + 1), 2: (ii + 1, jj), 3: (ii + 1, jj + 1)
    return ((ii + (corner >> 1)) + (jj + (corner & 1)) * aw) * 2 + (k & 1);
}

// One camera.  cells: (aw - 1)(ah - 1) rows; flow, flow_init: 2 aw ah; x: 6 + 2 aw ah (zero where the camera keeps).
// *rr: the data residual, *rr_reg: the regulariser's (0 with no visit, as the reference's `continue`), *count: the visits.
// -> true: x is the step to apply.
inline bool cm_warp_solve_camera(int aw, int ah, const double *cells, double n_vertex, double weight_option, const double *flow,
                                 const double *flow_init, double *x, double *rr, double *rr_reg, int64_t *count)
{
    const int n = 2 * aw * ah, hb = std::min(2 * aw + 3, n - 1), ld = hb + 1;
    const int cw = aw - 1, n_cells = cw * (ah - 1);
    for (int k = 0; k < 6 + n; k++) x[k] = 0.0;
    std::vector<double> L((size_t)n * ld, 0.0);          // (i, i - d) at L[i * ld + d]
    std::vector<double> B((size_t)n * 6, 0.0), ba((size_t)n, 0.0);   // the border and the anchors' Jb
    double D[36], bp[6];
    for (double &v : D) v = 0.0;
    for (double &v : bp) v = 0.0;
    double srr = 0.0, cnt = 0.0;
    for (int cell = 0; cell < n_cells; cell++) {
        const double *row = cells + (size_t)cell * kCmWarpRow;
        if (row[120] == 0.0) continue;                   // no visit: the row is zero
        const int ii = cell % cw, jj = cell / cw;
        int idx[14];
        for (int k = 0; k < 6; k++) idx[k] = k;
        for (int k = 0; k < 8; k++) idx[6 + k] = 6 + cm_warp_unknown(k, ii, jj, aw);
        int k = 0;
        for (int a = 0; a < 14; a++)
            for (int b = a; b < 14; b++) {
                const double v = row[k++];
                const int ga = idx[a], gb = idx[b];
                if (gb < 6) {                            // (a <= b and idx ascends over the first six)
                    D[ga * 6 + gb] += v;
                    if (ga != gb) D[gb * 6 + ga] += v;
                } else if (ga < 6) {
                    B[(size_t)(gb - 6) * 6 + ga] += v;
                } else {
                    const int hi = std::max(ga, gb) - 6, lo = std::min(ga, gb) - 6;
                    L[(size_t)hi * ld + (hi - lo)] += v;
                }
            }
        for (int a = 0; a < 6; a++) bp[a] += row[105 + a];
        for (int a = 6; a < 14; a++) ba[(size_t)(idx[a] - 6)] += row[105 + a];
        srr += row[119];
        cnt += row[120];
    }
    *rr = srr;
    *rr_reg = 0.0;
    *count = 0;
    if (!(cnt >= 0.0) || !(cnt < 9007199254740992.0)) return false;      // (a count that is no count: a NaN row)
    *count = (int64_t)cnt;
    if (*count == 0) return false;
    const double weight = weight_option * cnt / n_vertex;
    double reg = 0.0;
    for (int d = 0; d < n; d++) {
        const double r = weight * (flow[d] - flow_init[d]);
        L[(size_t)d * ld] += weight * weight;
        ba[(size_t)d] += weight * r;
        reg += r * r;
    }
    *rr_reg = reg;
    if (*count < 6) return false;
    // the band's Cholesky factor, in place
    for (int j = 0; j < n; j++) {
        double *Lj = L.data() + (size_t)j * ld;
        double s = Lj[0];
        for (int k = std::max(0, j - hb); k < j; k++) s -= Lj[j - k] * Lj[j - k];
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        const double piv = std::sqrt(s);
        Lj[0] = piv;
        const int last = std::min(n - 1, j + hb);
        for (int i = j + 1; i <= last; i++) {
            double *Li = L.data() + (size_t)i * ld;
            double t = Li[i - j];
            for (int k = std::max(0, i - hb); k < j; k++) t -= Li[i - k] * Lj[j - k];
            Li[i - j] = t / piv;
        }
    }
    // Z = A^-1 (B | Jb_a): L w = (B | Jb_a), then L^T z = w, the seven columns side by side
    std::vector<double> Z((size_t)n * 7);
    for (int i = 0; i < n; i++) {
        for (int c = 0; c < 6; c++) Z[(size_t)i * 7 + c] = B[(size_t)i * 6 + c];
        Z[(size_t)i * 7 + 6] = ba[(size_t)i];
    }
    for (int i = 0; i < n; i++) {
        const double *Li = L.data() + (size_t)i * ld;
        double *zi = Z.data() + (size_t)i * 7;
        for (int k = std::max(0, i - hb); k < i; k++) {
            const double l = Li[i - k];
            const double *zk = Z.data() + (size_t)k * 7;
            for (int c = 0; c < 7; c++) zi[c] -= l * zk[c];
        }
        for (int c = 0; c < 7; c++) zi[c] /= Li[0];
    }
    for (int i = n - 1; i >= 0; i--) {
        double *zi = Z.data() + (size_t)i * 7;
        const int last = std::min(n - 1, i + hb);
        for (int k = i + 1; k <= last; k++) {
            const double l = L[(size_t)k * ld + (k - i)];
            const double *zk = Z.data() + (size_t)k * 7;
            for (int c = 0; c < 7; c++) zi[c] -= l * zk[c];
        }
        const double piv = L[(size_t)i * ld];
        for (int c = 0; c < 7; c++) zi[c] /= piv;
    }
    // JJ x = -Jb in blocks: D xp + B^T xa = -Jb_p, B xp + A xa = -Jb_a.  With y = Z's last column: xa = -y - Z xp and
    // (D - B^T Z) xp = -(Jb_p - B^T y).
    double S[36], rhs[6], xp[6];
    for (int a = 0; a < 6; a++) {
        for (int b = 0; b < 6; b++) {
            double s = D[a * 6 + b];
            for (int i = 0; i < n; i++) s -= B[(size_t)i * 6 + a] * Z[(size_t)i * 7 + b];
            S[a * 6 + b] = s;
        }
        double s = bp[a];
        for (int i = 0; i < n; i++) s -= B[(size_t)i * 6 + a] * Z[(size_t)i * 7 + 6];
        rhs[a] = -s;
    }
    const double det = solve6(S, rhs, xp);
    if (!(det > 0.0) || !std::isfinite(det)) return false;
    bool ok = true;
    for (int a = 0; a < 6; a++) ok = ok && std::isfinite(xp[a]);
    std::vector<double> xa((size_t)n);
    for (int i = 0; i < n && ok; i++) {
        double s = -Z[(size_t)i * 7 + 6];
        for (int a = 0; a < 6; a++) s -= Z[(size_t)i * 7 + a] * xp[a];
        xa[(size_t)i] = s;
        ok = std::isfinite(s);
    }
    if (!ok) return false;
    for (int a = 0; a < 6; a++) x[a] = xp[a];
    for (int i = 0; i < n; i++) x[6 + i] = xa[(size_t)i];
    return true;
}

// Every camera of a map, on up to `threads` host threads (camera c on thread c % threads): cells n_cameras x cells x 121,
// flows n_cameras x 2 aw ah, x n_cameras x (6 + 2 aw ah), rr / rr_reg / count / moved per camera.  Identical bits for every
// thread count: a camera's arithmetic never leaves its thread.
inline void cm_warp_solve_all(int n_cameras, int threads, int aw, int ah, const double *cells, double n_vertex, double weight_option,
                              const double *flows, const double *flow_init, double *x, double *rr, double *rr_reg, int64_t *count,
                              char *moved)
{
    const size_t n = (size_t)2 * aw * ah, per_cells = (size_t)(aw - 1) * (ah - 1) * kCmWarpRow;
    threads = std::max(1, std::min(std::min(threads, kCmWarpMaxThreads), n_cameras));
    auto work = [&](int t) {
        for (int c = t; c < n_cameras; c += threads)
            moved[c] = cm_warp_solve_camera(aw, ah, cells + per_cells * (size_t)c, n_vertex, weight_option, flows + n * (size_t)c, flow_init,
                                            x + (6 + n) * (size_t)c, rr + c, rr_reg + c, count + c)
                           ? 1 : 0;
    };
    if (threads == 1) { work(0); return; }
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; t++) pool.emplace_back(work, t);
    work(0);
    for (std::thread &t : pool) t.join();
}

}  // namespace visma
