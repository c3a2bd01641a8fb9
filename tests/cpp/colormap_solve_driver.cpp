// colormap_solve_driver.cpp -- the host half of the non-rigid color map optimization (visma_amd/csrc/colormap_solve.hpp: one
// camera's banded system assembled from its cell rows, the regulariser, the solve; every camera of a map on host threads) on
// the inputs a hostile caller or a hostile frame could produce.  Stand-alone, no GPU, no library: built with
// -fsanitize=address,undefined (tests/cpp/build_colormap_solve.py), so that an index past a band, a read past the rows or a
// signed overflow ends the run.  Every case must RETURN what is expected.  Prints one line per case and exits 0 only if
// all pass.
#include <climits>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "colormap_solve.hpp"

using namespace visma;

static int failures = 0;

static void expect(const char *name, bool ok)
{
    std::printf("%s: %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) failures++;
}

// a small generator of its own: the same numbers everywhere
static double rnd(unsigned *s)
{
    *s = *s * 1664525u + 1013904223u;
    return (double)(*s >> 8) / 16777216.0 - 0.5;
}

// n synthetic visits added to a cell's row
static void add_visits(double *row, int n, unsigned seed)
{
    for (int t = 0; t < n; t++) {
        double R[16];
        for (int k = 0; k < 15; k++) R[k] = rnd(&seed);
        R[15] = 1.0;
        int k = 0;
        for (int a = 0; a < 14; a++)
            for (int b = a; b < 14; b++) row[k++] += R[a] * R[b];
        for (int a = 0; a < 14; a++) row[k++] += R[14] * R[a];
        row[k++] += R[14] * R[14];
        row[k++] += 1.0;
    }
}

struct Case {
    int aw, ah;
    std::vector<double> cells, flow, flow_init, x;
    double rr, reg;
    int64_t count;
    Case(int aw_, int ah_) : aw(aw_), ah(ah_), cells((size_t)(aw_ - 1) * (ah_ - 1) * kCmWarpRow, 0.0), flow((size_t)aw_ * ah_ * 2, 0.0),
                             flow_init((size_t)aw_ * ah_ * 2, 0.0), x(6 + (size_t)aw_ * ah_ * 2, 7.0), rr(0), reg(0), count(0)
    {
        for (size_t d = 0; d < flow.size(); d++) { flow_init[d] = (double)(d % 17); flow[d] = flow_init[d] + 0.01 * (double)(d % 5); }
    }
    double *row(int cell) { return cells.data() + (size_t)cell * kCmWarpRow; }
    bool solve(double n_vertex, double weight) { return cm_warp_solve_camera(aw, ah, cells.data(), n_vertex, weight, flow.data(), flow_init.data(), x.data(), &rr, &reg, &count); }
    bool zero() const { for (double v : x) if (v != 0.0) return false; return true; }
    bool finite() const { for (double v : x) if (!std::isfinite(v)) return false; return true; }
};

// the residual of the assembled system at x, for a case small enough to assemble densely here
static double residual(Case &c, double n_vertex, double weight_option)
{
    const int n = 6 + 2 * c.aw * c.ah, cw = c.aw - 1;
    std::vector<double> JJ((size_t)n * n, 0.0), Jb((size_t)n, 0.0);
    double cnt = 0.0;
    for (int cell = 0; cell < cw * (c.ah - 1); cell++) {
        const double *row = c.row(cell);
        int idx[14];
        for (int k = 0; k < 6; k++) idx[k] = k;
        for (int k = 0; k < 8; k++) idx[6 + k] = 6 + cm_warp_unknown(k, cell % cw, cell / cw, c.aw);
        int k = 0;
        for (int a = 0; a < 14; a++)
            for (int b = a; b < 14; b++, k++) {
                JJ[(size_t)idx[a] * n + idx[b]] += row[k];
                if (a != b) JJ[(size_t)idx[b] * n + idx[a]] += row[k];
            }
        for (int a = 0; a < 14; a++) Jb[(size_t)idx[a]] += row[105 + a];
        cnt += row[120];
    }
    const double weight = weight_option * cnt / n_vertex;
    for (int d = 6; d < n; d++) {
        JJ[(size_t)d * n + d] += weight * weight;
        Jb[(size_t)d] += weight * (weight * (c.flow[(size_t)d - 6] - c.flow_init[(size_t)d - 6]));
    }
    double worst = 0.0;
    for (int a = 0; a < n; a++) {
        double s = Jb[(size_t)a];
        for (int b = 0; b < n; b++) s += JJ[(size_t)a * n + b] * c.x[(size_t)b];
        worst = std::max(worst, std::fabs(s));
    }
    return worst;
}

int main()
{
    {   // the smallest field: 2 x 2 anchors, one cell
        Case c(2, 2);
        add_visits(c.row(0), 50, 1u);
        const bool moved = c.solve(100.0, 0.316);
        expect("anchors 2 x 2: solved", moved && c.finite() && c.count == 50 && residual(c, 100.0, 0.316) < 1e-9);
    }
    {   // every cell visited, a field wider than high and one higher than wide
        Case c(5, 3), d(3, 6);
        for (int cell = 0; cell < 8; cell++) add_visits(c.row(cell), 9 + cell, 10u + (unsigned)cell);
        for (int cell = 0; cell < 10; cell++) add_visits(d.row(cell), 7 + cell, 30u + (unsigned)cell);
        expect("5 x 3: solved", c.solve(500.0, 0.5) && residual(c, 500.0, 0.5) < 1e-9);
        expect("3 x 6: solved", d.solve(500.0, 0.5) && residual(d, 500.0, 0.5) < 1e-9);
    }
    {   // the largest field there is: 64 vertical anchors, 128 x 64 = 8192 anchors; a few cells visited, most rows empty
        Case c(128, 64);
        const int cw = 127;
        const int cells[] = {0, 1, cw, 63 * cw - 1, 126, 40 * cw + 77};
        for (int cell : cells) add_visits(c.row(cell), 30, 100u + (unsigned)cell);
        const bool moved = c.solve(1000.0, 1.0);
        expect("128 x 64: solved", moved && c.finite() && c.count == 180 && c.reg > 0.0);
    }
    {   // empty rows alone: count 0, nothing moves, no regulariser residual
        Case c(4, 3);
        expect("no visit: keeps", !c.solve(100.0, 0.5) && c.zero() && c.count == 0 && c.reg == 0.0 && c.rr == 0.0);
    }
    {   // fewer than 6 visits: keeps and reports
        Case c(4, 3);
        add_visits(c.row(2), 5, 5u);
        expect("5 visits: keeps", !c.solve(100.0, 0.5) && c.zero() && c.count == 5 && c.reg > 0.0);
        add_visits(c.row(2), 1, 6u);
        expect("6 visits: solved", c.solve(100.0, 0.5) && c.count == 6);
    }
    {   // weight 0 with anchors nothing visits: a pivot that is zero
        Case c(4, 3);
        add_visits(c.row(0), 60, 7u);
        expect("weight 0, unvisited anchors: keeps", !c.solve(100.0, 0.0) && c.zero() && c.count == 60);
        expect("... with a weight: solved", c.solve(100.0, 0.25) && residual(c, 100.0, 0.25) < 1e-9);
    }
    {   // rows that are not numbers: a sum of the system, the count (rr alone is reported, the system does not read it); a negative count
        const double bad[] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
        bool ok = true;
        for (double b : bad)
            for (int at : {0, 50, 104, 105, 118, 120}) {
                Case c(4, 3);
                add_visits(c.row(1), 40, 8u);
                add_visits(c.row(4), 40, 9u);
                c.row(4)[at] = b;
                ok = ok && !c.solve(100.0, 0.5) && c.zero();
            }
        expect("NaN and inf rows: keep", ok);
        Case c(4, 3);
        add_visits(c.row(1), 40, 8u);
        c.row(1)[120] = -3.0;
        expect("a negative count: keeps", !c.solve(100.0, 0.5) && c.zero() && c.count == 0);
    }
    {   // a count of INT_MAX: the weight is a double, nothing overflows
        Case c(4, 3);
        add_visits(c.row(3), 40, 11u);
        c.row(3)[120] = (double)INT_MAX;
        const bool moved = c.solve(1.0, 0.316);
        expect("count INT_MAX: returns", c.count == (int64_t)INT_MAX && c.finite() && (moved || c.zero()));
        c.row(3)[120] = 9.1e15;
        expect("a count beyond 2^53: keeps", !c.solve(1.0, 0.316) && c.zero() && c.count == 0);
    }
    {   // many cameras: 1 and 16 threads, and more threads than cameras, give the same bits
        const int aw = 6, ah = 4, n = 23;
        const size_t per = (size_t)(aw - 1) * (ah - 1) * kCmWarpRow, A2 = (size_t)aw * ah * 2;
        std::vector<double> cells(per * n, 0.0), flows(A2 * n), init(A2);
        for (size_t d = 0; d < A2; d++) init[d] = (double)(d % 11);
        for (int c = 0; c < n; c++) {
            for (size_t d = 0; d < A2; d++) flows[(size_t)c * A2 + d] = init[d] + 0.02 * (double)((d + (size_t)c) % 7);
            if (c % 5 == 4) continue;                                        // (cameras without a visit among them)
            for (int cell = 0; cell < 15; cell += 1 + c % 3) add_visits(cells.data() + (size_t)c * per + (size_t)cell * kCmWarpRow, 8 + c, 200u + (unsigned)(c * 16 + cell));
        }
        std::vector<double> x[3], rr[3], reg[3];
        std::vector<int64_t> count[3];
        std::vector<char> moved[3];
        const int threads[3] = {1, 16, 64};
        for (int t = 0; t < 3; t++) {
            x[t].assign((6 + A2) * n, -1.0); rr[t].assign(n, -1.0); reg[t].assign(n, -1.0); count[t].assign(n, -1); moved[t].assign(n, 2);
            cm_warp_solve_all(n, threads[t], aw, ah, cells.data(), 300.0, 0.316, flows.data(), init.data(), x[t].data(), rr[t].data(), reg[t].data(),
                              count[t].data(), moved[t].data());
        }
        bool same = true;
        int movers = 0;
        for (int t = 1; t < 3; t++)
            same = same && !std::memcmp(x[0].data(), x[t].data(), sizeof(double) * x[0].size()) && !std::memcmp(rr[0].data(), rr[t].data(), sizeof(double) * n) &&
                   !std::memcmp(reg[0].data(), reg[t].data(), sizeof(double) * n) && count[0] == count[t] && moved[0] == moved[t];
        for (int c = 0; c < n; c++) movers += moved[0][(size_t)c];
        expect("1, 16 and 64 threads: identical bits", same && movers >= 15 && movers < n);
    }
    {   // the shape
        int aw, ah; double step;
        cm_warp_shape(83, 61, 5, &aw, &ah, &step);
        bool ok = aw == 7 && ah == 5 && step == 15.25;
        cm_warp_shape(640, 480, 16, &aw, &ah, &step);
        ok = ok && aw == 21 && ah == 16 && step == 32.0;
        cm_warp_shape(21, 21, 2, &aw, &ah, &step);
        ok = ok && aw == 2 && ah == 2;
        cm_warp_shape(67108864, 21, 64, &aw, &ah, &step);                   // (what create refuses: no overflow on the way there)
        ok = ok && aw > kCmWarpMaxAnchors;
        expect("anchor shapes", ok);
    }
    std::printf("%s\n", failures ? "FAILED" : "all passed");
    return failures ? 1 : 0;
}
