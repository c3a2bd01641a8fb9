"""The arithmetic of the NON-RIGID color map optimization (Open3D's ImageWarpingField, the warped QueryImageIntensity,
SetProxyIntensityForVertex and SetGeometryColorAverage, OptimizeImageCoorNonrigid: Core/ColorMap/ColorMapOptimization.cpp),
restated in numpy on top of tests/colormap_spec.py: the yardstick of the GPU tests.  tests/golden/colormap_warp.npz pins it to
the compiled reference (tests/golden/gen_colormap_warp.py).

  field       anchor_h = number_of_vertical_anchors, step = float(h) / (anchor_h - 1), anchor_w = int(ceil(float(w) / step) + 1);
              flow[(i + j anchor_w) 2 + {0, 1}] = {i step, j step}: the initial value and the regulariser's anchor
  cell        i = (int)(u / step) (toward zero), j likewise, p = (u - i step) / step, q likewise
  shift       ((1-p)(1-q)) g00 + ((1-p) q) g01 + (p (1-q)) g10 + (p q) g11: each scalar weight first, the four terms left to right
  proxy, colours   colormap_spec's walk; behind the margin test on the float (u, v) the shift of them, the margin test on
              it, the pixel int(round(shift))
  iteration   per camera over its visible list: G, u, v in f64 as the rigid terms(); cell, p, q, (uu, vv) the shift;
              TestImageBoundary(uu, vv, 10); gray, dx, dy = FloatValueAt(uu, vv); dfdx = ((g10 - g00)(1-q) + (g11 - g01) q) / step,
              dfdy = ((g01 - g00)(1-p) + (g11 - g10) p) / step; dIdx = dIdf . dfdx, dIdy = dIdf . dfdy; C[0..5] the rigid ones,
              C[6..13] = dIdf{0,1} * {(1-p)(1-q), (1-p) q, p (1-q), p q} (dIdf * (1-p) first); r = proxy - gray.  The 121 terms of
              a visit: the 105 upper entries of C C^T row by row, -r C, r r, 1 -- summed PER CELL (cell ii + jj (anchor_w - 1)).
              weight = option weight * count / n_vertex; per flow entry JJ(d, d) += weight^2, Jb(d) += weight (weight (flow -
              flow_init)), rr_reg += (weight (flow - flow_init))^2; x = -JJ^-1 Jb; the pose update of colormap_spec, flow += x[6:];
              after all cameras the proxies anew.

Deviations from the reference (visma_icp.h states the same):
  1. a visit whose cell is outside [0, anchor_w - 2] x [0, anchor_h - 2], or whose u / step or v / step is not finite or
     reaches 2^30 in magnitude, is skipped (the reference indexes JJ out of bounds there: undefined).  u in (-step, 0)
     truncates to cell 0 with p < 0: in range, kept.
  2. a camera keeps its pose and its flow, and reports its count, with fewer than 6 accepted visits, with a system that is not
     positive definite, or with a step that is not finite (the reference continues only at count == 0).
  3. the order is defined: cell by cell, within a cell in ascending vertex id.

`how`: "sequential" (cumsum, the library's order within a cell) or "pairwise" (numpy's).  `solve`: "dense" (numpy on the
assembled (6 + 2A)^2 matrix) or a callable (aw, ah, rows, n_vertex, weight, flow, flow_init) -> (x, rr_reg, kept), e.g. the
library's banded solve.  `trace` receives every decision."""
import numpy as np

import colormap_spec as S

ROW = 121
PAIRS = [(x, y) for x in range(14) for y in range(x, 14)] + [(14, x) for x in range(14)] + [(14, 14), (15, 15)]
BIG = 2.0 ** 30


def anchor_shape(w, h, anchors):
    """-> anchor_w, anchor_h, anchor_step"""
    step = float(h) / (anchors - 1)
    return int(np.ceil(float(w) / step) + 1), int(anchors), step


def initial_flow(aw, ah, step):
    f = np.zeros(aw * ah * 2)
    for j in range(ah):
        for i in range(aw):
            f[(i + j * aw) * 2], f[(i + j * aw) * 2 + 1] = i * step, j * step
    return f


def cell_of(u, v, step):
    """-> ii, jj (int64; 0 where not representable), representable (deviation 1's first half)"""
    with np.errstate(all="ignore"):
        du, dv = u / step, v / step
        ok = np.isfinite(du) & np.isfinite(dv) & (np.abs(du) < BIG) & (np.abs(dv) < BIG)
    ii, jj = np.trunc(np.where(ok, du, 0)).astype(np.int64), np.trunc(np.where(ok, dv, 0)).astype(np.int64)
    return ii, jj, ok


def corners(flow, aw, ii, jj):
    """-> g00, g01, g10, g11, each n x 2: QueryFlow(ii, jj), (ii, jj + 1), (ii + 1, jj), (ii + 1, jj + 1)"""
    f = flow.reshape(-1, 2)
    return f[ii + jj * aw], f[ii + (jj + 1) * aw], f[ii + 1 + jj * aw], f[ii + 1 + (jj + 1) * aw]


def shift(g, p, q):
    g00, g01, g10, g11 = g
    w00, w01, w10, w11 = (1 - p) * (1 - q), (1 - p) * q, p * (1 - q), p * q
    return tuple(((w00 * g00[:, k] + w01 * g01[:, k]) + w10 * g10[:, k]) + w11 * g11[:, k] for k in range(2))


def per_vertex(V, vis, E, K, flows, aw, ah, step, images, channels, trace=None):
    """colormap_spec.per_vertex with the warped pixel"""
    n, h, w = len(images), images[0].shape[0], images[0].shape[1]
    tot, cnt = np.zeros((len(V), channels)), np.zeros(len(V))
    for c in range(n):
        u, v, _ = S.project(E[c], K, V)
        ok = vis[c] & S.inside(u, v, w, h)
        ud, vd = np.where(ok, u, 10.0).astype(np.float64), np.where(ok, v, 10.0).astype(np.float64)
        ii, jj, _ = cell_of(ud, vd, step)
        assert ii.max() <= aw - 2 and jj.max() <= ah - 2 and ii.min() >= 0 and jj.min() >= 0      # inside the margin: always
        p, q = (ud - ii * step) / step, (vd - jj * step) / step
        su, sv = shift(corners(flows[c], aw, ii, jj), p, q)
        ok2 = ok & S.inside(su, sv, w, h)
        pu, pv = np.where(ok2, S.round_pixel(np.where(ok2, su, 0)), 0), np.where(ok2, S.round_pixel(np.where(ok2, sv, 0)), 0)
        val = images[c][pv, pu].reshape(len(V), channels).astype(np.float64)
        tot = np.where(ok2[:, None], tot + val, tot)
        cnt = cnt + ok2
        if trace is not None:
            trace.append(np.stack([ok, ok2, ii, jj, pu, pv]))
    return np.where(cnt[:, None] > 0, tot / np.maximum(cnt, 1)[:, None], 0.0)


def terms(V, visible, pose, K, flow, aw, ah, step, gray, dx, dy, proxy, trace=None, info=None):
    """camera: `visible` its ascending vertex list -> (cells, T): per accepted visit, in list order, its cell and its 121 terms"""
    fx, fy, cx, cy = (float(k) for k in K)
    h, w = gray.shape
    P = V[visible]
    G0, G1, G2 = S.transform(pose, P)
    with np.errstate(all="ignore"):
        u, v = (fx * G0 + cx * G2) / G2, (fy * G1 + cy * G2) / G2
    ii, jj, rep = cell_of(u, v, step)
    inr = rep & (ii >= 0) & (ii <= aw - 2) & (jj >= 0) & (jj <= ah - 2)
    ii, jj = np.where(inr, ii, 0), np.where(inr, jj, 0)
    with np.errstate(all="ignore"):
        p, q = (u - ii * step) / step, (v - jj * step) / step
        g = corners(flow, aw, ii, jj)
        uu, vv = shift(g, p, q)
    ok = inr & S.inside(uu, vv, w, h)
    if trace is not None:
        trace.append(np.stack([inr, ok, ii, jj]))
    if info is not None:
        info.append(dict(skipped=int((~inr).sum()), rejected=int((inr & ~ok).sum()), negative_p=int((ok & ((p < 0) | (q < 0))).sum())))
    G0, G1, G2, p, q, uu, vv, ii, jj = (a[ok] for a in (G0, G1, G2, p, q, uu, vv, ii, jj))
    g00, g01, g10, g11 = (a[ok] for a in g)
    gr, dfx, dfy = S.bilinear(gray, uu, vv), S.bilinear(dx, uu, vv), S.bilinear(dy, uu, vv)
    dfdx = [((g10[:, k] - g00[:, k]) * (1 - q) + (g11[:, k] - g01[:, k]) * q) / step for k in range(2)]
    dfdy = [((g01[:, k] - g00[:, k]) * (1 - p) + (g11[:, k] - g10[:, k]) * p) / step for k in range(2)]
    dIdx, dIdy = dfx * dfdx[0] + dfy * dfdx[1], dfx * dfdy[0] + dfy * dfdy[1]
    invz = 1.0 / G2
    v0 = dIdx * fx * invz; v1 = dIdy * fy * invz
    v2 = -(v0 * G0 + v1 * G1) * invz
    r = proxy[visible][ok] - gr
    R = [-G2 * v1 + G1 * v2, G2 * v0 - G0 * v2, -G1 * v0 + G0 * v1, v0, v1, v2,
         dfx * (1 - p) * (1 - q), dfy * (1 - p) * (1 - q), dfx * (1 - p) * q, dfy * (1 - p) * q,
         dfx * p * (1 - q), dfy * p * (1 - q), dfx * p * q, dfy * p * q, -r, np.ones_like(r)]
    T = np.stack([R[x] * R[y] for x, y in PAIRS], 1) if len(r) else np.zeros((0, ROW))
    return (ii + jj * (aw - 1)).astype(np.int64), T


def cell_rows(cells, T, n_cells, how="pairwise"):
    """-> (n_cells x 121 sums, n_cells x 121 of K 2^-53 sum|term|: colormap_spec.sum_bound per cell)"""
    rows, bound = np.zeros((n_cells, ROW)), np.zeros((n_cells, ROW))
    for c in np.unique(cells):
        t = T[cells == c]                                  # (the list ascends in vertex id: so does a cell's share of it)
        rows[c] = np.cumsum(t, axis=0)[-1] if how == "sequential" else t.sum(axis=0)
        bound[c] = S.sum_bound(t)
    return rows, bound


def unknowns(cell, aw):
    """the 14 unknowns of a cell's C: 6 of the pose, then (ii, jj), (ii, jj + 1), (ii + 1, jj), (ii + 1, jj + 1), x then y each"""
    ii, jj = cell % (aw - 1), cell // (aw - 1)
    a = [ii + jj * aw, ii + (jj + 1) * aw, ii + 1 + jj * aw, ii + 1 + (jj + 1) * aw]
    return list(range(6)) + [6 + 2 * k + d for k in a for d in (0, 1)]


def assemble(aw, ah, rows, n_vertex, weight_option, flow, flow_init):
    """-> JJ ((6 + 2A)^2, dense), Jb, rr, rr_reg, count: the reference's system of one camera from its cell rows"""
    n = 6 + 2 * aw * ah
    JJ, Jb = np.zeros((n, n)), np.zeros(n)
    for cell in range(len(rows)):
        if rows[cell, 120] == 0:
            continue
        idx = unknowns(cell, aw)
        for k, (x, y) in enumerate(PAIRS[:105]):
            JJ[idx[x], idx[y]] += rows[cell, k]
            if x != y:
                JJ[idx[y], idx[x]] += rows[cell, k]
        for x in range(14):
            Jb[idx[x]] += rows[cell, 105 + x]
    rr, count = rows[:, 119].sum(), rows[:, 120].sum()
    if count == 0:
        return JJ, Jb, rr, 0.0, 0
    weight = weight_option * count / n_vertex
    r = weight * (flow - flow_init)
    JJ[np.arange(6, n), np.arange(6, n)] += weight * weight
    Jb[6:] += weight * r
    return JJ, Jb, rr, float((r * r).sum()), int(count)


def solve_dense(aw, ah, rows, n_vertex, weight_option, flow, flow_init):
    """-> x, rr_reg, kept (deviation 2)"""
    JJ, Jb, _, reg, count = assemble(aw, ah, rows, n_vertex, weight_option, flow, flow_init)
    zero = np.zeros(len(Jb))
    if count < 6 or not np.all(np.isfinite(JJ)):
        return zero, reg, True
    try:
        np.linalg.cholesky(JJ)
        x = np.linalg.solve(JJ, -Jb)
    except np.linalg.LinAlgError:
        return zero, reg, True
    if not np.all(np.isfinite(x)):
        return zero, reg, True
    return x, reg, False


def pose_update(x):
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    A = np.eye(4); A[:3, :3] = Rz @ Ry @ Rx; A[:3, 3] = x[3:6]
    return A


class State(S.State):
    """colormap_spec.State with a warping field per image"""

    def __init__(self, V, depths, colors, E, K, option, trace=None):
        super().__init__(V, depths, colors, E, K, option, trace)
        h, w = self.gray[0].shape
        self.aw, self.ah, self.anchor_step = anchor_shape(w, h, option["number_of_vertical_anchors"])
        self.flow_init = initial_flow(self.aw, self.ah, self.anchor_step)
        self.flows = np.tile(self.flow_init, (len(self.E), 1))
        self.n_cells = (self.aw - 1) * (self.ah - 1)
        self.info = []

    def proxy(self):
        return per_vertex(self.V, self.vis, self.E, self.K, self.flows, self.aw, self.ah, self.anchor_step, [g[..., None] for g in self.gray], 1,
                          self.trace)[:, 0]

    def colours(self):
        return per_vertex(self.V, self.vis, self.E, self.K, self.flows, self.aw, self.ah, self.anchor_step,
                          [(c.astype(S.F32) / S.F32(255.0)).astype(S.F32) for c in self.colors], 3, self.trace)

    def terms(self, c, proxy):
        return terms(self.V, self.lists[c], self.E[c], self.K, self.flows[c], self.aw, self.ah, self.anchor_step, self.gray[c], self.dx[c],
                     self.dy[c], proxy, self.trace, self.info)

    def cell_sums(self, how="pairwise"):
        """-> rows, bounds: n x cells x 121 each"""
        p = self.proxy()
        out = [cell_rows(*self.terms(c, p), self.n_cells, how) for c in range(len(self.E))]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def step(self, how="pairwise", solve="dense", rows=None):
        """one iteration -> rr, rr_reg, count per camera (of the state before it); rows: this state's cell_sums(how)[0], if at hand"""
        if rows is None:
            rows, _ = self.cell_sums(how)
        fn = solve_dense if solve == "dense" else solve
        rr, reg, count = rows[:, :, 119].sum(axis=1), np.zeros(len(rows)), rows[:, :, 120].sum(axis=1).astype(np.int64)
        for c in range(len(rows)):
            x, reg[c], kept = fn(self.aw, self.ah, rows[c], len(self.V), self.option["non_rigid_anchor_point_weight"], self.flows[c],
                                 self.flow_init)
            if not kept:
                self.E[c] = pose_update(x) @ self.E[c]
                self.flows[c] = self.flows[c] + x[6:]
        return rr, reg, count

    def run(self, k, how="pairwise", solve="dense"):
        """-> rr and rr_reg (summed over the cameras) of every iteration: k x 2"""
        out = []
        for _ in range(k):
            rr, reg, _ = self.step(how, solve)
            out.append((rr.sum(), reg.sum()))
        return np.array(out).reshape(k, 2)
