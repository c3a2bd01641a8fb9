"""The arithmetic of color map optimization (Open3D's ColorMapOptimization, rigid variant:
Core/ColorMap/ColorMapOptimization.cpp), restated in numpy: the yardstick of the GPU tests.  tests/golden/colormap.npz pins it
to the compiled reference (tests/golden/gen_colormap.py).

  images      gray = Gaussian3((0.2990f R + 0.5870f G + 0.1140f B) / 255.0f), dx = Sobel3Dx(gray), dy = Sobel3Dy(gray): the
              filters of tests/odometry_spec.py (fp32 products, f64 sums in tap order, one cast)
  mask        255 where sqrt(dx^2 + dy^2) of the depth's Sobel images, in f64, exceeds the threshold; then a square maximum
  project     Vt = E (X, Y, Z, 1) in f64, every row ((e0 X + e1 Y) + e2 Z) + e3; u = float(Vt0 fx / Vt2 + cx), v likewise,
              z = float(Vt2)
  visible     z >= 0, the rounded pixel inside, depth there <= maximum_allowable_depth, mask there != 255,
              fabsf(z - depth) < depth_threshold_for_visiblity_check; a projection that is not finite is not visible.
              Computed once.  A camera's list ascends in vertex id, a vertex's cameras ascend in camera id.
  proxy       over the vertex's cameras: the margin test (10 pixels) on the float u, v; gray at the rounded pixel added to a
              double; the mean, 0.0 without a camera
  iteration   terms(): per visible vertex inside the margin the 29 terms of the camera's sums (21 upper entries of C C^T row
              by row, -r C, r^2, 1); x = -JJ^-1 Jb; pose <- [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5] pose; after all cameras the
              proxies anew.  A camera with fewer than 6 terms or a singular JJ keeps its pose (the reference turns it into NaN).
  colours     as the proxy, (float(R) / 255.0f, ...) added as doubles

`how` names the order of a camera's sums: "sequential" (the reference's) or "pairwise" (numpy's): the fixture records how
far apart the two end.  `trace`, a list, receives every decision (visibility, margin tests, rounded pixels) so that the
generator can check that they are stable."""
import numpy as np

import odometry_spec as O

F32 = np.float32
U = 2.0 ** -53
MARGIN = 10.0
N_SUMS = 29


def default_option():
    return dict(non_rigid_camera_coordinate=False, number_of_vertical_anchors=16, non_rigid_anchor_point_weight=0.316,
                maximum_iteration=300.0, maximum_allowable_depth=2.5, depth_threshold_for_visiblity_check=0.03,
                depth_threshold_for_discontinuity_check=0.1, half_dilation_kernel_size_for_discontinuity_map=3)


# ---- images -----------------------------------------------------------------------------------------------------------------
def gray_of_rgb(rgb):
    r, g, b = (rgb[..., k].astype(F32) for k in range(3))
    return ((F32(0.2990) * r + F32(0.5870) * g + F32(0.1140) * b) / F32(255.0)).astype(F32)


def gradient_images(rgb):
    """-> gray, dx, dy (h x w fp32)"""
    gray = O.gaussian3(gray_of_rgb(rgb))
    return gray, O.sobel_dx(gray), O.sobel_dy(gray)


def dilate(mask, k):
    """a square maximum of half-size k; neighbours outside the image are ignored"""
    h, w = mask.shape
    out = mask.copy()
    for axis, n in ((1, w), (0, h)):
        src = out.copy()
        for s in range(1, k + 1):
            if s >= n:
                break
            a = [slice(None), slice(None)]; b = [slice(None), slice(None)]
            a[axis], b[axis] = slice(s, None), slice(None, n - s)
            out[tuple(b)] = np.maximum(out[tuple(b)], src[tuple(a)])
            out[tuple(a)] = np.maximum(out[tuple(a)], src[tuple(b)])
    return out


def depth_mask(depth, threshold, k):
    depth = np.ascontiguousarray(depth, F32)
    dx, dy = O.sobel_dx(depth).astype(np.float64), O.sobel_dy(depth).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mag = np.sqrt(dx * dx + dy * dy)
        raw = np.where(mag > threshold, 255, 0).astype(np.uint8)
    return dilate(raw, int(k))


# ---- projection ---------------------------------------------------------------------------------------------------------------
def transform(E, V):
    """rows ((e0 X + e1 Y) + e2 Z) + e3 -> three f64 arrays"""
    X, Y, Z = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(invalid="ignore"):                                # (a vertex that is not finite)
        return tuple(((E[r, 0] * X + E[r, 1] * Y) + E[r, 2] * Z) + E[r, 3] for r in range(3))


def project(E, K, V):
    """Project3DPointAndGetUVDepth -> u, v, z (fp32)"""
    fx, fy, cx, cy = (float(k) for k in K)
    t0, t1, t2 = transform(E, V)
    with np.errstate(all="ignore"):
        return ((t0 * fx) / t2 + cx).astype(F32), ((t1 * fy) / t2 + cy).astype(F32), t2.astype(F32)


def inside(u, v, w, h):
    """TestImageBoundary(u, v, 10) on doubles"""
    u = np.asarray(u, np.float64); v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return (u >= MARGIN) & (u < w - MARGIN) & (v >= MARGIN) & (v < h - MARGIN)


def round_pixel(u):
    """int(roundf(u)): half away from zero"""
    return (np.sign(u) * np.floor(np.abs(u.astype(np.float64)) + 0.5)).astype(np.int64)


def visibility(V, depths, masks, E, K, option, trace=None):
    """-> bool n_cameras x n_vertices"""
    n, h, w = depths.shape
    out = np.zeros((n, len(V)), bool)
    for c in range(n):
        u, v, z = project(E[c], K, V)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(u) & np.isfinite(v) & np.isfinite(z) & (z >= 0) & (np.abs(u) < 2.0 ** 30) & (np.abs(v) < 2.0 ** 30)
        ud, vd = round_pixel(np.where(ok, u, 0)), round_pixel(np.where(ok, v, 0))
        ok &= (ud >= 0) & (ud < w) & (vd >= 0) & (vd < h)
        ud, vd = np.where(ok, ud, 0), np.where(ok, vd, 0)
        d = depths[c][vd, ud]
        ok &= ~(d.astype(np.float64) > option["maximum_allowable_depth"])
        ok &= masks[c][vd, ud] != 255
        with np.errstate(invalid="ignore"):
            ok &= np.abs(z - d).astype(F32).astype(np.float64) < option["depth_threshold_for_visiblity_check"]
        out[c] = ok
        if trace is not None:
            trace.append(ok.copy())
    return out


def per_vertex(V, vis, E, K, images, channels, trace=None):
    """the proxy's and the colours' walk: per vertex, over its cameras ascending, `channels` values at the rounded pixel
    (images[c] -> h x w x channels f64-exact) -> sums / count (n x channels), 0 without a camera"""
    n, h, w = len(images), images[0].shape[0], images[0].shape[1]
    tot, cnt = np.zeros((len(V), channels)), np.zeros(len(V))
    for c in range(n):
        u, v, _ = project(E[c], K, V)
        ok = vis[c] & inside(u, v, w, h)
        ud, vd = np.where(ok, round_pixel(np.where(ok, u, 0)), 0), np.where(ok, round_pixel(np.where(ok, v, 0)), 0)
        val = images[c][vd, ud].reshape(len(V), channels).astype(np.float64)
        tot = np.where(ok[:, None], tot + val, tot)
        cnt = cnt + ok
        if trace is not None:
            trace.append(np.stack([ok, ud, vd]))
    return np.where(cnt[:, None] > 0, tot / np.maximum(cnt, 1)[:, None], 0.0)


def proxy_intensity(V, vis, E, K, grays, trace=None):
    return per_vertex(V, vis, E, K, [g[..., None] for g in grays], 1, trace)[:, 0]


def vertex_colors(V, vis, E, K, colors, trace=None):
    return per_vertex(V, vis, E, K, [(c.astype(F32) / F32(255.0)).astype(F32) for c in colors], 3, trace)


# ---- the iteration ------------------------------------------------------------------------------------------------------------
def bilinear(img, u, v):
    """FloatValueAt"""
    h, w = img.shape
    ui = np.clip(u.astype(np.int64), 0, w - 2); vi = np.clip(v.astype(np.int64), 0, h - 2)
    pu, pv = u - ui, v - vi
    f = lambda a: a.astype(np.float64)
    return ((f(img[vi, ui]) * (1 - pv) + f(img[vi + 1, ui]) * pv) * (1 - pu) +
            (f(img[vi, ui + 1]) * (1 - pv) + f(img[vi + 1, ui + 1]) * pv) * pu)


def terms(V, visible, pose, K, gray, dx, dy, proxy, trace=None):
    """camera: `visible` its ascending vertex list -> the terms of its 29 sums, one row per accepted vertex"""
    fx, fy, cx, cy = (float(k) for k in K)
    h, w = gray.shape
    P = V[visible]
    G0, G1, G2 = transform(pose, P)
    with np.errstate(all="ignore"):
        u, v = (fx * G0 + cx * G2) / G2, (fy * G1 + cy * G2) / G2
    ok = inside(u, v, w, h)
    if trace is not None:
        trace.append(ok.copy())
    G0, G1, G2, u, v = G0[ok], G1[ok], G2[ok], u[ok], v[ok]
    g, dIdx, dIdy = bilinear(gray, u, v), bilinear(dx, u, v), bilinear(dy, u, v)
    invz = 1.0 / G2
    v0 = dIdx * fx * invz; v1 = dIdy * fy * invz
    v2 = -(v0 * G0 + v1 * G1) * invz
    C = [-G2 * v1 + G1 * v2, G2 * v0 - G0 * v2, -G1 * v0 + G0 * v1, v0, v1, v2]
    r = proxy[visible][ok] - g
    cols = [C[x] * C[y] for x in range(6) for y in range(x, 6)] + [-(r * C[x]) for x in range(6)] + [r * r, np.ones_like(r)]
    return np.stack(cols, 1) if len(r) else np.zeros((0, N_SUMS))


def total(T, how="pairwise"):
    if len(T) == 0:
        return np.zeros(N_SUMS)
    return np.cumsum(T, axis=0)[-1] if how == "sequential" else T.sum(axis=0)


def sum_bound(T):
    """K 2^-53 sum|term| per column, K the camera's count: what two orders of the same f64 sum may differ by (a tree's own
    error is log2 K, not K, units: the bound covers a tree against the serial order)"""
    return len(T) * U * np.abs(T).sum(axis=0)


def unpack(row):
    JJ = np.zeros((6, 6)); k = 0
    for x in range(6):
        for y in range(x, 6):
            JJ[x, y] = JJ[y, x] = row[k]; k += 1
    return JJ, row[21:27].copy()


def delta_of(row):
    """-> the 4 x 4 update of a camera's sums, or None where it keeps its pose"""
    if row[28] < 6:
        return None
    JJ, Jb = unpack(row)
    try:
        x = np.linalg.solve(JJ, -Jb)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(x)):
        return None
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    A = np.eye(4); A[:3, :3] = Rz @ Ry @ Rx; A[:3, 3] = x[3:6]
    return A


class State:
    """everything prepare makes, and the poses"""

    def __init__(self, V, depths, colors, E, K, option, trace=None):
        self.V, self.K, self.option = np.ascontiguousarray(V, np.float64), np.asarray(K, np.float64), option
        self.colors = colors
        self.E = np.array(E, np.float64).reshape(len(depths), 4, 4).copy()
        imgs = [gradient_images(c) for c in colors]
        self.gray, self.dx, self.dy = ([i[k] for i in imgs] for k in range(3))
        self.mask = [depth_mask(d, option["depth_threshold_for_discontinuity_check"], option["half_dilation_kernel_size_for_discontinuity_map"])
                     for d in depths]
        self.vis = visibility(self.V, np.asarray(depths), self.mask, self.E, self.K, option, trace)
        self.lists = [np.flatnonzero(v).astype(np.int32) for v in self.vis]
        self.trace = trace

    def proxy(self):
        return proxy_intensity(self.V, self.vis, self.E, self.K, self.gray, self.trace)

    def terms(self, c, proxy):
        return terms(self.V, self.lists[c], self.E[c], self.K, self.gray[c], self.dx[c], self.dy[c], proxy, self.trace)

    def sums(self, how="pairwise"):
        p = self.proxy()
        return np.stack([total(self.terms(c, p), how) for c in range(len(self.E))])

    def step(self, how="pairwise"):
        """one iteration -> the cameras' rows (n x 29)"""
        rows = self.sums(how)
        for c, row in enumerate(rows):
            A = delta_of(row)
            if A is not None:
                self.E[c] = A @ self.E[c]
        return rows

    def run(self, k, how="pairwise"):
        """-> the residual (sum of rr over the cameras) of every iteration"""
        return np.array([self.step(how)[:, 27].sum() for _ in range(k)])

    def colours(self):
        return vertex_colors(self.V, self.vis, self.E, self.K, self.colors, self.trace)
