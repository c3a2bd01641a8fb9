"""The numpy specification of RGB-D odometry (Open3D 0.3.0: Core/Odometry/Odometry.cpp, RGBDOdometryJacobian.cpp and the
image functions of Core/Geometry they call), stage by stage, as the library computes it (visma_amd/csrc/odometry*.hip).
tests/golden/odometry.npz (tests/golden/gen_odometry.py) pins it to the compiled reference.

Images are h x w fp32 arrays in C order.  What is exact and what is bounded:

  filters, down-sampling, pyramids, xyz    bit for bit: every operation and its precision is written out below (the fp32
                        product of a pixel and a weight, the f64 sum over the taps in the order -1, 0, +1, one cast).
  normalisation         bit for bit.  The mean is a sum of fp32 values in f64: every gray of magnitude in [2^-10, 2^9) is a
                        multiple of 2^-33, so up to 2^19 of them sum exactly in ANY order and math.fsum is that sum.  The
                        scaled pixel (float)(0.5 / mean * p) then has one value.  (The generator refuses a fixture whose
                        mean depends on the order of its sum; it cannot refuse one with a product near an fp32 rounding
                        midpoint, of which an image of 7,500 pixels is expected to hold some, and need not.)
  correspondences       equal, away from the decisions' boundaries: Trace records how close every decision (the
                        truncation of u_t and v_t, which includes the image border, and the depth-difference test) came.
  J^T J, J^T r, sum r2  two evaluations of these sums differ by at most step_bound: 2 (n + 32) u S per entry, n the number
                        of rows, u = 2^-53, S the sum over the rows of the product of the entries' ABSOLUTE forms -- every
                        J entry and residual with each of its sub-terms replaced by its magnitude, because the differences
                        inside them cancel and the bare terms would not bound them.  2 n u S is the summation in any
                        order on both sides; 2 * 32 u S the rounding of the about 30 operations behind one term, twice.
                        The photometric difference is ONE fp32 subtraction on both sides (as the reference writes it) and
                        carries no error of its own.

Deviations of the library that the specification shares (include/visma_icp.h): a source pixel whose transformed depth is
<= 0 or whose projection is not finite has no pair; an all-zero initial pose is the identity everywhere; the information
matrix is the pure sum (the reference adds (1 + OpenMP threads) I) and the zero matrix on failure."""
import math

import numpy as np

GAUSSIAN3 = (0.25, 0.5, 0.25)
SOBEL31 = (-1.0, 0.0, 1.0)
SOBEL32 = (1.0, 2.0, 1.0)
SOBEL_SCALE = 0.125
LAMBDA_HYBRID_DEPTH = 0.968
COLOR, HYBRID = 0, 1
U = 2.0 ** -53
F32 = np.float32


def default_option():
    return dict(iterations=[20, 10, 5], max_depth_diff=0.03, min_depth=0.0, max_depth=4.0)


def same_image(a, b):
    """bit for bit, a NaN equal to any NaN (its sign and payload are not part of the contract)"""
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def image_digest(a):
    """SHA-256 of the fp32 bytes with every NaN made canonical -> 32 uint8"""
    import hashlib
    a = np.ascontiguousarray(a, F32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return np.frombuffer(hashlib.sha256(b.tobytes()).digest(), np.uint8).copy()


# ---- images -----------------------------------------------------------------------------------------------------------
def filter_horizontal(img, k):
    h, w = img.shape
    x = np.arange(w)
    acc = np.zeros((h, w), np.float64)
    with np.errstate(invalid="ignore"):
        for i, wt in zip((-1, 0, 1), k):
            prod = img[:, np.clip(x + i, 0, w - 1)] * F32(wt)          # fp32 product
            acc = acc + prod.astype(np.float64)                        # f64 sum, tap order -1, 0, +1
    return acc.astype(F32)


def filter_image(img, kx, ky):
    """a horizontal pass, then the same arithmetic down the columns (the reference transposes in between)"""
    return np.ascontiguousarray(filter_horizontal(np.ascontiguousarray(filter_horizontal(img, kx).T), ky).T)


def gaussian3(img): return filter_image(img, GAUSSIAN3, GAUSSIAN3)
def sobel_dx(img): return filter_image(img, SOBEL31, SOBEL32)
def sobel_dy(img): return filter_image(img, SOBEL32, SOBEL31)


def downsample(img):
    h, w = img.shape
    oh, ow = h // 2, w // 2
    a = img[0:2 * oh:2, 0:2 * ow:2]; b = img[0:2 * oh:2, 1:2 * ow:2]
    c = img[1:2 * oh:2, 0:2 * ow:2]; d = img[1:2 * oh:2, 1:2 * ow:2]
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray((((a + b) + c) + d) / F32(4.0))


def preprocess_depth(depth, option):
    d = np.array(depth, F32)
    d64 = d.astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad = (d64 < option["min_depth"]) | (d64 > option["max_depth"]) | (d <= 0)
    d[bad] = np.nan
    return d


def camera_matrix(intrinsic, level=0):
    fx, fy, cx, cy = [float(v) for v in intrinsic]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    for _ in range(level):
        K = 0.5 * K
        K[2, 2] = 1.0
    return K


def xyz_image(depth, K):
    h, w = depth.shape
    z = depth.astype(np.float64)
    x = np.arange(w, dtype=np.float64)[None, :]; y = np.arange(h, dtype=np.float64)[:, None]
    inv_fx, inv_fy = 1.0 / K[0, 0], 1.0 / K[1, 1]
    with np.errstate(invalid="ignore"):
        return np.stack([((x - K[0, 2]) * z * inv_fx).astype(F32), ((y - K[1, 2]) * z * inv_fy).astype(F32), depth.astype(F32)], -1)


def pose_or_identity(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return np.eye(4) if np.all(T == 0.0) else T


# ---- correspondences --------------------------------------------------------------------------------------------------
class Trace:
    """how close the correspondence decisions came to their boundaries, relative to the quantity tested"""
    def __init__(self):
        self.rounding = np.inf
        self.depth = np.inf

    def margin(self):
        return min(self.rounding, self.depth)


def correspondences(K, T, depth_s, depth_t, max_depth_diff, trace=None):
    """-> idx (h * w int32): the target pixel v_t * w + u_t of source pixel v_s * w + u_s, or -1"""
    h, w = depth_s.shape
    T = pose_or_identity(T)
    M = K @ T[:3, :3] @ np.linalg.inv(K)
    Kt = K @ T[:3, 3]
    u = np.arange(w, dtype=np.float64)[None, :]; v = np.arange(h, dtype=np.float64)[:, None]
    d = depth_s.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = d * (M[0, 0] * u + M[0, 1] * v + M[0, 2]) + Kt[0]
        y = d * (M[1, 0] * u + M[1, 1] * v + M[1, 2]) + Kt[1]
        z = d * (M[2, 0] * u + M[2, 1] * v + M[2, 2]) + Kt[2]
        qu, qv = x / z + 0.5, y / z + 0.5
        ok = ~np.isnan(d) & (z > 0) & np.isfinite(qu) & np.isfinite(qv) & (np.abs(qu) < 2.0 ** 30) & (np.abs(qv) < 2.0 ** 30)
        ut = np.where(ok, np.trunc(np.where(ok, qu, 0)), -1).astype(np.int64)
        vt = np.where(ok, np.trunc(np.where(ok, qv, 0)), -1).astype(np.int64)
        if trace is not None and ok.any():
            for q in (qu[ok], qv[ok]):
                r = np.rint(q)
                m = np.abs(q - r) / np.maximum(np.abs(q), 1.0)
                m = m[r != 0]                                          # (truncation has no boundary at 0)
                if m.size:
                    trace.rounding = min(trace.rounding, float(m.min()))
        inside = ok & (ut >= 0) & (ut < w) & (vt >= 0) & (vt < h)
        dt = np.where(inside, depth_t[np.clip(vt, 0, h - 1), np.clip(ut, 0, w - 1)], np.nan).astype(np.float64)
        diff = np.abs(z - dt)
        pair = inside & ~np.isnan(dt) & (diff <= max_depth_diff)
        if trace is not None:
            t = inside & ~np.isnan(dt)
            if t.any() and max_depth_diff > 0:
                trace.depth = min(trace.depth, float((np.abs(diff[t] - max_depth_diff) / max_depth_diff).min()))
    return np.where(pair, vt * w + ut, -1).astype(np.int32).ravel()


# ---- preparation ------------------------------------------------------------------------------------------------------
WHICH = ("src_gray", "src_depth", "tgt_gray", "tgt_depth", "tgt_gray_dx", "tgt_gray_dy", "tgt_depth_dx", "tgt_depth_dy", "src_xyz")


def normalize_intensity(gray_s, gray_t, idx):
    s = np.flatnonzero(idx >= 0)
    t = idx[s]
    K = len(s)
    out = []
    for g, at in ((gray_s, s), (gray_t, t)):
        mean = math.fsum(g.ravel()[at].astype(np.float64).tolist()) / K if K else float("nan")
        with np.errstate(invalid="ignore", divide="ignore"):
            scale = np.float64(0.5) / np.float64(mean)
            out.append(((scale * g.astype(np.float64)) + 0.0).astype(F32))
    return out[0], out[1], K


def normalized_products(gray, idx_positions, K):
    """the f64 products of normalize_intensity (the generator's midpoint test)"""
    mean = math.fsum(gray.ravel()[idx_positions].astype(np.float64).tolist()) / K
    return (0.5 / mean) * gray.astype(np.float64)


def prepare(src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init, option, n_levels=None, trace=None):
    """-> a dict: levels (a list of dicts of the WHICH images, level 0 first), K (camera matrix per level),
    tgt_xyz (level 0), init_pairs"""
    n_levels = len(option["iterations"]) if n_levels is None else n_levels
    sg, tg = gaussian3(np.asarray(src_gray, F32)), gaussian3(np.asarray(tgt_gray, F32))
    sd = gaussian3(preprocess_depth(src_depth, option)); td = gaussian3(preprocess_depth(tgt_depth, option))
    K0 = camera_matrix(intrinsic)
    idx = correspondences(K0, init, sd, td, option["max_depth_diff"], trace)
    sg, tg, pairs = normalize_intensity(sg, tg, idx)
    levels = []
    for l in range(n_levels):
        if l > 0:
            p = levels[-1]
            sg, tg = downsample(gaussian3(p["src_gray"])), downsample(gaussian3(p["tgt_gray"]))
            sd, td = downsample(p["src_depth"]), downsample(p["tgt_depth"])
        Kl = camera_matrix(intrinsic, l)
        levels.append(dict(src_gray=sg, src_depth=sd, tgt_gray=tg, tgt_depth=td,
                           tgt_gray_dx=sobel_dx(tg), tgt_gray_dy=sobel_dy(tg), tgt_depth_dx=sobel_dx(td), tgt_depth_dy=sobel_dy(td),
                           src_xyz=xyz_image(sd, Kl)))
    return dict(levels=levels, K=[camera_matrix(intrinsic, l) for l in range(n_levels)],
                tgt_xyz=xyz_image(levels[0]["tgt_depth"], K0), init_pairs=pairs, option=option)


# ---- the step ---------------------------------------------------------------------------------------------------------
def jacobian_rows(level, K, T, idx, method):
    """-> J (n x 6), r (n), and their absolute forms Ja, ra; n = pairs (colour) or 2 x pairs (hybrid: photometric rows first)"""
    T = pose_or_identity(T)
    s = np.flatnonzero(idx >= 0); t = idx[s]
    f = lambda name, at: level[name].ravel()[at]
    fx, fy = K[0, 0], K[1, 1]
    R, tr = T[:3, :3], T[:3, 3]
    P = level["src_xyz"].reshape(-1, 3)[s].astype(np.float64)
    p = [R[i, 0] * P[:, 0] + R[i, 1] * P[:, 1] + R[i, 2] * P[:, 2] + tr[i] for i in range(3)]
    pa = [abs(R[i, 0]) * abs(P[:, 0]) + abs(R[i, 1]) * abs(P[:, 1]) + abs(R[i, 2]) * abs(P[:, 2]) + abs(tr[i]) for i in range(3)]
    invz = 1.0 / p[2]
    ainvz = np.abs(invz)

    def row(gx, gy, scale, minus_z):
        """J = scale * [the row of a value with image gradient (gx, gy) at the projection], and its absolute form"""
        c0 = gx * fx * invz; c1 = gy * fy * invz
        c2 = -(c0 * p[0] + c1 * p[1]) * invz
        a0, a1 = np.abs(c0), np.abs(c1)
        a2 = (a0 * pa[0] + a1 * pa[1]) * ainvz
        if not minus_z:
            J = [-p[2] * c1 + p[1] * c2, p[2] * c0 - p[0] * c2, -p[1] * c0 + p[0] * c1, c0, c1, c2]
            A = [pa[2] * a1 + pa[1] * a2, pa[2] * a0 + pa[0] * a2, pa[1] * a0 + pa[0] * a1, a0, a1, a2]
        else:                                                           # the depth row: d/dxi of (D_t(proj) - z)
            J = [(-p[2] * c1 + p[1] * c2) - p[1], (p[2] * c0 - p[0] * c2) + p[0], -p[1] * c0 + p[0] * c1, c0, c1, c2 - 1.0]
            A = [pa[2] * a1 + pa[1] * a2 + pa[1], pa[2] * a0 + pa[0] * a2 + pa[0], pa[1] * a0 + pa[0] * a1, a0, a1, a2 + 1.0]
        return scale * np.stack(J, 1), scale * np.stack(A, 1)

    gt, gs = f("tgt_gray", t), f("src_gray", s)
    with np.errstate(invalid="ignore"):
        diff_photo = (gt - gs).astype(np.float64)                       # ONE fp32 subtraction, then widened
    adiff_photo = np.abs(diff_photo)                                    # (exactly the same number on both sides)
    dIdx = SOBEL_SCALE * f("tgt_gray_dx", t).astype(np.float64); dIdy = SOBEL_SCALE * f("tgt_gray_dy", t).astype(np.float64)
    if method == COLOR:
        J, A = row(dIdx, dIdy, 1.0, False)
        return J, diff_photo, A, adiff_photo
    s_img, s_dep = math.sqrt(1.0 - LAMBDA_HYBRID_DEPTH), math.sqrt(LAMBDA_HYBRID_DEPTH)
    dDdx = SOBEL_SCALE * f("tgt_depth_dx", t).astype(np.float64); dDdy = SOBEL_SCALE * f("tgt_depth_dy", t).astype(np.float64)
    dDdx = np.where(np.isnan(dDdx), 0.0, dDdx); dDdy = np.where(np.isnan(dDdy), 0.0, dDdy)
    dt = f("tgt_depth", t).astype(np.float64)
    diff_geo = dt - p[2]
    Jp, Ap = row(dIdx, dIdy, s_img, False)
    Jg, Ag = row(dDdx, dDdy, s_dep, True)
    return (np.concatenate([Jp, Jg]), np.concatenate([s_img * diff_photo, s_dep * diff_geo]),
            np.concatenate([Ap, Ag]), np.concatenate([s_img * adiff_photo, s_dep * (np.abs(dt) + pa[2])]))


def step_sums(level, K, T, idx, method):
    """-> dict: K (pairs), rows, JTJ (6 x 6), JTr (6), r2, and S_JTJ, S_JTr, S_r2 (the sums of the absolute forms)"""
    J, r, A, ra = jacobian_rows(level, K, T, idx, method)
    fs = lambda v: math.fsum(v.tolist())
    JTJ = np.array([[fs(J[:, a] * J[:, b]) for b in range(6)] for a in range(6)])
    JTr = np.array([fs(J[:, a] * r) for a in range(6)])
    return dict(K=int(np.count_nonzero(idx >= 0)), rows=len(r), JTJ=JTJ, JTr=JTr, r2=fs(r * r),
                S_JTJ=A.T @ A, S_JTr=A.T @ ra, S_r2=float(ra @ ra))


def step_bound(rows, S):
    """two evaluations of a sum over `rows` terms whose absolute forms sum to S"""
    return 2.0 * (rows + 32) * U * np.asarray(S, np.float64)


def solve_step(JTJ, JTr):
    """-> ok, the 4 x 4 update: x = -(J^T J)^-1 J^T r as Rz(x2) Ry(x1) Rx(x0) and the translation x[3:]; |det| < 1e-6: no solution"""
    det = np.linalg.det(JTJ)
    if not np.isfinite(det) or abs(det) < 1e-6:
        return False, np.eye(4), det
    x = np.linalg.solve(JTJ, -JTr)
    ca, sa, cb, sb, cg, sg = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    T = np.eye(4)
    T[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                 [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    T[:3, 3] = x[3:]
    return True, T, det


def multiscale(prep, init, method, option, trace=None):
    """-> ok, T, poses (the pose after every iteration), counts (the pairs of every iteration), dets"""
    T = pose_or_identity(init).copy()
    its = option["iterations"]
    n = len(its)
    poses, counts, dets = [], [], []
    for level in range(n - 1, -1, -1):
        L, K = prep["levels"][level], prep["K"][level]
        for _ in range(its[n - level - 1]):
            idx = correspondences(K, T, L["src_depth"], L["tgt_depth"], option["max_depth_diff"], trace)
            s = step_sums(L, K, T, idx, method)
            counts.append(s["K"])
            ok, dT, det = solve_step(s["JTJ"], s["JTr"]) if s["K"] > 0 else (False, np.eye(4), 0.0)
            dets.append(det)
            T = dT @ T
            poses.append(T.copy())
            if not ok:
                return False, np.eye(4), poses, counts, dets
    return True, T, poses, counts, dets


# ---- the information matrix -------------------------------------------------------------------------------------------
def information_terms(q):
    """sum G^T G over the points q (K x 3), G = [-hat(q) | I], and per entry the sum of |term|"""
    M, S = np.zeros((6, 6)), np.zeros((6, 6))
    fs = lambda v: math.fsum(np.asarray(v, np.float64).tolist())
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    rows = [(np.zeros_like(x), z, -y, 1, 0, 0), (-z, np.zeros_like(x), x, 0, 1, 0), (y, -x, np.zeros_like(x), 0, 0, 1)]
    one = np.ones_like(x)
    for g in rows:
        g = [c * one if np.isscalar(c) else c for c in g]
        for a in range(6):
            for b in range(6):
                t = g[a] * g[b]
                M[a, b] += fs(t); S[a, b] += fs(np.abs(t))
    return M, S


def information_bound(K, S):
    return 2.0 * (K + 4) * U * S


def information(prep, T, option, trace=None):
    """-> the 6 x 6 (the pure sum), K, the absolute sums"""
    L = prep["levels"][0]
    idx = correspondences(prep["K"][0], T, L["src_depth"], L["tgt_depth"], option["max_depth_diff"], trace)
    t = idx[idx >= 0]
    M, S = information_terms(prep["tgt_xyz"].reshape(-1, 3)[t].astype(np.float64))
    return M, len(t), S


def rgbd_odometry(src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init, method, option, trace=None):
    """-> ok, T, info, extras"""
    prep = prepare(src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init, option, trace=trace)
    ok, T, poses, counts, dets = multiscale(prep, init, method, option, trace)
    extras = dict(prep=prep, poses=poses, counts=counts, dets=dets, info_K=0)
    if not ok:
        return False, np.eye(4), np.zeros((6, 6)), extras
    M, K, S = information(prep, T, option, trace)
    extras.update(info_K=K, info_S=S)
    return True, T, M, extras
