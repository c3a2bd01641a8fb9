"""The rule of the mesh renderer (include/visma_icp.h, visma_amd/csrc/render_math.hpp) in numpy f64: what the device, the host
entry point and this file all follow operation for operation.  numpy does not fuse: every product, sum and quotient below
rounds once, in the order written.

    render(V, F, w, h, K, E, z_near, z_far, encoding)  ->  depth (f32), index (i32), mask (u8), z64 (the winner's f64 depth)
    setup_box(A, B, C, w, h, K, z_near)                ->  (x0, y0, x1, y1), inclusive, or None: where a triangle is drawn
    edges(depth)                                       ->  u8
    depth_buffer(z, z_near, z_far), linearize_depth(zb, z_near, z_far)

A triangle is tested only at the pixels of its screen box (setup_box, render_math.hpp's render_setup operation for operation),
and the box is part of the rule: nothing where a camera coordinate is not finite or no vertex lies at z >= z_near, the whole
image where one or two do, the padded box of the projected vertices where all three do.  In exact arithmetic the box contains
every pixel a triangle covers, so it changes nothing there.  In f64 it does: the edge values of a degenerate triangle are
rounding noise, z = det / s is noise over noise, and it lands inside [z_near, z_far] anywhere on the image.  Measured against
exact rationals (test_render_spec.py) at 32 x 24: without the box a triangle whose vertices lie on a line through the camera
centre drew 114 pixels (exact arithmetic: 0), 215 of 1000 random triangles of that family drew pixels outside their box, and
1078 of 3000 scenes with every vertex a few ulps under z_near drew pixels because det / s rounds up to z_near (exact
arithmetic: none).  render(..., unboxed=True) tests every triangle at every pixel as this file once did: for tests only."""
import numpy as np

METRIC, DEPTH_BUFFER = 0, 1
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera_points(V, E):
    V = np.asarray(V, np.float64).reshape(-1, 3)
    E = np.asarray(E, np.float64).reshape(4, 4)
    P = np.empty_like(V)
    with np.errstate(all="ignore"):
        for r in range(3):
            P[:, r] = ((E[r, 0] * V[:, 0] + E[r, 1] * V[:, 1]) + E[r, 2] * V[:, 2]) + E[r, 3]
    return P


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def setup(A, B, C):
    """-> n0, n1, n2, det"""
    n0, n1, n2 = cross(B, C), cross(C, A), cross(A, B)
    det = (A[0] * n0[0] + A[1] * n0[1]) + A[2] * n0[2]
    return n0, n1, n2, det


def span(lo, hi, last):
    """render_span: the pixels floor(lo) - 1 .. ceil(hi) + 1 clamped to [0, last], or None where that misses the image"""
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return 0, last
    lo, hi = np.floor(lo) - 1.0, np.ceil(hi) + 1.0
    if hi < 0.0 or lo > np.float64(last):
        return None
    return (0 if lo < 0.0 else int(lo)), (last if hi > np.float64(last) else int(hi))


def setup_box(A, B, C, w, h, K, z_near):
    """render_setup's box of the camera-space triangle (A, B, C): (x0, y0, x1, y1), inclusive, or None where nothing is drawn"""
    A, B, C = (np.asarray(p, np.float64) for p in (A, B, C))
    fx, fy, cx, cy = (np.float64(x) for x in K)
    z_near = np.float64(z_near)
    if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C).all()):
        return None
    front = int(A[2] >= z_near) + int(B[2] >= z_near) + int(C[2] >= z_near)
    if front == 0:
        return None
    if front < 3:
        return 0, 0, w - 1, h - 1
    with np.errstate(all="ignore"):
        ua, ub, uc = (fx * (p[0] / p[2]) + cx for p in (A, B, C))
        va, vb, vc = (fy * (p[1] / p[2]) + cy for p in (A, B, C))
        xs = span(np.fmin(ua, np.fmin(ub, uc)), np.fmax(ua, np.fmax(ub, uc)), w - 1)    # (fmin, fmax: a NaN loses, as in C)
        ys = span(np.fmin(va, np.fmin(vb, vc)), np.fmax(va, np.fmax(vb, vc)), h - 1)
    if xs is None or ys is None:
        return None
    return xs[0], ys[0], xs[1], ys[1]


def rays(w, h, K):
    fx, fy, cx, cy = (np.float64(x) for x in K)
    dx = (np.arange(w, dtype=np.float64) - cx) / fx
    dy = (np.arange(h, dtype=np.float64) - cy) / fy
    return np.meshgrid(dx, dy)                               # h x w each


def depth_buffer(z, z_near, z_far):
    z_near, z_far = np.float64(z_near), np.float64(z_far)
    return (0.5 * ((z_far + z_near) - ((2.0 * z_near) * z_far) / z)) / (z_far - z_near) + 0.5


def linearize_depth(zb, z_near, z_far):
    zb, z_near, z_far = np.float64(zb), np.float64(z_near), np.float64(z_far)
    return ((2.0 * z_near) * z_far) / ((z_far + z_near) - (2.0 * zb - 1.0) * (z_far - z_near))


def render(V, F, w, h, K, E, z_near, z_far, encoding=METRIC, unboxed=False):
    """unboxed (tests only): every triangle with finite camera points is tested at every pixel, its box ignored"""
    P = camera_points(V, E)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    DX, DY = rays(w, h, K)
    z_near, z_far = np.float64(z_near), np.float64(z_far)
    key = np.full((h, w), NO_KEY, np.uint64)
    z64 = np.zeros((h, w), np.float64)
    with np.errstate(all="ignore"):
        for t, (a, b, c) in enumerate(F):
            A, B, C = P[a], P[b], P[c]
            if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C).all()):
                continue
            box = (0, 0, w - 1, h - 1) if unboxed else setup_box(A, B, C, w, h, K, z_near)
            if box is None:
                continue
            at = (slice(box[1], box[3] + 1), slice(box[0], box[2] + 1))
            dx, dy = DX[at], DY[at]
            n0, n1, n2, det = setup(A, B, C)
            e0 = (n0[0] * dx + n0[1] * dy) + n0[2]
            e1 = (n1[0] * dx + n1[1] * dy) + n1[2]
            e2 = (n2[0] * dx + n2[1] * dy) + n2[2]
            s = (e0 + e1) + e2
            z = det / s
            inside = (s != 0.0) & (((e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)) | ((e0 <= 0.0) & (e1 <= 0.0) & (e2 <= 0.0)))
            drawn = inside & (z >= z_near) & (z <= z_far)
            k = (z.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
            win = drawn & (k < key[at])
            key[at][win] = k[win]                            # (key[at], z64[at]: views of the images)
            z64[at][win] = z[win]
    covered = key != NO_KEY
    index = np.where(covered, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    mask = np.where(covered, 255, 0).astype(np.uint8)
    metric = np.where(covered, (key >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0.0)).astype(np.float32)
    if encoding == METRIC:
        depth = metric
    else:
        with np.errstate(all="ignore"):
            zb = depth_buffer(np.where(covered, z64, 1.0), z_near, z_far).astype(np.float32)
        depth = np.where(covered, zb, np.float32(1.0)).astype(np.float32)
    return depth, index, mask, z64


def edges(depth):
    d = np.asarray(depth, np.float32)
    h, w = d.shape
    with np.errstate(all="ignore"):
        v = np.where(d > 0.0, d.astype(np.float64), -1.0)
    out = np.zeros((h, w), np.uint8)
    if w <= 10 or h <= 10:
        return out
    at = lambda ox, oy: v[5 + oy:h - 5 + oy, 5 + ox:w - 5 + ox]
    with np.errstate(all="ignore"):
        delta = 0.25 * (((np.abs(at(-1, 0) - at(1, 0)) + np.abs(at(0, 1) - at(0, -1))) + np.abs(at(-1, -1) - at(1, 1)))
                        + np.abs(at(-1, 1) - at(1, -1)))
        c = np.where(delta >= 0.10, 1.0, np.where(delta >= 0.05, (delta - 0.05) / 0.05, 0.0))   # (a NaN delta: 0)
        px = np.floor(255.0 * c + 0.5)
    out[5:h - 5, 5:w - 5] = np.where(at(0, 0) == -1.0, 0.0, px).astype(np.uint8)
    return out
