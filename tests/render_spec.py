"""The rule of the mesh renderer (include/visma_icp.h, visma_amd/csrc/render_math.hpp) in numpy f64: what the device, the host
entry point and this file all follow operation for operation.  numpy does not fuse: every product, sum and quotient below
rounds once, in the order written.

    render(V, F, w, h, K, E, z_near, z_far, encoding)  ->  depth (f32), index (i32), mask (u8), z64 (the winner's f64 depth)
    edges(depth)                                       ->  u8
    depth_buffer(z, z_near, z_far), linearize_depth(zb, z_near, z_far)

Every triangle is tested at every pixel: the screen box of the implementations is a search bound only."""
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


def render(V, F, w, h, K, E, z_near, z_far, encoding=METRIC):
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
            n0, n1, n2, det = setup(A, B, C)
            e0 = (n0[0] * DX + n0[1] * DY) + n0[2]
            e1 = (n1[0] * DX + n1[1] * DY) + n1[2]
            e2 = (n2[0] * DX + n2[1] * DY) + n2[2]
            s = (e0 + e1) + e2
            z = det / s
            inside = (s != 0.0) & (((e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)) | ((e0 <= 0.0) & (e1 <= 0.0) & (e2 <= 0.0)))
            drawn = inside & (z >= z_near) & (z <= z_far)
            k = (z.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
            win = drawn & (k < key)
            key[win] = k[win]
            z64[win] = z[win]
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
