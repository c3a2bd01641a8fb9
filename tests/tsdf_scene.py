"""A numpy ray-caster for the TSDF tests: depth, RGB8 and float-gray frames of one small scene from known poses.

  scene     two tilted planes, n . p = c with n = (0.2, 1, 0.1), c = 0.45 (a floor) and n = (0.15, -0.1, 1), c = 0.55 (a
            back wall), and a sphere of radius 0.3 at (0.05, -0.05, 0.05): along every axis the signed distance changes
            sign, and the scene straddles the world's origin
  pinhole   fx = fy = 0.9 w, centre ((w - 1) / 2, (h - 1) / 2)
  cameras   four, looking at the scene from z < 0: camera_to_world(i); the LAST one stands inside the volume the tests
            integrate into, so that voxels lie behind it.  extrinsic(i), what Integrate takes, is its inverse.
  texture   0.5 + 0.2 sin(7x + 1) cos(5y) + 0.2 sin(9z + 3x) of the world point: the gray frame; the RGB8 frame is
            (g, 1 - g, 0.5 + 0.5 sin(11 y)) * 255, rounded
  holes     a ray that hits nothing and a block of pixels per frame have depth 0

Depth is the z coordinate in the camera's frame, fp32, h x w in C order."""
import numpy as np

N_FRAMES = 4
_POSES = (((0.05, -0.10, 0.02), (0.25, 0.10, -2.0)), ((-0.06, 0.22, -0.03), (-0.55, 0.05, -1.9)),
          ((0.12, -0.25, 0.05), (0.60, -0.20, -1.8)), ((0.03, 0.08, -0.04), (-0.10, 0.02, -0.72)))
PLANES = (((0.2, 1.0, 0.1), 0.45), ((0.15, -0.1, 1.0), 0.55))
SPHERE = ((0.05, -0.05, 0.05), 0.3)


def rigid(w, t):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    T = np.eye(4)
    if th > 0:
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = t
    return T


def camera_to_world(i):
    return rigid(*_POSES[i])


def extrinsic(i):
    """world -> camera: R^T, -R^T t written out (no general inverse: the tests' inputs do not depend on one)"""
    C = camera_to_world(i)
    E = np.eye(4)
    E[:3, :3] = C[:3, :3].T
    E[:3, 3] = -C[:3, :3].T @ C[:3, 3]
    return E


def intrinsic(w, h):
    """fx, fy, cx, cy"""
    return np.array([0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0])


def texture(P):
    return 0.5 + 0.2 * np.sin(7 * P[..., 0] + 1) * np.cos(5 * P[..., 1]) + 0.2 * np.sin(9 * P[..., 2] + 3 * P[..., 0])


def render(w, h, i):
    """-> depth (h x w fp32), rgb (h x w x 3 uint8), gray (h x w fp32) of camera i"""
    C = camera_to_world(i)
    fx, fy, cx, cy = intrinsic(w, h)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones((h, w))], -1)
    R, o = C[:3, :3], C[:3, 3]
    dw = d @ R.T
    best = np.full((h, w), np.inf)
    for n, c in PLANES:
        n = np.array(n); den = dw @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (c - o @ n) / den
        best = np.minimum(best, np.where((den > 1e-9) & (t > 0), t, np.inf))
    oc = o - np.array(SPHERE[0])
    a = (dw * dw).sum(-1); b = 2 * (dw @ oc); c = oc @ oc - SPHERE[1] ** 2
    disc = b * b - 4 * a * c
    t = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), np.inf)
    best = np.minimum(best, np.where(t > 0, t, np.inf))
    hit = np.isfinite(best) & (best < 6.0)
    z = np.where(hit, best, 0.0)
    P = o + dw * z[..., None]
    g = texture(P)
    rgb = np.stack([g, 1.0 - g, 0.5 + 0.5 * np.sin(11 * P[..., 1])], -1)
    depth = z.astype(np.float32)                                       # (the ray has z = 1: its parameter is the depth)
    s = lambda a, n: int(round(a * n))
    y0, x0 = s(0.15 + 0.2 * i, h), s(0.7 - 0.2 * i, w)
    depth[y0:y0 + max(1, h // 10), x0:x0 + max(1, w // 8)] = 0.0
    return (np.ascontiguousarray(depth), np.ascontiguousarray(np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8)),
            np.ascontiguousarray(g.astype(np.float32)))


def frames(w, h, n=N_FRAMES):
    """-> [(depth, rgb, gray, extrinsic)] of the first n cameras, and the intrinsic [fx, fy, cx, cy]"""
    return [render(w, h, i) + (extrinsic(i),) for i in range(n)], intrinsic(w, h)
