"""A numpy ray-caster for the RGB-D odometry tests: a pair of (gray, depth) frames of any size of one small scene.

  pinhole   fx = fy = 0.9 w, centre ((w - 1) / 2, (h - 1) / 2)
  scene     a wall z = 3, a floor y = 0.8, a sphere of radius 0.5 at (0.15, 0.2, 2.2)
  intensity 0.5 + 0.2 sin(7x + 1) cos(5y) + 0.2 sin(9z + 3x) of the world point
  cameras   the source at the identity, the target moved by the rotation vector (0.004, -0.012, 0.006) and the
            translation (0.015, -0.005, 0.01)
  holes     a block of zero depth in each frame (at the same relative place for every size)

Depth is the z coordinate in the camera's frame, fp32; the gray image is fp32 too.  truth() is the pose that takes
source-camera coordinates to target-camera coordinates: what the odometry estimates."""
import numpy as np

ROTVEC = (0.004, -0.012, 0.006)
TRANSLATION = (0.015, -0.005, 0.01)


def rigid(w, t):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    T = np.eye(4)
    if th > 0:
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = t
    return T


def intrinsic(w, h):
    """fx, fy, cx, cy"""
    return np.array([0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0])


def texture(P):
    return 0.5 + 0.2 * np.sin(7 * P[..., 0] + 1) * np.cos(5 * P[..., 1]) + 0.2 * np.sin(9 * P[..., 2] + 3 * P[..., 0])


def render(w, h, camera_to_world):
    fx, fy, cx, cy = intrinsic(w, h)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones((h, w))], -1)
    R, o = camera_to_world[:3, :3], camera_to_world[:3, 3]
    dw = d @ R.T
    best = np.full((h, w), np.inf)
    for n, c in (((0, 0, 1.0), 3.0), ((0, 1.0, 0), 0.8)):              # the wall, the floor
        n = np.array(n); den = dw @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (c - o @ n) / den
        best = np.minimum(best, np.where((den > 1e-9) & (t > 0), t, np.inf))
    oc = o - np.array([0.15, 0.2, 2.2])                                 # the sphere
    a = (dw * dw).sum(-1); b = 2 * (dw @ oc); c = oc @ oc - 0.25
    disc = b * b - 4 * a * c
    t = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), np.inf)
    best = np.minimum(best, np.where(t > 0, t, np.inf))
    P = o + dw * best[..., None]
    return texture(P).astype(np.float32), best.astype(np.float32)     # (the ray has z = 1: its parameter is the depth)


def frames(w, h):
    """-> src_gray, src_depth, tgt_gray, tgt_depth (h x w fp32, C order), intrinsic [fx, fy, cx, cy]"""
    sg, sd = render(w, h, np.eye(4))
    tg, td = render(w, h, rigid(ROTVEC, TRANSLATION))
    s = lambda a, n: int(round(a * n))
    sd[s(10 / 75, h):s(18 / 75, h), s(0.6, w):s(0.7, w)] = 0.0
    td[s(40 / 75, h):s(44 / 75, h), s(0.05, w):s(0.3, w)] = 0.0
    return (np.ascontiguousarray(sg), np.ascontiguousarray(sd), np.ascontiguousarray(tg), np.ascontiguousarray(td),
            intrinsic(w, h))


def truth():
    return np.linalg.inv(rigid(ROTVEC, TRANSLATION))
