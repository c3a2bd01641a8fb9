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


def render(w, h, camera_to_world, k=None):
    fx, fy, cx, cy = intrinsic(w, h) if k is None else k
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


def frames(w, h, k=None):
    """-> src_gray, src_depth, tgt_gray, tgt_depth (h x w fp32, C order), intrinsic [fx, fy, cx, cy] (k, or intrinsic(w, h))"""
    sg, sd = render(w, h, np.eye(4), k)
    tg, td = render(w, h, rigid(ROTVEC, TRANSLATION), k)
    s = lambda a, n: int(round(a * n))
    sd[s(10 / 75, h):s(18 / 75, h), s(0.6, w):s(0.7, w)] = 0.0
    td[s(40 / 75, h):s(44 / 75, h), s(0.05, w):s(0.3, w)] = 0.0
    return (np.ascontiguousarray(sg), np.ascontiguousarray(sd), np.ascontiguousarray(tg), np.ascontiguousarray(td),
            intrinsic(w, h) if k is None else np.asarray(k, np.float64))


def truth():
    return np.linalg.inv(rigid(ROTVEC, TRANSLATION))


# ---------------------------------------------------------------------------
# hostile frames (tests/test_odometry_hostile.py, tests/golden/gen_rgbd_hostile.py)
# ---------------------------------------------------------------------------
def asymmetric_intrinsic(w, h):
    """fx != fy, and a principal point that is no integer and lies off the centre"""
    return np.array([0.9 * w, 1.15 * w, 0.43 * w + 0.3, 0.57 * h - 0.2])


# what a sensor hands over besides a depth, (v, u) -> value, in the source and in the target of a 16 x 12 pair
HOSTILE_SRC = (((1, 2), np.nan), ((2, 9), np.inf), ((5, 5), -np.inf), ((7, 12), -1.0), ((9, 3), 0.0), ((10, 10), 0.2), ((4, 14), 1e30))
HOSTILE_TGT = (((2, 3), np.inf), ((3, 11), np.nan), ((6, 7), -1.0), ((8, 1), -np.inf), ((10, 13), 0.0), ((1, 8), 0.25), ((9, 9), 1e-40))


def hostile_frames():
    """16 x 12 under the asymmetric intrinsic; NaN, +inf, -inf, negative, 0, below min_depth = 0.3 and absurd depths planted in
    BOTH frames (every one of them becomes NaN in the processed depth and spreads through the 3 x 3 filters)"""
    w, h = 16, 12
    sg, sd, tg, td, k = frames(w, h, asymmetric_intrinsic(w, h))
    with np.errstate(all="ignore"):
        for (v, u), d in HOSTILE_SRC:
            sd[v, u] = np.float32(d)
        for (v, u), d in HOSTILE_TGT:
            td[v, u] = np.float32(d)
    return sg, sd, tg, td, k


def constant_frames(w=9, h=7):
    """constant gray over a fronto-parallel plane: every image gradient is zero, both methods' systems are singular"""
    g, d = np.full((h, w), 0.5, np.float32), np.full((h, w), 1.5, np.float32)
    return g, d, g.copy(), d.copy(), intrinsic(w, h)


# pairs -> the block (rows, columns) of pixels with a depth, from (2, 1): a pixel of the filtered depth is a number only where
# its whole 3 x 3 neighbourhood is, so a block of r x c leaves (r - 2) x (c - 2) pixels to pair
FEW_PAIR_BLOCKS = {1: (3, 3), 2: (3, 4), 3: (3, 5), 4: (4, 4), 5: (3, 7), 6: (4, 5)}


def few_pair_frames(n):
    """9 x 7 frames of the scene with a depth only inside a block that leaves exactly n pairs at the identity: the target has
    its own gray image and the SOURCE's depth (at 9 x 7 a pixel of the floor is far deeper than its neighbour, and the
    target's own depth would drop pairs through the depth-difference test)"""
    sg, sd, tg, td, k = frames(9, 7)
    r, c = FEW_PAIR_BLOCKS[n]
    keep = np.zeros((7, 9), bool)
    keep[2:2 + r, 1:1 + c] = True
    sd = np.where(keep, sd, 0).astype(np.float32)
    return sg, sd, tg, sd.copy(), k


def hostile_cases():
    """name -> (frames, the hybrid run's iterations per level, the colour run's, min_depth): the cases of
    tests/golden/rgbd_hostile.npz, which holds their results only"""
    cases = {"o_const": (constant_frames(), [3], [3], 0.0)}
    for n in sorted(FEW_PAIR_BLOCKS):
        cases["o_n%d" % n] = (few_pair_frames(n), [3], [3], 0.0)
    cases["o_v"] = (hostile_frames(), [5], [2], 0.3)                  # one level: the full runs
    cases["o_v2"] = (hostile_frames(), [1, 1], [1], 0.3)              # two levels: NaN through the down-sampling
    for w, h in ((1, 1), (1, 5), (5, 1)):
        cases["o_%dx%d" % (w, h)] = (frames(w, h), [2], [2], 0.0)
    cases["o_9x7"] = (frames(9, 7), [3, 2], [2], 0.0)
    cases["o_deep"] = (frames(256, 128, asymmetric_intrinsic(256, 128)), [1] * 8, [1], 0.0)   # the deepest pyramid there is
    return cases
