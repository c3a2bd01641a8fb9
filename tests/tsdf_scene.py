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


def render(w, h, i, k=None):
    """-> depth (h x w fp32), rgb (h x w x 3 uint8), gray (h x w fp32) of camera i; k: another intrinsic than intrinsic(w, h)"""
    C = camera_to_world(i)
    fx, fy, cx, cy = intrinsic(w, h) if k is None else k
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


# ---------------------------------------------------------------------------
# hostile frames (tests/test_tsdf_hostile.py, tests/golden/gen_rgbd_hostile.py)
# ---------------------------------------------------------------------------
def asymmetric_intrinsic(w, h):
    """fx != fy, and a principal point that is no integer and lies off the centre"""
    return np.array([0.9 * w, 1.15 * w, 0.43 * w + 0.3, 0.57 * h - 0.2])


def asymmetric_frames(w, h, n=N_FRAMES):
    k = asymmetric_intrinsic(w, h)
    return [render(w, h, i, k) + (extrinsic(i),) for i in range(n)], k


# what a sensor hands over besides a depth: (v, u) -> value, on a 16 x 12 frame.  The first block lies on the pixels a
# stride of 4 visits ((0, 0) stays ordinary: it is all that a stride beyond the image leaves), (5, 10) and (10, 5) on
# those a stride of 5 visits, the rest in between.  +inf stands on both sides of the principal point's column.
HOSTILE_W, HOSTILE_H = 16, 12
HOSTILE_DEPTHS = (((0, 12), np.inf), ((4, 0), np.inf), ((8, 8), 1e30), ((0, 4), np.nan), ((4, 8), -np.inf), ((8, 0), -1.0),
                  ((4, 12), 1e-40), ((8, 12), 0.0),
                  ((5, 10), np.inf), ((10, 5), 1e30),
                  ((5, 7), np.inf), ((6, 9), 1e30), ((3, 3), np.nan), ((7, 2), 1e-40), ((10, 14), -np.inf), ((2, 10), -1.0),
                  ((9, 5), 0.0))


def hostile_frames(cameras=(3, 0)):
    """16 x 12 frames of the given cameras under the asymmetric intrinsic, with HOSTILE_DEPTHS planted in each: NaN, +inf,
    -inf, -1, 1e-40 (a denormal in fp32), 1e30 and 0 among ordinary depths -> [(depth, rgb, gray, extrinsic)], intrinsic"""
    k = asymmetric_intrinsic(HOSTILE_W, HOSTILE_H)
    out = []
    for i in cameras:
        depth, rgb, gray = render(HOSTILE_W, HOSTILE_H, i, k)
        with np.errstate(all="ignore"):
            for (v, u), d in HOSTILE_DEPTHS:
                depth[v, u] = np.float32(d)
        out.append((depth, rgb, gray, extrinsic(i)))
    return out, k


def non_finite_frame():
    """16 x 12 of nothing but +inf, NaN, -inf and 1e30 (no pixel back-projects to a point a unit index can hold)"""
    k = asymmetric_intrinsic(HOSTILE_W, HOSTILE_H)
    depth, rgb, gray = render(HOSTILE_W, HOSTILE_H, 0, k)
    vals = np.array([np.inf, np.nan, -np.inf, 1e30], np.float32)
    depth = vals[(np.arange(HOSTILE_W)[None, :] + np.arange(HOSTILE_H)[:, None]) % 4].astype(np.float32)
    return (np.ascontiguousarray(depth), rgb, gray, extrinsic(0)), k


def edge_case(name):
    """The tiny frames of the image-edge cases, in exactly representable numbers: a volume of 5^3 voxels of 0.25 whose
    column (2, 2) lies on the optical axis (px = py = 0 exactly), identity rotation, voxel centres at pz = -0.25, 0 (exactly),
    0.25, 0.5, 0.75; fx = 4, fy = 2 (powers of two); constant depth 0.375 (a sign change between z = 2 and z = 3).  In fp32 the column's u_f is cx + 0.5 exactly, so
    the principal point decides on which side of 0.0001 or of w - 0.0001 it lands:

      1x1, 7x1, 1x7     (w x h) a principal point inside the image
      u_hi_out / u_hi_in    w = 7: u_f == fp32(7 - 0.0001f) exactly (the first value that is NOT inside) / one ulp below it
      u_lo_out / u_lo_in    w = 7: u_f = 3355 x 2^-25 < 0.0001f / 3356 x 2^-25 > 0.0001f (the neighbours of 0.0001f among the values
                            cx + 0.5 can take)
      v_*                   the same for v_f with h = 7

    -> dict(w, h, depth, rgb, gray, extrinsic, intrinsic, length, R, sdf_trunc, origin)"""
    f32 = np.float32
    shapes = {"1x1": (1, 1), "7x1": (7, 1), "1x7": (1, 7)}
    if name in shapes:
        w, h = shapes[name]
        cx, cy = 0.25 * (w - 1) + 0.125, 0.5 * (h - 1) - 0.125
    else:
        axis, side, where = name.split("_")
        w, h = (7, 1) if axis == "u" else (1, 7)
        if side == "hi":
            c = f32(f32(7.0) - f32(0.0001)) - f32(0.5)
            if where == "in":
                c = np.nextafter(c, f32(-np.inf))
        else:
            c = f32((3355 if where == "out" else 3356) * 2.0 ** -25) - f32(0.5)
        cx, cy = (float(c), 0.125) if axis == "u" else (0.125, float(c))
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    gray = (0.25 + 0.0625 * ((i + 2 * j) % 8)).astype(f32)
    rgb = np.stack([16 * ((i + j) % 16), 255 - 32 * (j % 8), 8 * (i % 32)], -1).astype(np.uint8)
    return dict(w=w, h=h, depth=np.full((h, w), 0.375, f32), rgb=np.ascontiguousarray(rgb), gray=np.ascontiguousarray(gray),
                extrinsic=np.eye(4), intrinsic=np.array([4.0, 2.0, cx, cy]), length=1.25, R=5, sdf_trunc=0.75,
                origin=(-0.625, -0.625, -0.375))


EDGE_CASES = ("1x1", "7x1", "1x7", "u_hi_out", "u_hi_in", "u_lo_out", "u_lo_in", "v_hi_out", "v_hi_in", "v_lo_out", "v_lo_in")
