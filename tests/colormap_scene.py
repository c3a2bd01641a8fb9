"""The scene of the color map tests: RGB-D frames of a textured analytic scene from six cameras whose extrinsics are a
little wrong, and vertices sampled on its surfaces.

  scene     the two tilted planes and the sphere of tests/tsdf_scene.py's kind: a floor n . p = 0.5 with n = (0.2, 1, 0.1),
            a back wall n . p = 0.55 with n = (0.15, -0.1, 1), a sphere of radius 0.33 at (0.05, -0.05, 0.0)
  texture   0.5 + 0.22 sin(5x + 1) cos(4y) + 0.2 sin(6z + 3x + 2y) of the world point: smooth, with a gradient everywhere
            at the 2 cm a pixel covers; RGB8 = (g, 1 - 0.8 g, 0.5 + 0.4 sin(6y + 2x)) * 255, rounded
  pinhole   83 x 61 (both odd: no 4- or 16-pixel alignment holds; the 10-pixel margin leaves 63 x 41), fx = fy = 0.9 w
  cameras   six, camera_to_world(i): five look at the scene from z about -1.1; the LAST is turned so far to the side that it
            sees a sliver of the wall only (under 5 % of the vertices).  extrinsic(i) is the TRUE world -> camera;
            perturbed(i) is what the optimisation is given: the true one times a rotation of about 0.3 degrees and a
            translation of about 3 mm
  vertices  on the wall, the floor and the whole sphere (its far side is seen by no camera), and one behind every camera
  holes     a block of depth-0 pixels per frame; the sphere's silhouette is a depth edge; with the tests' option
            (maximum_allowable_depth 1.8) the far part of the wall is too deep

Depth is the z coordinate in the camera's frame, fp32, h x w in C order."""
import numpy as np

from tsdf_scene import rigid

W, H = 83, 61
N_CAMERAS = 6
PLANES = (((0.2, 1.0, 0.1), 0.5), ((0.15, -0.1, 1.0), 0.55))
SPHERE = ((0.05, -0.05, 0.0), 0.33)
_POSES = (((0.05, -0.10, 0.02), (0.25, 0.10, -1.15)), ((-0.06, 0.22, -0.03), (-0.45, 0.05, -1.05)),
          ((0.12, -0.25, 0.05), (0.50, -0.20, -1.0)), ((0.03, 0.08, -0.04), (-0.10, 0.02, -1.2)),
          ((-0.08, -0.05, 0.03), (0.05, -0.25, -1.1)), ((0.02, 0.6, 0.0), (-0.2, 0.0, -1.1)))
# per camera: a rotation vector of about 0.3 degrees (0.0052 rad) and a translation of about 3 mm
_ERRORS = (((0.004, -0.003, 0.002), (0.002, -0.002, 0.001)), ((-0.003, 0.004, -0.001), (-0.002, 0.001, 0.002)),
           ((0.002, 0.003, 0.004), (0.001, 0.002, -0.002)), ((-0.004, -0.002, 0.003), (0.002, 0.002, 0.001)),
           ((0.003, -0.004, -0.002), (-0.001, -0.002, 0.002)), ((0.002, 0.002, -0.003), (0.002, -0.001, -0.002)))
MAX_DEPTH = 1.8                                                       # the tests' maximum_allowable_depth


def camera_to_world(i):
    return rigid(*_POSES[i])


def invert_rigid(C):
    """R^T, -R^T t written out"""
    E = np.eye(4)
    E[:3, :3] = C[:3, :3].T
    E[:3, 3] = -C[:3, :3].T @ C[:3, 3]
    return E


def extrinsic(i):
    return invert_rigid(camera_to_world(i))


def perturbed(i):
    return rigid(*_ERRORS[i]) @ extrinsic(i)


def intrinsic(w=W, h=H):
    """fx, fy, cx, cy"""
    return np.array([0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0])


def texture(P):
    return 0.5 + 0.22 * np.sin(5 * P[..., 0] + 1) * np.cos(4 * P[..., 1]) + 0.2 * np.sin(6 * P[..., 2] + 3 * P[..., 0] + 2 * P[..., 1])


def render_from(C, i=0, w=W, h=H):
    """-> depth (h x w fp32), rgb (h x w x 3 uint8) of a camera with pose C (camera -> world); i places the depth-0 block"""
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
    rgb = np.stack([g, 1.0 - 0.8 * g, 0.5 + 0.4 * np.sin(6 * P[..., 1] + 2 * P[..., 0])], -1)
    rgb[~hit] = 0.0
    depth = z.astype(np.float32)                                       # (the ray has z = 1: its parameter is the depth)
    y0, x0 = int(round((0.2 + 0.1 * i) * h)), int(round((0.75 - 0.1 * i) * w))
    depth[y0:y0 + 4, x0:x0 + 5] = 0.0
    return np.ascontiguousarray(depth), np.ascontiguousarray(np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8))


def render(i, w=W, h=H):
    return render_from(camera_to_world(i), i, w, h)


def vertices(n_wall=2000, n_floor=500, n_sphere=700, seed=5):
    """n x 3 f64: the wall, the floor, the whole sphere, and one point behind every camera (the last row)"""
    rng = np.random.default_rng(seed)
    out = []
    (nf, cf), (nw, cw) = PLANES
    xy = rng.uniform((-1.3, -0.75), (1.3, 0.45), (n_wall, 2))
    out.append(np.column_stack([xy, (cw - nw[0] * xy[:, 0] - nw[1] * xy[:, 1]) / nw[2]]))
    xz = rng.uniform((-1.0, -0.7), (1.0, 0.45), (n_floor, 2))
    out.append(np.column_stack([xz[:, 0], (cf - nf[0] * xz[:, 0] - nf[2] * xz[:, 1]) / nf[1], xz[:, 1]]))
    s = rng.normal(size=(n_sphere, 3))
    out.append(np.array(SPHERE[0]) + SPHERE[1] * s / np.linalg.norm(s, axis=1, keepdims=True))
    out.append(np.array([[0.05, -0.05, -1.7]]))
    return np.ascontiguousarray(np.vstack(out))


def frames(n=N_CAMERAS):
    """-> depths (n x H x W fp32), colors (n x H x W x 3 uint8), the PERTURBED extrinsics (n x 4 x 4), intrinsic"""
    r = [render(i) for i in range(n)]
    return (np.stack([d for d, _ in r]), np.stack([c for _, c in r]), np.stack([perturbed(i) for i in range(n)]), intrinsic())


def turned_away():
    """a camera that looks away from the scene (it sees a stretch of floor no vertex lies on, and the one vertex in front of
    it projects onto a pixel without depth): depth, colour and its extrinsic"""
    C = rigid((0.0, np.pi, 0.0), (0.0, 0.0, -1.2))
    d, c = render_from(C, 0)
    return d, c, invert_rigid(C)
