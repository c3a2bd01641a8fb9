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


# ---------------------------------------------------------------------------
# hostile cases (tests/test_colormap_hostile.py, tests/golden/gen_rgbd_hostile.py): exact numbers.  32 x 24 images, fx = fy =
# 16, the principal point (16, 12), cameras without rotation, vertices on the plane z = 1: a vertex (X, Y, 1) projects to
# u = 16 X + 16, v = 16 Y + 12 without a rounding in fp32 and in f64, and a camera moved by 1 / 16 sees it one pixel further.
# The 10-pixel margin leaves u in [10, 22), v in [10, 14).
# ---------------------------------------------------------------------------
HW, HH = 32, 24
HK = np.array([16.0, 16.0, 16.0, 12.0])


def at_pixel(u, v, z=1.0):
    """the vertex that projects to (u, v) under HK from the identity"""
    return np.array([(u - 16.0) / 16.0 * z, (v - 12.0) / 16.0 * z, z])


def shifted(du=0.0, dv=0.0):
    """world -> camera of a camera that sees every vertex of the plane z = 1 (du, dv) pixels further"""
    E = np.eye(4)
    E[0, 3], E[1, 3] = du / 16.0, dv / 16.0
    return E


def pattern(du=0.0, dv=0.0, w=HW, h=HH):
    """the RGB8 image of a smooth texture painted on the plane z = 1, as a camera (du, dv) pixels further sees it"""
    v, u = np.meshgrid(np.arange(h, dtype=np.float64) - dv, np.arange(w, dtype=np.float64) - du, indexing="ij")
    g = 0.5 + 0.25 * np.sin(0.45 * u + 0.3) * np.cos(0.35 * v) + 0.2 * np.sin(0.3 * v + 0.15 * u)
    rgb = np.stack([g, 1.0 - 0.8 * g, 0.5 + 0.4 * np.sin(0.5 * v + 0.2 * u)], -1)
    return np.ascontiguousarray(np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8))


def pose_error(c):
    """how far (pixels) camera c's image is from where its extrinsic says: what the optimisation has to find"""
    return 0.12 * ((c * 5) % 7 - 3) / 3.0, 0.1 * ((c * 3) % 5 - 2) / 2.0


def boundary_case():
    """VERTICES ON THE DECISIONS.  Two cameras (the identity; one pixel further in u), depth 1 everywhere but for three
    pixels of camera 0: NaN at (13, 12), +inf at (13, 18), -1 at (11, 19) (v, u).  Vertices, in this order:
      0 .. 47     a grid, one per pixel of the inside region, at (u + 0.25, v + 0.25): three of them land on the bad pixels
      48 .. 59    u == 10, one fp32 ulp below, one above (v = 12); the same at u == 22; at v == 10 and v == 14 (u = 16)
      60, 61      u = 10 - 2^-40 and u = 22 - 2^-40: fp32 rounds them to 10 and 22, so the proxy (fp32) and the iteration
                  (f64) decide differently
      62 .. 65    a NaN coordinate, an inf coordinate, the camera centre (z == 0), behind the camera
    -> depths, colors, extrinsics, intrinsic, vertices, option overrides"""
    f32 = np.float32
    depths = np.ones((2, HH, HW), np.float32)
    depths[0, 13, 12], depths[0, 13, 18], depths[0, 11, 19] = np.nan, np.inf, -1.0
    colors = np.stack([pattern(0.0 + pose_error(0)[0], pose_error(0)[1]), pattern(1.0 + pose_error(1)[0], pose_error(1)[1])])
    V = [at_pixel(10.25 + i, 10.25 + j) for j in range(4) for i in range(12)]
    for edge, axis in ((10.0, 0), (22.0, 0), (10.0, 1), (14.0, 1)):
        for val in (f32(edge), np.nextafter(f32(edge), f32(0)), np.nextafter(f32(edge), f32(100))):
            V.append(at_pixel(float(val), 12.0) if axis == 0 else at_pixel(16.0, float(val)))
    V += [at_pixel(10.0 - 2.0 ** -40, 12.5), at_pixel(22.0 - 2.0 ** -40, 12.5)]
    V += [np.array([np.nan, 0.0, 1.0]), np.array([np.inf, 0.0, 1.0]), np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.0])]
    return depths, colors, np.stack([shifted(), shifted(1.0)]), HK.copy(), np.ascontiguousarray(np.stack(V)), dict(half_dilation_kernel_size_for_discontinuity_map=0)


KEEP_NORMAL = 2                                                        # cameras 0, 1: ordinary
KEEP_CONSTANT = KEEP_NORMAL + 6                                        # cameras 2 .. 7 see 1 .. 6 vertices; camera 8 has constant images


def keep_pose_case(degenerate=True):
    """CAMERAS THAT MUST KEEP THEIR POSE.  Vertices 0 .. 71 lie left of u = 16.5 (four per pixel of 6 x 3 pixels) and are all
    that cameras 0 and 1 (one pixel further in v) have depths for; vertices 72 .. 91, one per pixel of u = 17 .. 21, are seen
    by the other cameras only: camera 2 + k has a depth on the pixels of the first 1 + k of them (k = 0 .. 5: 1 .. 5 accepted
    vertices, and exactly 6), camera 8 on the last ten, under a CONSTANT colour image (zero gradients: a singular system).
    No depth edge counts (the discontinuity threshold is 10).  degenerate=False: cameras 0 and 1 alone, the same vertices.
    -> depths, colors, extrinsics, intrinsic, vertices, option overrides"""
    V = [at_pixel(10 + i + dx, 10 + j + dy) for j in range(3) for i in range(6) for dx in (0.2, 0.45) for dy in (0.15, 0.4)]
    V += [at_pixel(17.25 + i, 10.25 + j) for j in range(4) for i in range(5)]
    V = np.ascontiguousarray(np.stack(V))
    n = KEEP_CONSTANT + 1 if degenerate else KEEP_NORMAL
    depths = np.zeros((n, HH, HW), np.float32)
    depths[:KEEP_NORMAL, :, :17] = 1.0
    colors = np.stack([pattern(pose_error(c)[0], (1.0 if c == 1 else 0.0) + pose_error(c)[1]) for c in range(n)])
    E = np.stack([shifted(0.0, 1.0) if c == 1 else shifted() for c in range(n)])
    if degenerate:
        right = V[len(V) - 20:]
        px = np.rint(right[:, :2] * 16.0 + HK[2:] - 0.25).astype(int)        # (u, v) of their pixels
        for k in range(6):
            for u, v in px[:k + 1]:
                depths[KEEP_NORMAL + k, v, u] = 1.0
        for u, v in px[10:]:
            depths[KEEP_CONSTANT, v, u] = 1.0
        colors[KEEP_CONSTANT] = 128
    return depths, colors, E, HK.copy(), V, dict(depth_threshold_for_discontinuity_check=10.0)


def seam_case(n_vertices=40, n_cameras=2, half_dilation=3):
    """21 x 21 images, the smallest there are: the inside region is the one pixel (10, 10).  Cameras without rotation,
    camera c moved by (c % 5 - 2, c // 5 % 5 - 2) sixteenths of a pixel; depth 1 but for a step to 1.5 right of column 15 (the
    dilation cases' edge); vertices on z = 1 on a spiral around the pixel (10, 10), about a third of them inside.
    -> depths, colors, extrinsics, intrinsic, vertices, option overrides"""
    w = h = 21
    K = np.array([16.0, 16.0, 10.0, 10.0])
    depths = np.ones((n_cameras, h, w), np.float32)
    depths[:, :, 16:] = 1.5
    shift = [((c % 5 - 2) / 16.0, (c // 5 % 5 - 2) / 16.0) for c in range(n_cameras)]
    colors = np.stack([pattern(du + pose_error(c)[0], dv + pose_error(c)[1], w, h) for c, (du, dv) in enumerate(shift)])
    E = np.stack([shifted(du, dv) for du, dv in shift])
    i = np.arange(n_vertices)
    r, a = 0.02 + 0.9 * ((i * 7) % 64) / 64.0, 2.399963 * i
    uv = np.stack([10.4 + r * np.cos(a), 10.4 + r * np.sin(a)], 1)
    V = np.ascontiguousarray(np.column_stack([(uv[:, 0] - 10.0) / 16.0, (uv[:, 1] - 10.0) / 16.0, np.ones(n_vertices)]))
    return depths, colors, E, K, V, dict(half_dilation_kernel_size_for_discontinuity_map=half_dilation)
