"""The scenes of the non-rigid color map tests: tests/colormap_scene.py's (83 x 61, six cameras, 3,201 vertices), and a DISTORTED
copy of it: every colour image resampled through a smooth field of about 2 pixels that no rigid pose explains (the depth
images, the vertices and the extrinsics stay).  A rigid optimisation is left with the field as residual; a warping field
per image absorbs it.

  field     camera c's pixel (u, v) shows what the undistorted image has at
            (u + 2 sin(2 pi v / 61 + 0.7 c) cos(pi u / 83), v + 1.6 sin(2 pi u / 83 + 0.4 c + 1) cos(pi v / 61)):
            a wave of one period over the image: a barrel-like bend, opposite at opposite borders
  resample  bilinear in f64 on the RGB8 values (coordinates clamped to the image), rounded to uint8"""
import numpy as np

import colormap_scene as scene

W, H, N_CAMERAS = scene.W, scene.H, scene.N_CAMERAS


def field(c, w=W, h=H):
    """-> du, dv (h x w)"""
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return (2.0 * np.sin(2 * np.pi * v / h + 0.7 * c) * np.cos(np.pi * u / w),
            1.6 * np.sin(2 * np.pi * u / w + 0.4 * c + 1.0) * np.cos(np.pi * v / h))


def resample(rgb, du, dv):
    h, w = rgb.shape[:2]
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y = np.clip(u + du, 0, w - 1), np.clip(v + dv, 0, h - 1)
    x0, y0 = np.minimum(x.astype(int), w - 2), np.minimum(y.astype(int), h - 2)
    a, b = (x - x0)[..., None], (y - y0)[..., None]
    f = rgb.astype(np.float64)
    out = (f[y0, x0] * (1 - a) + f[y0, x0 + 1] * a) * (1 - b) + (f[y0 + 1, x0] * (1 - a) + f[y0 + 1, x0 + 1] * a) * b
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def frames():
    """colormap_scene.frames() as it is"""
    return scene.frames()


def distorted_frames():
    """-> depths, colors (resampled), the perturbed extrinsics, intrinsic"""
    depths, colors, E, K = scene.frames()
    return depths, np.stack([resample(colors[c], *field(c)) for c in range(len(colors))]), E, K


def vertices():
    return scene.vertices()
