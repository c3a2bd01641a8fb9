"""The inputs of the ExtractTriangleMesh tests: what tests/golden/gen_tsdf_mesh.py feeds the compiled reference and what
the tests feed the specification and the library.  load(name) -> a dict; spec_volume(case) integrates it with tests/tsdf_spec.py
(bit for bit the reference's volume: the generator asserts it).  The scene frames are those stored in tests/golden/tsdf.npz."""
import os

import numpy as np

import tsdf_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("u21", "u32", "u67", "s0", "s1", "s2", "s5", "sp5", "sp8", "plane", "ambig")
# the cases without a valid cube that has a diagonally signed face: compared with the reference in full.  The scene's depth
# discontinuities (the sphere's silhouette, the holes) leave such cubes in every other case (counted by the generator: 9 in
# u32 up to 114 in s1), so those are compared as "ambig" is: the vertices bit for bit, the mesh an oriented manifold.
UNAMBIGUOUS = ("u21", "sp5", "sp8", "plane")
AMBIGUOUS = tuple(n for n in NAMES if n not in UNAMBIGUOUS)
_UNIFORM = {"u21": (21, S.COLOR_RGB8), "u32": (32, S.COLOR_GRAY32), "u67": (67, S.COLOR_NONE)}
_golden = None


def _tsdf_golden():
    global _golden
    if _golden is None:
        g = np.load(os.path.join(HERE, "golden", "tsdf.npz"))
        _golden = {k: g[k] for k in g.files}
    return _golden


def _scene_frames(n):
    g = _tsdf_golden()
    return [(g["f%d_depth" % i], g["f%d_rgb" % i], g["f%d_gray" % i], g["f%d_extrinsic" % i]) for i in range(n)]


def _paint(depth):
    """colour images for a made-up depth frame, in exactly representable numbers"""
    h, w = depth.shape
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    gray = (0.25 + 0.0625 * ((i + 2 * j) % 8)).astype(np.float32)
    rgb = np.stack([16 * ((i + j) % 16), 255 - 32 * (j % 8), 8 * (i % 32)], -1).astype(np.uint8)
    return np.ascontiguousarray(rgb), np.ascontiguousarray(gray)


def load(name):
    g = _tsdf_golden()
    if name in _UNIFORM:
        R, t = _UNIFORM[name]
        length = float(g["length"])
        return dict(name=name, scalable=False, R=R, color_type=t, length=length, voxel_length=length / R,
                    sdf_trunc=float(g["u%d_sdf_trunc" % R]), origin=tuple(float(v) for v in g["origin"]),
                    frames=_scene_frames(4), intrinsic=g["intrinsic"])
    if name in ("s0", "s1", "s2"):
        R, stride, vl, trunc, t, nf = g[name + "_config"]
        return dict(name=name, scalable=True, R=int(R), stride=int(stride), voxel_length=float(vl), sdf_trunc=float(trunc),
                    color_type=int(t), frames=_scene_frames(int(nf)), intrinsic=g["intrinsic"])
    if name == "s5":
        return dict(name=name, scalable=True, R=5, stride=4, voxel_length=0.04, sdf_trunc=0.12, color_type=S.COLOR_RGB8,
                    frames=_scene_frames(2), intrinsic=g["intrinsic"])
    if name in ("sp5", "sp8"):
        # a smooth slanted surface: no discontinuity, so no ambiguous cube (and no tsdf of exactly 0); it crosses unit
        # borders on every axis, with negative unit indices, and its rim has missing neighbour units
        i, j = np.meshgrid(np.arange(18), np.arange(24), indexing="ij")
        depth = (1.003 + 0.0131 * j + 0.0293 * i).astype(np.float32)
        rgb, gray = _paint(depth)
        return dict(name=name, scalable=True, R=int(name[2:]), stride=2, voxel_length=0.05, sdf_trunc=0.15, color_type=S.COLOR_RGB8,
                    frames=[(depth, rgb, gray, np.eye(4))], intrinsic=np.array([20.0, 20.0, 11.5, 8.5]))
    if name == "plane":
        depth = np.full((17, 17), 0.5, np.float32)
        depth[:, :8] = 0.25
        rgb, gray = _paint(depth)
        return dict(name=name, scalable=False, R=5, color_type=S.COLOR_RGB8, length=1.25, voxel_length=0.25, sdf_trunc=0.75,
                    origin=(-0.625, -0.625, -0.375), frames=[(depth, rgb, gray, np.eye(4))], intrinsic=np.array([4.0, 4.0, 8.0, 8.0]))
    if name == "ambig":
        i, j = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
        depth = np.where((i + j) % 2 == 0, 1.2, 1.4).astype(np.float32)
        rgb, gray = _paint(depth)
        return dict(name=name, scalable=False, R=16, color_type=S.COLOR_GRAY32, length=1.6, voxel_length=0.1, sdf_trunc=0.3,
                    origin=(-0.8, -0.8, 0.5), frames=[(depth, rgb, gray, np.eye(4))], intrinsic=np.array([13.0, 13.0, 7.5, 7.5]))
    raise KeyError(name)


def color_of(case, frame):
    return {S.COLOR_NONE: None, S.COLOR_RGB8: frame[1], S.COLOR_GRAY32: frame[2]}[case["color_type"]]


def spec_volume(case):
    """the case's volume as tests/tsdf_spec.py integrates it"""
    if case["scalable"]:
        vol = S.new_scalable(case["voxel_length"], case["sdf_trunc"], case["color_type"], case["R"], case["stride"])
        for fr in case["frames"]:
            S.scalable_integrate(vol, fr[0], color_of(case, fr), case["intrinsic"], fr[3])
    else:
        vol = S.new_volume(case["length"], case["R"], case["sdf_trunc"], case["color_type"], case["origin"])
        for fr in case["frames"]:
            S.integrate(vol, fr[0], color_of(case, fr), case["intrinsic"], fr[3])
    return vol


def lib_volume(ctx, case, **kw):
    """the case's volume on the device (a visma_amd TsdfVolume), integrated"""
    if case["scalable"]:
        vol = ctx.tsdf_scalable(case["voxel_length"], case["sdf_trunc"], case["color_type"], case["R"], case["stride"], **kw)
    else:
        vol = ctx.tsdf_uniform(case["length"], case["R"], case["sdf_trunc"], case["color_type"], case["origin"])
    for fr in case["frames"]:
        vol.integrate(fr[0], color_of(case, fr), case["intrinsic"], fr[3])
    return vol
