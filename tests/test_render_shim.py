"""feh::gpu::Renderer (include/visma_geometry.hpp) with the reference's members, and the resident chain volume -> mesh ->
cicp::RenderDepth -> Integrate, through tests/cpp/render_driver.cpp compiled in both Eigen storage orders: the images are
render_host's for the camera point pose * model * X, bit for bit; LinearizeDepth inverts what RenderDepth delivers; the chain
gives the Python route's bytes."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import render_cases as cases
import render_spec as S
import tsdf_scene

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_render  # noqa: E402


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_render.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_render.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("render driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_render.build()
    assert outs and all(os.path.exists(p) for p in outs)


def drive(exe, mode, payload, tmp_path):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(payload)
    p = subprocess.run([exe, mode, inp, outp], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-400:])
    return open(outp, "rb").read()


def doubles(*parts):
    flat = np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in parts])
    return struct.pack("<%dd" % len(flat), *flat)


@pytest.mark.gpu
@pytest.mark.parametrize("which,form", ((0, 0), (0, 1), (1, 2)))
def test_the_renderer_of_the_reference_names(lib, driver_bins, tmp_path, which, form):
    c = cases.CASES["sphere_close_64x48"]
    w, h = c["w"], c["h"]
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)          # the reference's members take floats
    V, K = f32(c["V"]), f32(c["K"])
    zn, zf = f32(0.05), f32(10.0)
    pose, model = f32(cases.pose((0.02, -0.01, 0.3), (0.0, 1.0, 0.2), 0.2)), f32(c["E"])
    payload = doubles([form, len(V)], V, [len(c["F"])], c["F"], [w, h], K, [zn, zf], pose, model)
    raw = drive(driver_bins[which], "renderer", payload, tmp_path)
    px = w * h
    depth = np.frombuffer(raw[:4 * px], np.float32).reshape(h, w)
    mask = np.frombuffer(raw[4 * px:5 * px], np.uint8).reshape(h, w)
    edge = np.frombuffer(raw[5 * px:6 * px], np.uint8).reshape(h, w)
    metres = np.frombuffer(raw[6 * px:], np.float32).reshape(h, w)
    E = np.zeros((4, 4))                                     # pose * model, each entry summed left to right in f64
    for i in range(4):
        for j in range(4):
            a = 0.0
            for l in range(4):
                a += pose[i, l] * model[l, j]
            E[i, j] = a
    want_zb = lib.render_host(V, c["F"], w, h, K, E, zn, zf, "depth_buffer")
    want = lib.render_host(V, c["F"], w, h, K, E, zn, zf)
    assert depth.tobytes() == want_zb[0].tobytes() and mask.tobytes() == want[2].tobytes() and edge.tobytes() == want[3].tobytes()
    assert (mask == 255).sum() > 500 and edge.any()
    # LinearizeDepth inverts RenderDepth's encoding (to what fp32 keeps of it), and the background is the far plane
    back = np.array([lib.linearize_depth(float(z), zn, zf) for z in depth.reshape(-1)]).astype(np.float32).reshape(h, w)
    assert metres.tobytes() == back.tobytes()
    on = mask == 255
    z = want[0][on].astype(np.float64)
    assert np.all(np.abs(metres[on] - z) <= 2.0 ** -23 * z * z * (zf - zn) / (2 * zn * zf) + 1e-6 * z)
    assert np.all(np.abs(metres[~on] - zf) <= 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("which", (0, 1))
def test_the_resident_chain_gives_the_python_routes_bytes(lib, driver_bins, tmp_path, which):
    frames, k = tsdf_scene.frames(64, 48, 1)
    depth, rgb, gray, E = frames[0]
    payload = doubles([64, 48]) + np.ascontiguousarray(depth, np.float32).tobytes() + doubles(k, E)
    raw = drive(driver_bins[which], "chain", payload, tmp_path)
    got, at = [], 0
    for dtype in (np.float32, np.int32, np.uint8, np.uint8):
        w, h, ch, bpc = np.frombuffer(raw[at:at + 16], "<i4")
        assert (w, h, ch, bpc) == (64, 48, 1, np.dtype(dtype).itemsize)
        got.append(np.frombuffer(raw[at + 16:at + 16 + w * h * bpc], dtype).reshape(h, w))
        at += 16 + w * h * bpc
    n = int(np.frombuffer(raw[at:at + 4], "<i4")[0])
    assert n == 32 ** 3
    tsdf, weight = np.frombuffer(raw[at + 4:at + 4 + 4 * n], np.float32), np.frombuffer(raw[at + 4 + 4 * n:at + 4 + 8 * n], np.float32)
    ctx = lib.Context(0)
    try:
        vol = ctx.tsdf_uniform(2.0, 32, 0.1, lib.TSDF_COLOR_NONE, origin=(-1.0, -1.0, -1.0))
        vol.integrate(depth, None, k, E)
        vol.extract_triangle_mesh()
        mesh = vol.triangle_mesh()
        d, i, m = mesh.render(64, 48, k, E)
        e = ctx.render_edges(d)
        want = [x.get() for x in (d, i, m, e)]
        second = ctx.tsdf_uniform(2.0, 32, 0.1, lib.TSDF_COLOR_NONE, origin=(-1.0, -1.0, -1.0))
        second.integrate(d, None, k, E)
        want_tsdf, want_weight, _ = second.volume()
    finally:
        ctx.close()
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert (got[2] == 255).sum() > 300 and weight.any()
    assert tsdf.tobytes() == want_tsdf.tobytes() and weight.tobytes() == want_weight.tobytes()
