"""The reference's image front end on the stand-alone header set (include/Core/Geometry/Image.h, RGBDImage.h):
tests/cpp/image_driver.cpp calls CreateFloatImageFromImage, ConvertDepthToFloatImage, CreateImageFromFloatImage<T>, FilterImage
(both forms), FilterHorizontalImage, FlipImage, DownsampleImage, DilateImage, LinearTransformImage, ClipIntensityImage,
CreateImagePyramid, FilterImagePyramid, CreateDepthToCameraDistanceMultiplierFloatImage, Image::FloatValueAt /
TestImageBoundary, the five CreateRGBDImageFrom* factories and the two RGB-D pyramid functions with the reference's names and
signatures, compiled in both Eigen storage orders.  On cases of tests/image_cases.py its images equal the specification's bit
for bit (tests/test_image_spec.py pins that to the compiled reference; tests/test_image.py the Python route to it).  Also: a
chain on cicp::DeviceImage gives the Python route's bytes, and TSDFVolume::Integrate of DeviceImages the volume of the
host-array route."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import image_cases as cases
import image_spec as S
import tsdf_scene

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_image  # noqa: E402

ITEMS = ("shape_65x33", "shape_5x2", "shape_1x1", "values", "convert_3x1", "convert_2x2", "convert_1x4", "depth_trunc", "from_float", "rgbd",
         "dilate_65x33", "value_at", "pyramid", "multiplier", "front_end", "from_float_saturated", "nyu_saturated", "value_at_undefined")
ROWMAJOR_ITEMS = ("shape_33x65", "rgbd", "pyramid")


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_image.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_image.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("image driver not prebuilt and no Eigen headers here")
    return paths


def test_shim_compiles(lib):
    """the header set and the driver compile (both Eigen storage orders) wherever Eigen's headers are"""
    if build_shim.eigen_dir() is None:
        pytest.skip("no Eigen headers here")
    outs = build_image.build()
    assert outs and all(os.path.exists(p) for p in outs)


def drive(exe, mode, payload, tmp_path):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(payload)
    p = subprocess.run([exe, mode, inp, outp], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-400:])
    return open(outp, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", [(n, 0) for n in ITEMS] + [(n, 1) for n in ROWMAJOR_ITEMS])
def test_the_reference_names_give_the_specification(driver_bins, tmp_path, name, which):
    got = cases.decode(drive(driver_bins[which], "cases", cases.encode(*cases.case(name)), tmp_path))
    cases.same(got, cases.spec(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("which", (0, 1))
def test_a_device_image_chain_gives_the_python_routes_bytes(lib, driver_bins, tmp_path, which):
    (color, depth), _ = cases.case("front_end")
    got, _ = cases.decode(drive(driver_bins[which], "chain", cases.encode_image(color) + cases.encode_image(depth), tmp_path))
    ctx = lib.Context(0)
    try:
        want = []
        with ctx.image(color) as c, ctx.image(depth) as d:
            gray, metres = ctx.rgbd(c, d, "tum")
            for level in gray.pyramid(3, True):
                g = level.filter("gaussian5")
                g.linear_transform(4.0, -1.5); g.clip_intensity(0.0, 1.0)
                want.append(g.from_float(1).get())
            want.append(metres.get())
            cp, dp = gray.pyramid(2, True), metres.pyramid(2, False)
            for a, b in zip(ctx.filter_pyramid(cp, "gaussian3"), ctx.filter_pyramid(dp, "gaussian3")):
                want += [a.get(), b.get()]
    finally:
        ctx.close()
    assert len(got) == len(want) == 8
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    # ... which are the specification's
    regs, _ = cases.spec("front_end")
    assert cases.bits(got[0]).tobytes() == cases.bits(regs[16]).tobytes() and cases.bits(got[3]).tobytes() == cases.bits(regs[3]).tobytes()
    assert got[0].dtype == np.uint8 and got[0].min() == 0 and got[0].max() == 255


@pytest.mark.gpu
def test_integrate_of_device_images_gives_the_host_array_routes_volume(lib, driver_bins, tmp_path):
    frames, k = tsdf_scene.frames(64, 48, 1)
    depth, rgb, gray, E = frames[0]
    payload = cases.encode_image(depth) + cases.encode_image(rgb) + struct.pack("<20d", *(list(k) + list(np.asarray(E).reshape(-1))))
    raw = drive(driver_bins[0], "integrate", payload, tmp_path)
    n = int(np.frombuffer(raw[:4], "<i4")[0])
    assert n == 32 ** 3
    tsdf, weight = np.frombuffer(raw[4:4 + 4 * n], np.float32), np.frombuffer(raw[4 + 4 * n:4 + 8 * n], np.float32)
    at = 4 + 8 * n
    npts = int(np.frombuffer(raw[at:at + 4], "<i4")[0])
    points = np.frombuffer(raw[at + 4:], "<f8").reshape(npts, 3)
    ctx = lib.Context(0)
    try:
        vol = ctx.tsdf_uniform(2.0, 32, 0.1, lib.TSDF_COLOR_RGB8, origin=(-1.0, -1.0, -1.0))
        vol.integrate(depth, rgb, k, E)
        want_tsdf, want_weight, _ = vol.volume()
        sc = ctx.tsdf_scalable(2.0 / 32, 0.1, lib.TSDF_COLOR_RGB8, volume_unit_resolution=8, depth_sampling_stride=4)
        sc.integrate(depth, rgb, k, E)
        want_points = sc.extract_point_cloud()[0]
    finally:
        ctx.close()
    assert weight.any() and tsdf.tobytes() == want_tsdf.tobytes() and weight.tobytes() == want_weight.tobytes()
    assert npts > 100 and points.tobytes() == np.ascontiguousarray(want_points).tobytes()
