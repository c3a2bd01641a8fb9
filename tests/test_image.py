"""The Image operations on the GPU (visma_icp_image_*; image.hip) against the numpy specification tests/image_spec.py, which
tests/test_image_spec.py pins to the compiled reference: every case of tests/image_cases.py (the stated deviations included),
format, shape and bits.  Empty results and error codes exactly; two runs byte for byte; and every hand-off of a resident image
(TSDF integration, RGB-D odometry, the odometry pyramid's levels) against its host-array entry point on the same pixels, byte
for byte."""
import ctypes as C

import numpy as np
import pytest

import image_cases as cases
import image_spec as S
import odometry_scene
import odometry_spec
import tsdf_scene

INVALID, STATE = 1, 5


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


class LibOps:
    """tests/image_cases.py's operations over the library: a register is an Image"""

    def __init__(self, ctx):
        self.ctx = ctx

    def upload(self, a): return self.ctx.image(a)
    def close(self, r): r.close()
    def empty(self): return self.ctx.image(np.zeros((0, 0), np.uint8)).filter_horizontal([1.0])     # (not 1 x float: the empty image)

    def download(self, r):
        a = r.get()
        if r.info() == (0, 0, 0, 0):
            assert a.size == 0
            return S.EMPTY
        assert S.info(a) == r.info(), (S.info(a), r.info())
        return a

    def to_float(self, r, t): return r.to_float(t)
    def depth_to_float(self, r, s, t): return r.depth_to_float(s, t)
    def from_float(self, r, b): return r.from_float(b)
    def filter(self, r, t): return r.filter(t)
    def filter_separable(self, r, dx, dy): return r.filter_separable(dx, dy)
    def filter_horizontal(self, r, k): return r.filter_horizontal(k)
    def flip(self, r): return r.flip()
    def downsample(self, r): return r.downsample()
    def dilate(self, r, k): return r.dilate(k)
    def copy(self, r): return r.copy()
    def linear_transform(self, r, s, o): r.linear_transform(s, o)
    def clip_intensity(self, r, lo, hi): r.clip_intensity(lo, hi)
    def pyramid(self, r, n, g): return r.pyramid(n, g)
    def filter_pyramid(self, rs, t): return self.ctx.filter_pyramid(rs, t)
    def distance_multiplier(self, k, w, h): return self.ctx.distance_multiplier(k, w, h)
    def float_value_at(self, r, uv): return r.float_value_at(uv)
    def rgbd(self, c, d, fmt, s, t, conv): return self.ctx.rgbd(c, d, fmt, s, t, conv)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES + cases.SPEC_ONLY)
def test_a_case_equals_the_specification(lib, ctx, name):
    got = cases.run(LibOps(ctx), *cases.case(name))
    print("%s: %d registers, %d results" % (name, len(got[0]), len(got[1])))
    cases.same(got, cases.spec(name), name)


@pytest.mark.gpu
def test_two_runs_are_bit_identical(lib, ctx):
    for name in ("shape_130x67", "shape_65x33", "values", "pyramid", "front_end", "dilate_65x33"):
        a, ra = cases.run(LibOps(ctx), *cases.case(name))
        b, rb = cases.run(LibOps(ctx), *cases.case(name))
        assert ra.tobytes() == rb.tobytes(), name
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b], name


def code(lib, call):
    with pytest.raises(lib.IcpError) as e:
        call()
    return e.value.code


@pytest.mark.gpu
def test_empty_results_and_error_codes(lib, ctx):
    L, h = ctx.L, ctx._h
    f = ctx.image(np.ones((3, 4), np.float32))
    b = ctx.image(np.ones((3, 4), np.uint8))
    rgb = ctx.image(np.ones((3, 4, 3), np.float32))
    # the empty image, exactly: 0 x 0, no channels, no bytes
    for img in (b.filter(0), b.filter_horizontal([1.0]), f.filter_horizontal([0.5, 0.5]), f.filter_horizontal([]), b.flip(), b.downsample(),
                rgb.filter_separable([1.0], [1.0]), f.dilate(1), b.from_float(1), rgb.from_float(2)):
        assert img.info() == (0, 0, 0, 0) and img.get().size == 0
        assert img.to_float().info() == (0, 0, 0, 0)         # IsEmpty(): the empty image again
    assert b.pyramid(3) == [] and rgb.pyramid(2, False) == []
    # in place on an unsupported format: untouched, and no error
    before = b.get().tobytes()
    b.linear_transform(2.0, 1.0); b.clip_intensity(0.0, 0.5)
    assert b.get().tobytes() == before
    # an image without pixels keeps its format
    tiny = ctx.image(np.ones((1, 1), np.float32))
    assert tiny.downsample().info() == (0, 0, 1, 4) and tiny.downsample().filter(1).info() == (0, 0, 1, 4)
    assert tiny.downsample().flip().downsample().info() == (0, 0, 1, 4)
    # INVALID
    assert code(lib, lambda: f.to_float(2)) == INVALID
    assert code(lib, lambda: f.filter(5)) == INVALID and code(lib, lambda: f.filter(-1)) == INVALID
    assert code(lib, lambda: f.from_float(4)) == INVALID
    assert code(lib, lambda: ctx.rgbd(f, f, 5)) == INVALID
    assert code(lib, lambda: ctx.rgbd(rgb, f, "sun")) == INVALID          # a SUN depth is 1 x uint16
    out = C.c_void_p()
    data = np.zeros(16, np.uint8)
    for w, hh, ch, bpc in ((-1, 2, 1, 1), (2, -1, 1, 1), (2, 2, 0, 1), (2, 2, 5, 1), (2, 2, 1, 3), (2, 2, 1, 8)):
        assert L.visma_icp_image_create(h, w, hh, ch, bpc, data.ctypes.data_as(C.c_void_p), C.byref(out)) == INVALID and not out.value
    assert L.visma_icp_image_create(h, 2, 2, 1, 1, None, C.byref(out)) == INVALID
    assert L.visma_icp_image_create(h, 2, 2, 1, 1, data.ctypes.data_as(C.c_void_p), None) == INVALID
    assert L.visma_icp_image_get(h, f._i, data.ctypes.data_as(C.c_void_p), 47) == INVALID          # 48 bytes
    assert L.visma_icp_image_copy(h, None, C.byref(out)) == INVALID
    assert L.visma_icp_image_info(None, None, None, None, None) == INVALID
    assert L.visma_icp_image_from_odometry(h, 8, 0, C.byref(out)) == INVALID                         # src_xyz is no Image
    assert L.visma_icp_image_from_odometry(h, 0, 8, C.byref(out)) == INVALID
    # an image of another context
    other = lib.Context(0)
    try:
        assert L.visma_icp_image_copy(other._h, f._i, C.byref(out)) == INVALID and not out.value
        assert L.visma_icp_image_destroy(other._h, f._i) == INVALID
        # STATE: no odometry frames in a context that never prepared
        assert L.visma_icp_image_from_odometry(other._h, 0, 0, C.byref(out)) == STATE
    finally:
        other.close()
    # a destroyed image is no image of the context any more
    gone = f.copy()
    handle = gone._i
    gone.close()
    assert L.visma_icp_image_copy(h, handle, C.byref(out)) == INVALID
    for img in (f, b, rgb, tiny):
        img.close()


# ---- the hand-offs ------------------------------------------------------------------------------------------------------------
def volume_bytes(vol):
    if vol.scalable:
        units = vol.units()
        return [np.asarray(units).tobytes()] + [x.tobytes() for u in units for x in vol.volume(u) if x is not None]
    return [x.tobytes() for x in vol.volume() if x is not None]


def make_volume(lib, ctx, scalable, color_type):
    if scalable:
        return ctx.tsdf_scalable(2.0 / 32, 0.1, color_type, volume_unit_resolution=8, depth_sampling_stride=4)
    return ctx.tsdf_uniform(2.0, 32, 0.1, color_type, origin=(-1.0, -1.0, -1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("scalable", (False, True))
@pytest.mark.parametrize("color", ("rgb8", "gray32", "none"))
def test_integrate_of_resident_images_equals_the_host_array_entry_point(lib, ctx, scalable, color):
    frames, k = tsdf_scene.frames(64, 48, 2)
    ct = {"rgb8": lib.TSDF_COLOR_RGB8, "gray32": lib.TSDF_COLOR_GRAY32, "none": lib.TSDF_COLOR_NONE}[color]
    a, b = make_volume(lib, ctx, scalable, ct), make_volume(lib, ctx, scalable, ct)
    try:
        for depth, rgb, gray, E in frames:
            col = {"rgb8": rgb, "gray32": gray, "none": None}[color]
            a.integrate(depth, col, k, E)
            with ctx.image(depth) as d:
                c = None if col is None else ctx.image(col)
                b.integrate(d, c, k, E)
                if c is not None:
                    c.close()
        va, vb = volume_bytes(a), volume_bytes(b)
        assert len(va) == len(vb) and va == vb
        assert any(np.frombuffer(x, np.uint8).any() for x in va)         # something was integrated
        # a wrong-format image leaves the volume's bytes unchanged
        depth, rgb, gray, E = frames[0]
        wrong = [(ctx.image((depth * 1000).astype(np.uint16)), None if color == "none" else ctx.image({"rgb8": rgb, "gray32": gray}[color]))]
        if color != "none":
            wrong.append((ctx.image(depth), ctx.image(gray if color == "rgb8" else rgb)))
            wrong.append((ctx.image(depth), ctx.image(np.zeros((48, 63, 3), np.uint8) if color == "rgb8" else np.zeros((47, 64), np.float32))))
            wrong.append((ctx.image(depth), None))
        for d, c in wrong:
            assert code(lib, lambda: b.integrate(d, c, k, E)) == INVALID
            d.close()
            if c is not None:
                c.close()
        assert volume_bytes(b) == vb
    finally:
        a.close(); b.close()


@pytest.fixture(scope="module")
def pair():
    return odometry_scene.frames(64, 48)


@pytest.mark.gpu
@pytest.mark.parametrize("method", (0, 1))
def test_rgbd_odometry_of_resident_images_equals_the_host_array_entry_point(lib, ctx, pair, method):
    sg, sd, tg, td, k = pair
    option = lib.odometry_option(iterations=(4, 3, 2))
    want = ctx.rgbd_odometry(sg, sd, tg, td, k, method=method, option=option)
    imgs = [ctx.image(a) for a in (sg, sd, tg, td)]
    got = ctx.rgbd_odometry(*imgs, k, method=method, option=option)
    assert got.success == want.success and want.success
    assert got.T.tobytes() == want.T.tobytes() and got.information.tobytes() == want.information.tobytes()
    assert got.information_pairs == want.information_pairs and got.pairs.tobytes() == want.pairs.tobytes()
    # the resident pyramid is the host-array call's, and a level taken device to device is the level read back
    ctx.odometry_prepare(*imgs, k, option=option)
    resident = [[ctx.odometry_image(w, l) for w in range(8)] for l in range(3)]
    handed = []
    for l in range(3):
        for w in range(8):
            with ctx.image_from_odometry(w, l) as img:
                handed.append(img.get())
                assert img.info() == (64 >> l, 48 >> l, 1, 4)
    ctx.odometry_prepare(sg, sd, tg, td, k, option=option)
    for l in range(3):
        for w in range(8):
            host = ctx.odometry_image(w, l)
            assert host.tobytes() == resident[l][w].tobytes(), (l, w)
            assert host.tobytes() == handed[8 * l + w].tobytes() and host.shape == handed[8 * l + w].shape, (l, w)
    # wrong formats and sizes
    u16 = ctx.image(np.zeros((48, 64), np.uint16))
    small = ctx.image(np.zeros((47, 64), np.float32))
    assert code(lib, lambda: ctx.odometry_prepare(imgs[0], u16, imgs[2], imgs[3], k)) == INVALID
    assert code(lib, lambda: ctx.rgbd_odometry(imgs[0], imgs[1], small, imgs[3], k)) == INVALID
    for img in imgs + [u16, small]:
        img.close()


@pytest.mark.gpu
def test_the_odometry_pyramid_keeps_its_bytes_through_the_shared_filter(lib, ctx, pair):
    """The images of the resident odometry pyramid against odometry_spec's own functions (the 3-tap filter, the down-sampler
    and the scale kernel now come from the header the Image shares), and against the Image operations built from them."""
    sg, sd, tg, td, k = pair
    option = lib.odometry_option(iterations=(1, 1, 1))
    ctx.odometry_prepare(sg, sd, tg, td, k, option=option)
    opt = odometry_spec.default_option()
    # before NormalizeIntensity scales the grays, the depths: preprocess, Gaussian3, then down-sampled per level
    for which, depth in (("src_depth", sd), ("tgt_depth", td)):
        level = odometry_spec.gaussian3(odometry_spec.preprocess_depth(depth, opt))
        for l in range(3):
            got = ctx.odometry_image(which, l)
            assert odometry_spec.same_image(got, level), (which, l)
            if which == "tgt_depth":
                assert odometry_spec.same_image(ctx.odometry_image("tgt_depth_dx", l), odometry_spec.sobel_dx(level)), l
                assert odometry_spec.same_image(ctx.odometry_image("tgt_depth_dy", l), odometry_spec.sobel_dy(level)), l
                # ... and the Image's own route to the same levels
                with ctx.image(level) as img, img.filter("sobel3dx") as dx, img.filter("sobel3dy") as dy:
                    assert odometry_spec.same_image(dx.get(), odometry_spec.sobel_dx(level))
                    assert odometry_spec.same_image(dy.get(), odometry_spec.sobel_dy(level))
            level = odometry_spec.downsample(level)
    # the grays: level l + 1 is downsample(gaussian3(level l)) of the library's own (scaled) level l, and so are the Sobels
    for l in range(3):
        gray = ctx.odometry_image("tgt_gray", l)
        assert odometry_spec.same_image(ctx.odometry_image("tgt_gray_dx", l), odometry_spec.sobel_dx(gray)), l
        assert odometry_spec.same_image(ctx.odometry_image("tgt_gray_dy", l), odometry_spec.sobel_dy(gray)), l
        if l + 1 < 3:
            assert odometry_spec.same_image(ctx.odometry_image("tgt_gray", l + 1), odometry_spec.downsample(odometry_spec.gaussian3(gray))), l
            with ctx.image(gray) as img:
                levels = img.pyramid(2, True)
                assert odometry_spec.same_image(levels[1].get(), ctx.odometry_image("tgt_gray", l + 1)), l
                for x in levels:
                    x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride", (1, 3))
@pytest.mark.parametrize("kind", ("float", "uint16"))
def test_cloud_from_depth_image_equals_the_host_array_entry_point(lib, ctx, kind, stride):
    frames, k = tsdf_scene.frames(64, 48, 2)
    depth, rgb, gray, E = frames[1]
    depth = depth.copy()
    depth[5, 7] = np.nan; depth[6, 9] = -1.0; depth[0, 0] = 0.0
    if kind == "uint16":
        raw = np.minimum(depth * 1000.0, 65535.0)
        raw = np.where(np.isfinite(raw) & (raw > 0), raw, 0).astype(np.uint16)
        metres = S.depth_to_float(raw, 1000.0, 2.2)          # what the reference converts first; 2.2 m truncates a part of the frame
        assert 0 < np.count_nonzero(metres) < np.count_nonzero(raw)
        with ctx.image(raw) as img, ctx.cloud_from_depth_image(img, k, E, 1000.0, 2.2, stride) as cloud:
            got = cloud.get()
    else:
        metres = depth
        with ctx.image(depth) as img, ctx.cloud_from_depth_image(img, k, E, 123.0, 0.001, stride) as cloud:     # (the two doubles are not read)
            got = cloud.get()
    want = ctx.point_cloud_from_depth(metres, k, E, stride)
    assert len(want) > 100 and got["points"].tobytes() == want.tobytes() and got["points"].shape == want.shape
    assert got["normals"] is None and got["colors"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("color", ("rgb8", "gray32"))
def test_cloud_from_rgbd_images_equals_the_host_array_entry_point(lib, ctx, color):
    frames, k = tsdf_scene.frames(64, 48, 1)
    depth, rgb, gray, E = frames[0]
    col = rgb if color == "rgb8" else gray
    want_p, want_c = ctx.point_cloud_from_rgbd(depth, col, k, E)
    with ctx.image(depth) as d, ctx.image(col) as c, ctx.cloud_from_rgbd_images(d, c, k, E) as cloud:
        got = cloud.get()
    assert len(want_p) > 100 and got["points"].tobytes() == want_p.tobytes() and got["colors"].tobytes() == want_c.tobytes()
    assert got["normals"] is None
    # the default extrinsic is the identity, as the host-array entry point's
    with ctx.image(depth) as d, ctx.image(col) as c, ctx.cloud_from_rgbd_images(d, c, k) as cloud:
        assert cloud.get()["points"].tobytes() == ctx.point_cloud_from_rgbd(depth, col, k)[0].tobytes()


@pytest.mark.gpu
def test_cloud_from_images_of_unsupported_formats_is_the_empty_cloud(lib, ctx):
    frames, k = tsdf_scene.frames(64, 48, 1)
    depth, rgb, gray, E = frames[0]
    d, d8, d3, c16 = ctx.image(depth), ctx.image((depth * 50).astype(np.uint8)), ctx.image(rgb.astype(np.float32)), ctx.image(rgb.astype(np.uint16))
    d16 = ctx.image((depth * 1000).astype(np.uint16))
    for call in (lambda: ctx.cloud_from_depth_image(d8, k, E), lambda: ctx.cloud_from_depth_image(d3, k, E),
                 lambda: ctx.cloud_from_rgbd_images(d16, ctx.image(rgb), k, E), lambda: ctx.cloud_from_rgbd_images(d, c16, k, E),
                 lambda: ctx.cloud_from_rgbd_images(d, d3, k, E)):
        with call() as cloud:
            assert cloud.size() == (0, 0) and cloud.get()["points"].shape == (0, 3)
    assert code(lib, lambda: ctx.cloud_from_depth_image(d, k, E, stride=0)) == INVALID
    small = ctx.image(np.zeros((47, 64), np.float32))
    assert code(lib, lambda: ctx.cloud_from_rgbd_images(d, small, k, E)) == INVALID
    for img in (d, d8, d3, c16, d16, small):
        img.close()
