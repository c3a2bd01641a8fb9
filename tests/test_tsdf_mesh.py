"""ExtractTriangleMesh on the GPU (visma_icp_tsdf_extract_triangle_mesh; tsdf.hip) against the numpy specification
tests/tsdf_mesh_spec.py, which tests/test_tsdf_mesh_spec.py pins to the compiled reference.

The specification runs on the voxels the library's volume() returns, so every comparison is exact: vertices and colours bit
for bit and row for row, triangles index for index -- the order and the case rule are part of what is compared."""
import ctypes as C

import numpy as np
import pytest

import tsdf_mesh_cases as cases
import tsdf_mesh_spec as M
import tsdf_scene as scene
import tsdf_spec as S

INVALID, STATE = 1, 5


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def spec_of(vol):
    """the specification's volume dict holding the voxels the library returns"""
    R, t = vol.resolution, vol.color_type
    if vol.scalable:
        sv = S.new_scalable(vol.voxel_length, vol.sdf_trunc, t, R, 1)
        for key in map(tuple, vol.units().tolist()):
            u = S.new_volume(sv["unit_length"], R, vol.sdf_trunc, t)
            u["tsdf"], u["weight"], u["color"] = vol.volume(key)
            sv["units"][key] = u
        return sv
    v = S.new_volume(vol.length, R, vol.sdf_trunc, t, vol.origin)
    v["tsdf"], v["weight"], v["color"] = vol.volume()
    return v


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_against_spec(vol, label):
    sv = spec_of(vol)
    want_v, want_c, want_t = (M.extract_scalable if vol.scalable else M.extract_uniform)(sv)
    got_v, got_c, got_t = vol.extract_triangle_mesh()
    print("%s: %d vertices, %d triangles" % (label, len(got_v), len(got_t)))
    assert got_v.shape == want_v.shape and np.array_equal(bits(got_v), bits(want_v)), label
    assert (got_c is None) == (want_c is None)
    if want_c is not None:
        assert got_c.shape == want_c.shape and np.array_equal(bits(got_c), bits(want_c)), label
    assert got_t.dtype == np.int32 and got_t.shape == want_t.shape and np.array_equal(got_t, want_t), label
    return got_v, got_c, got_t


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES)
def test_mesh_equals_the_specification(lib, ctx, name):
    case = cases.load(name)
    vol = cases.lib_volume(ctx, case)
    v, c, t = check_against_spec(vol, name)
    assert len(t) > 0
    vol.close()


def small_uniform(ctx, R, color_type=S.COLOR_RGB8, frames=True):
    """a cube of R^3 voxels of 0.25 in front of a 17 x 17 frame of depth 0.375 + 0.25 (R // 2): a sign change in its middle"""
    vol = ctx.tsdf_uniform(0.25 * R, R, 0.75, color_type, (-0.125 * R, -0.125 * R, 0.125))
    if frames:
        depth = np.full((17, 17), 0.375 + 0.25 * ((R - 1) // 2), np.float32)
        rgb, gray = cases._paint(depth)
        vol.integrate(depth, {S.COLOR_NONE: None, S.COLOR_RGB8: rgb, S.COLOR_GRAY32: gray}[color_type], np.array([4.0, 4.0, 8.0, 8.0]), np.eye(4))
    return vol


@pytest.mark.gpu
def test_volumes_without_a_cube_give_an_empty_mesh(lib, ctx):
    """R = 1, a volume no frame went into, a scalable volume without units, a volume after Reset()"""
    one = small_uniform(ctx, 1)
    fresh = small_uniform(ctx, 8, frames=False)
    units = ctx.tsdf_scalable(0.05, 0.15, S.COLOR_RGB8, 8, 4)
    again = small_uniform(ctx, 4)
    assert len(again.extract_triangle_mesh()[2]) > 0
    again.reset()
    for vol in (one, fresh, units, again):
        v, c, t = vol.extract_triangle_mesh()
        assert v.shape == (0, 3) and c.shape == (0, 3) and t.shape == (0, 3)
        vol.close()


@pytest.mark.gpu
def test_a_single_cube(lib, ctx):
    vol = small_uniform(ctx, 2)
    v, c, t = check_against_spec(vol, "R = 2")
    assert len(v) == 4 and len(t) == 2                                   # the four z edges, one quad
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("color_type", (S.COLOR_NONE, S.COLOR_GRAY32))
def test_a_resolution_that_is_no_multiple_of_four(lib, ctx, color_type):
    case = dict(cases.load("u21"), R=7, color_type=color_type, sdf_trunc=3 * 1.6 / 7)
    vol = cases.lib_volume(ctx, case)
    v, c, t = check_against_spec(vol, "R = 7")
    assert len(t) > 0
    vol.close()


@pytest.mark.gpu
def test_one_item_beyond_a_tile(lib, ctx):
    """19 units of 3^3 voxels: 513 items, two tiles of 256 and one item"""
    depth = np.array([[0.0, 0.75, 0.0, 0.0], [0.75, 0.0, 0.0, 0.5], [0.5, 0.5, 0.0, 0.0]], np.float32)
    vol = ctx.tsdf_scalable(0.125, 0.125, S.COLOR_NONE, 3, 1)
    vol.integrate(depth, None, np.array([2.0, 2.0, 1.75, 1.125]), np.eye(4))
    assert len(vol.units()) == 19 and (19 * 27) % 256 == 1
    check_against_spec(vol, "513 items")
    vol.close()


@pytest.mark.gpu
def test_repeats_and_what_an_extraction_leaves_alone(lib, ctx):
    """two extractions give identical bytes; the volume and a following ExtractPointCloud are unchanged by one"""
    for name in ("u21", "s0"):
        case = cases.load(name)
        vol = cases.lib_volume(ctx, case)
        keys = [tuple(k) for k in vol.units().tolist()] if vol.scalable else [None]
        before = [vol.volume(k) for k in keys]
        cloud = vol.extract_point_cloud()
        a = vol.extract_triangle_mesh()
        b = vol.extract_triangle_mesh()
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        after = [vol.volume(k) for k in keys]
        for x, y in zip(before, after):
            for p, q in zip(x, y):
                assert p.tobytes() == q.tobytes()
        for p, q in zip(cloud, vol.extract_point_cloud()):
            assert p.tobytes() == q.tobytes()
        vol.close()


@pytest.mark.gpu
def test_errors(lib, ctx):
    L = lib.load()
    vol = small_uniform(ctx, 4)
    v = np.empty((64, 3)); t = np.empty((64, 3), np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    get = lambda nv, nt: L.visma_icp_tsdf_get_triangle_mesh(ctx._h, vol._v, v.ctypes.data_as(dp), None, t.ctypes.data_as(ip), nv, nt)
    assert get(0, 0) == STATE                                            # a get before its extract
    nv, nt = C.c_int64(0), C.c_int64(0)
    assert L.visma_icp_tsdf_extract_triangle_mesh(ctx._h, vol._v, C.byref(nv), C.byref(nt)) == 0
    assert 0 < nv.value <= 64 and 0 < nt.value <= 64
    assert get(nv.value + 1, nt.value) == INVALID and get(nv.value, nt.value - 1) == INVALID
    assert get(nv.value, nt.value) == 0
    assert L.visma_icp_tsdf_extract_triangle_mesh(ctx._h, vol._v, None, C.byref(nt)) == INVALID
    assert L.visma_icp_tsdf_extract_triangle_mesh(ctx._h, None, C.byref(nv), C.byref(nt)) == INVALID
    other = lib.Context(0)                                               # a volume of another context
    assert L.visma_icp_tsdf_extract_triangle_mesh(other._h, vol._v, C.byref(nv), C.byref(nt)) == INVALID
    other.close()
    depth = np.full((17, 17), 0.625, np.float32)                         # a frame invalidates the mesh
    vol.integrate(depth, cases._paint(depth)[0], np.array([4.0, 4.0, 8.0, 8.0]), np.eye(4))
    assert get(nv.value, nt.value) == STATE
    vol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scalable", (False, True))
def test_hostile_frames(lib, ctx, scalable):
    """NaN, +-inf, negative, denormal and huge depths among ordinary ones: a +inf depth integrates as tsdf 1 and must not
    break a cube's validity (there is no tsdf range test in the mesh)"""
    frames, k = scene.hostile_frames()
    if scalable:
        vol = ctx.tsdf_scalable(0.05, 0.15, S.COLOR_RGB8, 8, 4)
    else:
        vol = ctx.tsdf_uniform(1.6, 21, 3 * 1.6 / 21, S.COLOR_RGB8, (-0.8, -0.75, -0.85))
    for fr in frames:
        vol.integrate(fr[0], fr[1], k, fr[3])
    v, c, t = check_against_spec(vol, "hostile, scalable %d" % scalable)
    assert len(t) > 0 and np.isfinite(v).all() and np.isfinite(c).all()
    vol.close()
