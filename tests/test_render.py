"""The mesh renderer on the GPU (visma_icp_render, visma_icp_render_edges; render.hip) against visma_icp_render_host, which
tests/test_render_host.py pins to the written rule: every case of tests/render_cases.py bit for bit, the cull scenes and the
scenes of the large path (several items per triangle, three compaction tiles) among them; half a million triangles for the
grid strides, the scan's carry and the tile loops; the edge kernel on uploaded hostile images; a mesh extracted device
to device from a TSDF volume rendered at its frame's pose, the depth Image handed on to cloud_from_depth_image and to
TsdfVolume.integrate; two runs and a pose folded into the mesh byte for byte; wrong arguments and wrong-context objects
refused."""
import numpy as np
import pytest

import render_cases as cases
import render_spec as S
import tsdf_scene

INVALID = 1


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def code(lib, call):
    with pytest.raises(lib.IcpError) as e:
        call()
    return e.value.code


def device(ctx, c, mesh=None):
    """-> depth, index, mask, edges of the case on the device (edges of the metric depth, as render_host's)"""
    own = mesh is None
    mesh = ctx.trimesh(c["V"], c["F"]) if own else mesh
    args = (c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"])
    d, i, m = mesh.render(*args, encoding=c["encoding"])
    metric = d if c["encoding"] == 0 else mesh.render(*args)[0]
    e = ctx.render_edges(metric)
    assert d.info() == i.info() == (c["w"], c["h"], 1, 4) and m.info() == e.info() == (c["w"], c["h"], 1, 1)
    assert i.is_int32() and not d.is_int32() and not m.is_int32()
    out = d.get(), i.get(), m.get(), e.get()
    if own:
        mesh.close()
    return out


def same(got, want):
    for g, w, what in zip(got, want, ("depth", "index", "mask", "edges")):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert cases.bits(g).tobytes() == cases.bits(w).tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES)
def test_render_equals_render_host(lib, ctx, name):
    c = cases.CASES[name]
    same(device(ctx, c), cases.host(lib, c))


@pytest.mark.gpu
def test_the_strides_the_scan_carry_and_the_tile_loops(lib, ctx):
    """2048 x 256 + 300 triangles at 97 x 67 (render_cases.stride), against render_host; the numpy rule would take minutes.
    Every pass over triangles launches at most 2048 blocks of 256 and strides: rn_setup and rn_cover_small take a second
    trip, count_kernel and write_kernel a second tile per block (2050 tiles), and the scan carries across its chunks of 1024
    tiles twice.  Nearly all triangles lie behind the camera; of the 200 others, large (two items each) and small ones sit
    beyond triangle 2048 x 256, and large ones in tiles beyond 1024, where their item rows depend on the carry
    (tests/test_render_host.py asserts that the host sees them).  NOT reached, here or anywhere: rn_cover_large's own cap of
    2^20 blocks.  A second trip of its item loop needs more than 2^20 items, which is four billion box pixels; no test of a
    few seconds can walk them."""
    c, large, small = cases.stride()
    want = cases.stride_host(lib)
    seen = np.unique(want[1][want[1] >= 0])
    assert seen.max() > cases.STRIDE and (np.isin(seen, large) & (seen // cases.TILE > 1024)).any()
    same(device(ctx, c), want)


@pytest.mark.gpu
def test_render_edges_of_uploaded_images(lib, ctx):
    """rn_edges on images no render produces, against the written rule: NaN, infinities, negatives, -0.0 and a denormal as
    centres and as neighbours; no interior (w or h <= 10), one interior pixel, rows across blocks of 256 pixels."""
    def on_device(d):
        with ctx.image(d) as img, ctx.render_edges(img) as e:
            assert e.info() == (d.shape[1], d.shape[0], 1, 1)
            return e.get()

    d = cases.hostile_depth()
    want = S.edges(d)
    assert want.any() and (want[5:7, 5:11] == 0).any()
    got = on_device(d)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    for w, h in cases.EDGE_SHAPES:
        d = cases.stepped_depth(w, h, 5)
        want = S.edges(d)
        assert d.shape == (h, w)
        assert want.any() == (w > 10 and h > 10), (w, h)
        if (w, h) == (11, 11):
            assert want[5, 5] == 255 and want.sum() == 255
        got = on_device(d)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (w, h)


@pytest.mark.gpu
def test_a_mesh_from_a_volume_renders_and_its_depth_is_handed_on(lib, ctx):
    frames, k = tsdf_scene.frames(64, 48, 1)
    depth, rgb, gray, E = frames[0]
    vol = ctx.tsdf_uniform(2.0, 32, 0.1, lib.TSDF_COLOR_NONE, origin=(-1.0, -1.0, -1.0))
    vol.integrate(depth, None, k, E)
    vtx, _, tri = vol.extract_triangle_mesh()
    assert len(tri) > 100
    mesh = vol.triangle_mesh()                               # device to device
    c = cases.case(vtx, tri, 64, 48, k, E)
    got = device(ctx, c, mesh)
    same(got, cases.host(lib, c))
    assert (got[2] == 255).sum() > 300 and got[3].any()
    # where the sensor saw the surface inside the volume, the rendered depth is the sensor's to within a voxel
    both = (got[0] > 0) & (depth > 0)
    assert both.sum() > 300 and np.median(np.abs(got[0][both] - depth[both])) < 2.0 / 32
    d_img = mesh.render(64, 48, k, E)[0]
    # the resident depth into a cloud: the same rows as the downloaded pixels uploaded again
    with ctx.cloud_from_depth_image(d_img, k, E) as a, ctx.image(got[0]) as again, ctx.cloud_from_depth_image(again, k, E) as b:
        pa, pb = a.get()["points"], b.get()["points"]
        assert len(pa) == (got[0] > 0).sum() and pa.tobytes() == pb.tobytes()
    # ... and into a volume
    va = ctx.tsdf_uniform(2.0, 32, 0.1, lib.TSDF_COLOR_NONE, origin=(-1.0, -1.0, -1.0))
    vb = ctx.tsdf_uniform(2.0, 32, 0.1, lib.TSDF_COLOR_NONE, origin=(-1.0, -1.0, -1.0))
    va.integrate(d_img, None, k, E)
    vb.integrate(got[0], None, k, E)
    ta, tb = va.volume(), vb.volume()
    assert ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() == tb[1].tobytes() and ta[1].any()
    # the index image is no depth
    i_img = mesh.render(64, 48, k, E)[1]
    assert code(lib, lambda: va.integrate(i_img, None, k, E)) == INVALID
    assert code(lib, lambda: ctx.render_edges(i_img)) == INVALID
    with ctx.cloud_from_depth_image(i_img, k, E) as none:
        assert len(none) == 0
    assert i_img.copy().is_int32()
    for v in (vol, va, vb):
        v.close()
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("crowd", "sphere_tilted", "inside_box", "planes_depth_buffer"))
def test_two_runs_and_a_pose_folded_into_the_mesh_give_the_same_bytes(lib, ctx, name):
    c = cases.CASES[name]
    first = device(ctx, c)
    same(device(ctx, c), first)                              # nothing depends on scheduling
    # Transform(E) computes the renderer's own camera points, and the identity pose then leaves them as they are
    # (1 x + 0 y + 0 z + 0 is x): to the bit, depth included
    mesh = ctx.trimesh(c["V"], c["F"])
    mesh.transform(c["E"])
    same(device(ctx, cases.with_(c, E=np.eye(4)), mesh), first)
    mesh.close()


@pytest.mark.gpu
def test_wrong_arguments_and_wrong_context_objects_are_refused(lib, ctx):
    c = cases.CASES["sphere_anchor"]
    other = lib.Context(0)
    mesh, foreign = ctx.trimesh(c["V"], c["F"]), other.trimesh(c["V"], c["F"])
    for name, change in cases.INVALID:
        k = cases.with_(c, **change)
        assert code(lib, lambda: mesh.render(k["w"], k["h"], k["K"], k["E"], k["z_near"], k["z_far"], k["encoding"])) == INVALID, name
    args = (c["w"], c["h"], c["K"], c["E"])
    assert code(lib, lambda: lib.TriMesh(ctx, foreign._m).render(*args)) == INVALID
    d = foreign.render(*args)[0]
    assert code(lib, lambda: ctx.render_edges(d)) == INVALID
    mask = mesh.render(*args)[2]
    assert code(lib, lambda: ctx.render_edges(mask)) == INVALID        # not 1 x float
    # each output may be NULL
    import ctypes as C
    K, E = np.array(c["K"]), np.ascontiguousarray(c["E"]).reshape(-1)
    dp = C.POINTER(C.c_double)
    only = C.c_void_p()
    assert ctx.L.visma_icp_render(ctx._h, mesh._m, c["w"], c["h"], K.ctypes.data_as(dp), E.ctypes.data_as(dp), 0.05, 10.0, 0, None, None,
                                  C.byref(only)) == 0
    assert lib.Image(ctx, only).get().tobytes() == mask.get().tobytes()
    other.close()
    mesh.close()
