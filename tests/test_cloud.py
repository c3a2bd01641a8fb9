"""The PointCloud operations on the GPU (visma_icp_cloud_*; cloud.hip) against the numpy specification tests/cloud_spec.py,
which tests/test_cloud_spec.py pins to the compiled reference: every case and program of tests/cloud_cases.py with the
library's summation order (chunks of 16,384 points), rows and results as their bits (tests/cloud_cases.py: bits), counts and
flags exactly.  voxel_down_sample and estimate_normals of a resident cloud against the host-array entry points, and the cloud
of a TSDF volume against its read-back, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import cloud_cases as cases
import cloud_spec as S
import tsdf_scene

INVALID, STATE = 1, 5


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def upload(ctx, c):
    return ctx.cloud(c["points"], c["normals"], c["colors"])


def run(ctx, c, program):
    """cloud_spec.run on the library -> what get() returns, the results"""
    cloud, results = upload(ctx, c), []
    for op, *arg in program:
        if op == "transform":
            cloud.transform(arg[0])
        elif op == "norm":
            cloud.normalize_normals()
        elif op == "paint":
            cloud.paint_uniform_color(arg[0])
        elif op == "append":
            if arg[0] is None:
                cloud.append(cloud)
            else:
                with upload(ctx, arg[0]) as other:
                    cloud.append(other)
        elif op == "bounds":
            results.append(np.concatenate(cloud.bounds()))
        elif op in ("select", "uniform", "crop"):
            out = cloud.select(arg[0]) if op == "select" else cloud.uniform_down_sample(arg[0]) if op == "uniform" else cloud.crop(arg[0], arg[1])
            cloud.close()
            cloud = out
        elif op == "orient_dir":
            cloud.orient_normals_to_align_with_direction(arg[0])
        elif op == "orient_cam":
            cloud.orient_normals_towards_camera_location(arg[0])
        elif op == "meancov":
            mean, cov = cloud.mean_and_covariance()
            results.append(np.concatenate([mean, cov.reshape(-1)]))
        elif op == "mahal":
            results.append(cloud.mahalanobis_distance())
        else:
            raise ValueError(op)
    got = cloud.get()
    n, flags = cloud.size()
    assert n == len(got["points"]) == len(cloud)
    assert flags == sum(bit for bit, k in ((1, "normals"), (2, "colors")) if got[k] is not None)
    cloud.close()
    return got, results


def same(got, want, label):
    for k in S.ATTRS:
        assert (got[k] is None) == (want[k] is None), (label, k)
        if want[k] is not None:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
            bad = np.nonzero((cases.bits(got[k]) != cases.bits(want[k])).any(axis=1))[0]
            assert len(bad) == 0, (label, k, len(bad), bad[:5], got[k][bad[:3]], want[k][bad[:3]])


def same_results(got, want, label):
    assert len(got) == len(want), label
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (label, i, a.shape, b.shape)
        bad = np.nonzero(cases.bits(a) != cases.bits(b))[0]
        assert len(bad) == 0, (label, i, len(bad), bad[:5], a[bad[:5]], b[bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,p", cases.items())
def test_a_program_equals_the_specification(lib, ctx, name, p):
    c, programs = cases.load()[name]
    want, want_results = cases.spec(name, p, cases.CHUNK)
    got, results = run(ctx, c, programs[p])
    print("%s program %d: %d points, %d results" % (name, p, len(got["points"]), len(results)))
    same(got, want, (name, p))
    same_results(results, want_results, (name, p))


@pytest.mark.gpu
def test_two_runs_are_bit_identical(lib, ctx):
    for name in ("tile513", "big", "sums%d" % cases.SUM_SIZES[-1], "normals", "bounds_last_max"):
        c, programs = cases.load()[name]
        for program in programs:
            a, ra = run(ctx, c, program)
            b, rb = run(ctx, c, program)
            assert [x.tobytes() for x in ra] == [x.tobytes() for x in rb], name
            for k in S.ATTRS:
                assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), (name, k)


# ---- against the host-array entry points ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet():
    """about 5,000 points of a bumpy sheet with normals and colours, and a NaN point in their middle"""
    rng = np.random.default_rng(51)
    n = 5003
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    p = np.stack([xy[:, 0], xy[:, 1], 0.2 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + 0.002 * rng.normal(size=n)], axis=1)
    p[n // 2] = (np.nan, 0.1, 0.2)
    return p, rng.normal(size=(n, 3)), rng.uniform(size=(n, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("attrs", ("plain", "normals", "both"))
def test_voxel_down_sample_equals_the_host_array_entry_point(lib, ctx, sheet, attrs):
    p, nrm, col = sheet
    nrm, col = (nrm if attrs != "plain" else None), (col if attrs == "both" else None)
    for voxel in (0.05, 0.31, 0.0):
        want = dict(zip(S.ATTRS, ctx.voxel_down_sample(p, voxel, normals=nrm, colors=col)))
        with ctx.cloud(p, nrm, col) as cloud, cloud.voxel_down_sample(voxel) as down:
            got = down.get()
        print("voxel %g, %s: %d -> %d points" % (voxel, attrs, len(p), len(got["points"])))
        if len(want["points"]) == 0:                         # (an empty cloud has no attributes)
            want["normals"] = want["colors"] = None
        for k in S.ATTRS:
            assert (got[k] is None) == (want[k] is None), (voxel, attrs, k)
            assert got[k] is None or (got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes()), (voxel, attrs, k)
        assert (voxel == 0.0 and len(got["points"]) == 0) or 0 < len(got["points"]) < len(p)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,knn,radius", (("knn", 12, None), ("radius", None, 0.08), ("hybrid", 9, 0.1), ("trivial", 2, None),
                                              ("trivial_radius", 30, 0.0)))
@pytest.mark.parametrize("given", (False, True))
def test_estimate_normals_equals_the_host_array_entry_point(lib, ctx, sheet, kind, knn, radius, given):
    p, nrm, _ = sheet
    want = ctx.estimate_normals(p, knn=knn, radius=radius, normals=nrm if given else None)
    with ctx.cloud(p, nrm if given else None) as cloud:
        cloud.estimate_normals(knn=knn, radius=radius)
        got = cloud.get()
        if not given:                                        # a second call keeps the sign of the first one's normals
            cloud.estimate_normals(knn=knn, radius=radius)
            want_again = ctx.estimate_normals(p, knn=knn, radius=radius, normals=want)
            assert cloud.get()["normals"].tobytes() == want_again.tobytes(), kind
    assert got["normals"] is not None and got["normals"].shape == want.shape
    bad = np.nonzero((got["normals"].view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
    assert len(bad) == 0, (kind, given, len(bad), bad[:5], got["normals"][bad[:3]], want[bad[:3]])
    assert got["points"].tobytes() == p.tobytes()
    if kind.startswith("trivial"):
        assert (got["normals"] == (0.0, 0.0, 1.0)).all()
    else:
        assert (got["normals"][len(p) // 2] == (0.0, 0.0, 1.0)).all()       # the NaN point has no neighbours: the fall-back


@pytest.mark.gpu
def test_estimate_normals_without_a_finite_point(lib, ctx):
    """no point to bin from: the origin stays the zeros on both paths"""
    p = np.full((5, 3), np.nan)
    want = ctx.estimate_normals(p, knn=3)
    with ctx.cloud(p) as cloud:
        cloud.estimate_normals(knn=3)
        assert cloud.get()["normals"].tobytes() == want.tobytes()


# ---- the cloud of a TSDF volume ----------------------------------------------------------------------------------------------
def small_volume(ctx, color):
    frames, k = tsdf_scene.frames(64, 48)
    vol = ctx.tsdf_uniform(1.5, 24, 0.15, "rgb8" if color else "none", (-0.75, -0.75, -0.75))
    return vol, frames, k


@pytest.mark.gpu
@pytest.mark.parametrize("color", (True, False))
def test_from_tsdf(lib, ctx, color):
    vol, frames, k = small_volume(ctx, color)
    L, out = lib.load(), C.c_void_p()
    for voxel in (0, 1):                                     # before an extract
        assert L.visma_icp_cloud_from_tsdf(ctx._h, vol._v, voxel, C.byref(out)) == STATE and not out.value
    for fr in frames[:2]:
        vol.integrate(fr[0], fr[1] if color else None, k, fr[3])
    pts, nrm, col = vol.extract_point_cloud()
    assert L.visma_icp_cloud_from_tsdf(ctx._h, vol._v, 1, C.byref(out)) == STATE and not out.value     # the other kind is not extracted yet
    vpts, vcol = vol.extract_voxel_point_cloud()
    assert len(pts) > 100 and len(vpts) > 100 and (col is None) == (not color)
    with vol.point_cloud() as surface, vol.point_cloud(voxel=True) as voxels:
        got, vgot = surface.get(), voxels.get()
        same(got, S.cloud(pts, nrm, col), "surface")
        assert got["points"].tobytes() == pts.tobytes() and got["normals"].tobytes() == nrm.tobytes()
        assert (got["colors"] is None) == (not color) and (not color or got["colors"].tobytes() == col.tobytes())
        assert vgot["points"].tobytes() == vpts.tobytes() and vgot["normals"] is None and vgot["colors"].tobytes() == vcol.tobytes()
        # the copy is the cloud's own: changing it leaves the volume's extraction as it was
        surface.transform(np.diag([2.0, 2.0, 2.0, 1.0]))
        assert surface.get()["points"].tobytes() != pts.tobytes()
        with vol.point_cloud() as second:
            assert second.get()["points"].tobytes() == pts.tobytes()
    vol.integrate(frames[2][0], frames[2][1] if color else None, k, frames[2][3])
    for voxel in (0, 1):                                     # after a frame
        assert L.visma_icp_cloud_from_tsdf(ctx._h, vol._v, voxel, C.byref(out)) == STATE and not out.value
    vol.extract_point_cloud()
    vol.reset()
    assert L.visma_icp_cloud_from_tsdf(ctx._h, vol._v, 0, C.byref(out)) == STATE                     # after a reset
    vol.close()


# ---- errors --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors(lib, ctx):
    L = lib.load()
    dp, i64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    out = C.c_void_p()
    ptr = lambda a: a.ctypes.data_as(dp)
    assert L.visma_icp_cloud_create(ctx._h, ptr(p), -1, None, None, C.byref(out)) == INVALID and not out.value
    assert L.visma_icp_cloud_create(ctx._h, ptr(p), 1 << 31, None, None, C.byref(out)) == INVALID
    assert L.visma_icp_cloud_create(ctx._h, None, 3, None, None, C.byref(out)) == INVALID
    assert L.visma_icp_cloud_create(ctx._h, ptr(p), 3, None, None, None) == INVALID
    assert L.visma_icp_cloud_create(ctx._h, ptr(p), 3, None, None, C.byref(out)) == 0 and out.value
    cloud = lib.Cloud(ctx, C.c_void_p(out.value))
    # get: the count, attributes the cloud does not have
    got, extra = np.empty((3, 3)), np.empty((3, 3))
    assert L.visma_icp_cloud_get(ctx._h, cloud._c, ptr(got), None, None, 3) == 0 and np.array_equal(got, p)
    assert L.visma_icp_cloud_get(ctx._h, cloud._c, ptr(got), None, None, 2) == INVALID
    assert L.visma_icp_cloud_get(ctx._h, cloud._c, ptr(got), None, None, 4) == INVALID
    assert L.visma_icp_cloud_get(ctx._h, cloud._c, None, ptr(extra), None, 3) == STATE
    assert L.visma_icp_cloud_get(ctx._h, cloud._c, None, None, ptr(extra), 3) == STATE
    assert L.visma_icp_cloud_get(ctx._h, cloud._c, None, None, None, 3) == 0
    # select: an index outside [0, n)
    for bad in ([0, 1, 3], [-1], [1 << 40]):
        idx = np.array(bad, np.int64)
        assert L.visma_icp_cloud_select(ctx._h, cloud._c, idx.ctypes.data_as(i64), len(idx), C.byref(out)) == INVALID and not out.value
    assert L.visma_icp_cloud_select(ctx._h, cloud._c, None, 2, C.byref(out)) == INVALID
    assert L.visma_icp_cloud_uniform_down_sample(ctx._h, cloud._c, -1, C.byref(out)) == INVALID
    # missing normals
    ref = np.array([0.0, 0.0, 1.0])
    assert L.visma_icp_cloud_orient_normals_to_align_with_direction(ctx._h, cloud._c, ptr(ref)) == STATE
    assert L.visma_icp_cloud_orient_normals_towards_camera_location(ctx._h, cloud._c, ptr(ref)) == STATE
    assert L.visma_icp_cloud_estimate_normals(ctx._h, cloud._c, 3, 10, 0.1) == INVALID
    # NULL arguments
    assert L.visma_icp_cloud_transform(ctx._h, cloud._c, None) == INVALID
    assert L.visma_icp_cloud_transform(ctx._h, None, ptr(np.eye(4))) == INVALID
    assert L.visma_icp_cloud_crop(ctx._h, cloud._c, None, ptr(ref), C.byref(out)) == INVALID
    assert L.visma_icp_cloud_crop(ctx._h, cloud._c, ptr(ref), ptr(ref), None) == INVALID
    assert L.visma_icp_cloud_bounds(ctx._h, cloud._c, None, ptr(ref)) == INVALID
    assert L.visma_icp_cloud_mean_and_covariance(ctx._h, cloud._c, None, None) == INVALID
    assert L.visma_icp_cloud_mahalanobis_distance(ctx._h, cloud._c, None) == INVALID
    assert L.visma_icp_cloud_paint_uniform_color(ctx._h, cloud._c, None) == INVALID
    assert L.visma_icp_cloud_append(ctx._h, cloud._c, None) == INVALID
    # a cloud and a volume of another context
    other = lib.Context(0)
    foreign = other.cloud(p)
    assert L.visma_icp_cloud_normalize_normals(other._h, cloud._c) == INVALID
    assert L.visma_icp_cloud_destroy(other._h, cloud._c) == INVALID
    assert L.visma_icp_cloud_append(ctx._h, cloud._c, foreign._c) == INVALID
    assert L.visma_icp_cloud_append(other._h, cloud._c, foreign._c) == INVALID
    vol, frames, k = small_volume(ctx, False)
    vol.integrate(frames[0][0], None, k, frames[0][3])
    vol.extract_point_cloud()
    assert L.visma_icp_cloud_from_tsdf(other._h, vol._v, 0, C.byref(out)) == INVALID
    assert L.visma_icp_cloud_from_tsdf(ctx._h, None, 0, C.byref(out)) == INVALID
    assert L.visma_icp_cloud_from_tsdf(ctx._h, vol._v, 2, C.byref(out)) == INVALID
    assert L.visma_icp_cloud_from_tsdf(ctx._h, vol._v, 0, C.byref(out)) == 0 and out.value
    assert L.visma_icp_cloud_destroy(ctx._h, C.c_void_p(out.value)) == 0
    foreign.close()
    other.close()
    vol.close()
    assert cloud.get()["points"].tobytes() == p.tobytes() and cloud.size() == (3, 0)      # the errors left the cloud usable
    cloud.close()
