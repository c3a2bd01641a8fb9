"""The TriangleMesh operations on the GPU (visma_icp_trimesh_*; trimesh.hip) against the numpy specification
tests/trimesh_spec.py, which tests/test_trimesh_spec.py pins to the compiled reference: every case and program of
tests/trimesh_cases.py, vertices, normals and colours as their bits (tests/trimesh_cases.py: bits), triangles index for index,
removed counts exactly."""
import ctypes as C

import numpy as np
import pytest

import trimesh_cases as cases
import trimesh_spec as T
import tsdf_mesh_cases as tsdf_cases

INVALID, STATE = 1, 5


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def upload(ctx, m):
    return ctx.trimesh(m["vertices"], m["triangles"], m["vertex_normals"], m["vertex_colors"], m["triangle_normals"])


def run(ctx, m, program):
    """trimesh_spec.run on the library -> what get() returns, the removed counts"""
    mesh, removed = upload(ctx, m), []
    for op, *arg in program:
        if op == "ctn":
            mesh.compute_triangle_normals(bool(arg[0]))
        elif op == "cvn":
            mesh.compute_vertex_normals(bool(arg[0]))
        elif op == "norm":
            mesh.normalize_normals()
        elif op == "rdv":
            removed.append(mesh.remove_duplicated_vertices())
        elif op == "rdt":
            removed.append(mesh.remove_duplicated_triangles())
        elif op == "rnmt":
            removed.append(mesh.remove_non_manifold_triangles())
        elif op == "rnmv":
            removed.append(mesh.remove_non_manifold_vertices())
        elif op == "purge":
            removed.extend(mesh.purge())
        elif op in ("select", "crop"):
            out = mesh.select(arg[0]) if op == "select" else mesh.crop(arg[0], arg[1])
            mesh.close()
            mesh = out
        elif op == "transform":
            mesh.transform(arg[0])
        else:
            raise ValueError(op)
    got = mesh.get()
    nv, nt, flags = mesh.size()
    assert (nv, nt) == (len(got["vertices"]), len(got["triangles"]))
    assert flags == sum(bit for bit, k in ((1, "vertex_normals"), (2, "vertex_colors"), (4, "triangle_normals")) if got[k] is not None)
    mesh.close()
    return got, removed


def same(got, want, label):
    for k in T.ATTRS:
        assert (got[k] is None) == (want[k] is None), (label, k)
        if want[k] is not None:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
            bad = np.nonzero((cases.bits(got[k]) != cases.bits(want[k])).any(axis=1))[0]
            assert len(bad) == 0, (label, k, len(bad), bad[:5], got[k][bad[:3]], want[k][bad[:3]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,p", cases.items())
def test_a_program_equals_the_specification(lib, ctx, name, p):
    m, programs = cases.load()[name]
    want, want_removed = cases.spec(name, p)
    got, removed = run(ctx, m, programs[p])
    print("%s program %d: %d vertices, %d triangles, removed %s" % (name, p, len(got["vertices"]), len(got["triangles"]), removed))
    assert list(removed) == list(want_removed)
    same(got, want, (name, p))


@pytest.mark.gpu
def test_two_runs_are_bit_identical(lib, ctx):
    for name in ("soup", "fan", "tile513", "crop", "big"):
        m, programs = cases.load()[name]
        for program in programs:
            a, ra = run(ctx, m, program)
            b, rb = run(ctx, m, program)
            assert ra == rb
            for k in T.ATTRS:
                assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), (name, k)


@pytest.fixture(scope="module")
def tsdf_meshes(lib, ctx):
    """plane and u21 extracted once: the volume (vol.triangle_mesh() is a fresh device-to-device copy) and its download"""
    out = {}
    for name in ("plane", "u21"):
        vol = tsdf_cases.lib_volume(ctx, tsdf_cases.load(name))
        out[name] = (vol,) + tuple(vol.extract_triangle_mesh())
    yield out
    for item in out.values():
        item[0].close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("plane", "u21"))
def test_from_tsdf(lib, ctx, tsdf_meshes, name):
    vol, v, c, t = tsdf_meshes[name]
    want = T.mesh(v, t, None, c)
    copy, again = vol.triangle_mesh(), upload(ctx, want)     # device to device; downloaded and re-created
    got = copy.get()
    same(got, want, name)
    assert got["vertex_normals"] is None and got["triangle_normals"] is None and got["vertex_colors"] is not None
    for a in (copy, again):
        a.compute_vertex_normals(True)
    normals = copy.get()
    same(normals, again.get(), name)
    spec = T.copy(want)
    T.compute_vertex_normals(spec, True)
    same(normals, spec, name)
    # Purge: plane has coinciding vertices and zero-area triangles, u21 has neither
    removed = copy.purge()
    assert tuple(removed) == tuple(T.purge(spec))
    same(copy.get(), spec, name)
    print("%s: %d vertices, %d triangles, Purge removed %s" % (name, len(v), len(t), removed))
    if name == "plane":
        assert removed[0] > 0 and removed[1] + removed[2] > 0, removed
    else:
        assert removed == (0, 0, 0, 0)
        same(copy.get(), normals, name)                      # unchanged
    copy.close(); again.close()
    assert vol.extract_triangle_mesh()[0].tobytes() == v.tobytes()      # the copy was the mesh's own: the volume's is untouched


@pytest.mark.gpu
def test_errors(lib, ctx):
    L = lib.load()
    dp, ip, i64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    out = C.c_void_p()

    def create(tri, nv=3, h=None):
        t = np.array(tri, np.int32).reshape(-1, 3)
        return L.visma_icp_trimesh_create(h or ctx._h, v.ctypes.data_as(dp), nv, None, None, t.ctypes.data_as(ip), len(t), None, C.byref(out))

    for bad in ([[0, 1, 3]], [[0, -1, 2]], [[0, 1, 2], [2, 1, 1 << 30]]):
        assert create(bad) == INVALID and not out.value      # validated on the device before the mesh exists
    assert create([[0, 0, 0]], nv=0) == INVALID
    assert L.visma_icp_trimesh_create(ctx._h, v.ctypes.data_as(dp), 1 << 31, None, None, None, 0, None, C.byref(out)) == INVALID
    assert L.visma_icp_trimesh_create(ctx._h, v.ctypes.data_as(dp), 3, None, None, None, (1 << 31) // 3 + 1, None, C.byref(out)) == INVALID
    assert L.visma_icp_trimesh_create(ctx._h, None, 3, None, None, None, 0, None, C.byref(out)) == INVALID
    assert create([[0, 1, 2]]) == 0 and out.value
    mesh = lib.TriMesh(ctx, C.c_void_p(out.value))
    # get: counts, attributes the mesh does not have
    got_v, got_t, got_n = np.empty((3, 3)), np.empty((1, 3), np.int32), np.empty((3, 3))
    get = lambda nv, nt, vn=None, tn=None: L.visma_icp_trimesh_get(ctx._h, mesh._m, got_v.ctypes.data_as(dp), vn, None, got_t.ctypes.data_as(ip), tn, nv, nt)
    assert get(3, 1) == 0 and np.array_equal(got_v, v) and got_t.tolist() == [[0, 1, 2]]
    assert get(2, 1) == INVALID and get(3, 2) == INVALID
    assert get(3, 1, vn=got_n.ctypes.data_as(dp)) == STATE and get(3, 1, tn=got_n.ctypes.data_as(dp)) == STATE
    assert L.visma_icp_trimesh_get(ctx._h, mesh._m, None, None, got_n.ctypes.data_as(dp), None, None, 3, 1) == STATE
    assert L.visma_icp_trimesh_get(ctx._h, mesh._m, None, None, None, None, None, 3, 1) == 0
    # select: an index outside [0, nv)
    for bad in ([0, 1, 3], [-1]):
        idx = np.array(bad, np.int64)
        assert L.visma_icp_trimesh_select(ctx._h, mesh._m, idx.ctypes.data_as(i64), len(idx), C.byref(out)) == INVALID and not out.value
    # NULL arguments, a mesh of another context
    assert L.visma_icp_trimesh_purge(ctx._h, None, None) == INVALID
    assert L.visma_icp_trimesh_transform(ctx._h, mesh._m, None) == INVALID
    assert L.visma_icp_trimesh_crop(ctx._h, mesh._m, None, v.ctypes.data_as(dp), C.byref(out)) == INVALID
    other = lib.Context(0)
    assert L.visma_icp_trimesh_purge(other._h, mesh._m, None) == INVALID
    assert L.visma_icp_trimesh_destroy(other._h, mesh._m) == INVALID
    # from_tsdf: before an extract, after a frame, a volume of another context
    vol = tsdf_cases.lib_volume(ctx, tsdf_cases.load("plane"))
    assert L.visma_icp_trimesh_from_tsdf(ctx._h, vol._v, C.byref(out)) == STATE and not out.value
    vol.extract_triangle_mesh()
    assert L.visma_icp_trimesh_from_tsdf(other._h, vol._v, C.byref(out)) == INVALID
    assert L.visma_icp_trimesh_from_tsdf(ctx._h, None, C.byref(out)) == INVALID
    assert L.visma_icp_trimesh_from_tsdf(ctx._h, vol._v, C.byref(out)) == 0 and out.value
    assert L.visma_icp_trimesh_destroy(ctx._h, C.c_void_p(out.value)) == 0
    vol.reset()
    assert L.visma_icp_trimesh_from_tsdf(ctx._h, vol._v, C.byref(out)) == STATE
    other.close()
    vol.close()
    assert mesh.purge() == (0, 0, 0, 0)                      # the errors left the mesh usable
    mesh.close()
