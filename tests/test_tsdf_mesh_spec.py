"""The numpy specification of ExtractTriangleMesh (tests/tsdf_mesh_spec.py) against the compiled reference
(tests/golden/tsdf_mesh.npz, written by tests/golden/gen_tsdf_mesh.py).  No GPU.

The volumes are re-integrated by tests/tsdf_spec.py, which gives the reference's voxels bit for bit (tests/test_tsdf.py; the
generator asserts it for these cases too).  Which valid cubes there are, which edges carry a vertex and every vertex's
position and colour do not depend on the case table: the [vertex | colour] rows are the reference's bit for bit as a
multiset, in EVERY case.  Where no valid cube has a diagonally signed face (tsdf_mesh_cases.UNAMBIGUOUS) every cube's patch
has one boundary whatever table cuts it into triangles: triangle count, V - E + F and the mesh boundary are the reference's.
Elsewhere (AMBIGUOUS: the made-up checkerboard frame, and every scene case with a depth discontinuity) the rule joins the
edges of such cubes in its own way: there the mesh must be an oriented manifold with boundary, and the counts are printed."""
import hashlib
import os

import numpy as np
import pytest

import tsdf_mesh_cases as cases
import tsdf_mesh_spec as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "tsdf_mesh.npz"))
    return {k: g[k] for k in g.files}


_MESHES = {}


def spec_mesh(name):
    """computed once per case, shared and left unchanged -> case, vertices, colors, triangles, rising"""
    if name not in _MESHES:
        case = cases.load(name)
        vol = cases.spec_volume(case)
        _MESHES[name] = (case,) + tuple((M.extract_scalable if case["scalable"] else M.extract_uniform)(vol, with_edges=True))
    return _MESHES[name]


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).digest(), np.uint8)


def check_rows(golden, name, vertices, colors):
    rows = M.sort_rows_bits(vertices, colors) if colors is not None else M.sort_rows_bits(vertices)
    assert len(rows) == int(golden[name + "_nv"])
    assert np.array_equal(sha(rows), golden[name + "_rows_sha"]), name
    if name + "_rows" in golden:
        assert np.array_equal(rows.view(np.uint64), golden[name + "_rows"].view(np.uint64))


def check_oriented_manifold(vertices, tri):
    """every directed edge at most once (so an undirected edge has at most two triangles, wound oppositely), indices in range"""
    assert tri.min() >= 0 and tri.max() < len(vertices)
    d = M.directed_edges(tri)
    assert len(np.unique(d, axis=0)) == len(d)


@pytest.mark.parametrize("name", cases.NAMES)
def test_vertices_and_colours_are_the_references(golden, name):
    case, vertices, colors, tri, _ = spec_mesh(name)
    assert (colors is None) == (case["color_type"] == 0)
    check_rows(golden, name, vertices, colors)
    assert int(golden["winding_sign"]) == M.WINDING_SIGN


@pytest.mark.parametrize("name", cases.UNAMBIGUOUS)
def test_unambiguous_meshes_equal_the_references_up_to_diagonals(golden, name):
    case, vertices, colors, tri, rising = spec_mesh(name)
    assert int(golden[name + "_ambiguous"]) == 0
    assert len(tri) == int(golden[name + "_nt"])
    euler, boundary, repeated = M.mesh_stats(vertices, tri)
    assert euler == int(golden[name + "_euler"])
    assert repeated == 0
    check_oriented_manifold(vertices, tri)
    assert len(boundary) == int(golden[name + "_boundary_n"])
    assert np.array_equal(sha(boundary), golden[name + "_boundary_sha"])
    if name + "_boundary" in golden:
        assert np.array_equal(boundary.view(np.uint64), golden[name + "_boundary"].view(np.uint64))
    dots, flat = M.winding_dots(vertices, tri, rising)
    print("%s: %d triangles, %d of zero area, min |normal . direction| / voxel^2 %.3g" % (name, len(tri), flat, np.abs(dots).min() / case["voxel_length"] ** 2))
    assert (np.sign(dots) == int(golden["winding_sign"])).all()
    if name == "plane":
        assert flat > 0                                                  # degenerate triangles are kept


@pytest.mark.parametrize("name", cases.AMBIGUOUS)
def test_ambiguous_meshes_are_oriented_manifolds(golden, name):
    case, vertices, colors, tri, rising = spec_mesh(name)
    assert int(golden[name + "_ambiguous"]) >= (8 if name == "ambig" else 1)
    check_oriented_manifold(vertices, tri)
    print("%s: %d ambiguous cubes; triangles: the specification %d, the reference %d" % (name, int(golden[name + "_ambiguous"]), len(tri), int(golden[name + "_nt"])))
    assert len(np.unique(tri)) == len(vertices)                          # every vertex is used


def test_order_is_the_documented_one():
    """vertices ascend by (x, y, z, axis) -- ExtractPointCloud's order; a vertex belongs to exactly one voxel edge"""
    case, vertices, colors, tri, rising = spec_mesh("u21")
    vl, origin = case["voxel_length"], np.array(case["origin"])
    q = (vertices - origin) / vl - 0.5
    axis = np.argmax(np.abs(rising), 1)
    lower = np.floor(q + 1e-9).astype(int)                               # (no vertex of u21 sits on a voxel: no tsdf is 0)
    key = [tuple(r) for r in np.concatenate([lower, axis[:, None]], 1).tolist()]
    assert key == sorted(key)
