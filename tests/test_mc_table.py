"""The 256 cases of ExtractTriangleMesh's case rule (visma_icp_marching_cubes_case; visma_amd/csrc/mc_table.h) against the
numpy restatement of the rule (tests/tsdf_mesh_spec.py) and against what any closed, crack-free, consistently wound
triangulation must satisfy.  No GPU: the table is built on the host."""
import os

import numpy as np
import pytest

import tsdf_mesh_spec as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table(lib):
    return [[tuple(int(v) for v in t) for t in lib.marching_cubes_case(c)] for c in range(256)]


@pytest.fixture(scope="module")
def winding_sign():
    return int(np.load(os.path.join(HERE, "golden", "tsdf_mesh.npz"))["winding_sign"])


def face_of(e):
    """the (axis, side) faces the cube edge e lies on"""
    lower, axis = M.edge_of(e)
    return [(a, int(lower[a])) for a in range(3) if a != axis]


def boundary(tris):
    """directed edges of the triangles that no opposite edge cancels"""
    d = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    assert len(set(d)) == len(d), "a directed edge occurs twice"
    return sorted(e for e in d if (e[1], e[0]) not in d)


def test_bad_arguments(lib):
    import ctypes as C
    ids = (C.c_int32 * 15)()
    n = C.c_int(0)
    L = lib.load()
    for c in (-1, 256):
        assert L.visma_icp_marching_cubes_case(c, ids, C.byref(n)) == 1
    assert L.visma_icp_marching_cubes_case(1, None, C.byref(n)) == 1
    assert L.visma_icp_marching_cubes_case(1, ids, None) == 1


def test_equals_the_specification_entry_for_entry(table, winding_sign):
    assert winding_sign == M.WINDING_SIGN
    most = 0
    for c in range(256):
        assert table[c] == M.case_triangles(c, winding_sign), c
        most = max(most, len(table[c]))
    print("the most triangles of a case: %d" % most)
    assert most == 5
    assert table[0] == [] and table[255] == []


def test_every_cut_edge_is_used_and_nothing_else(table):
    for c in range(256):
        used = sorted({e for t in table[c] for e in t})
        assert used == M.cut_edges(c), c
        for t in table[c]:
            assert len(set(t)) == 3, c


def test_interior_edges_pair_up_and_the_rest_are_the_face_segments(table, winding_sign):
    for c in range(256):
        want = sorted(s for axis in range(3) for side in (0, 1) for s in M.face_segments(c, axis, side, winding_sign))
        got = boundary(table[c])
        assert got == want, c
        for a, b in got:                                             # ... and each lies on a face
            assert set(face_of(a)) & set(face_of(b)), (c, a, b)


def test_two_cubes_agree_on_their_common_face(table):
    """for every case A, every face of A and every case B whose opposite face has the same four signs: A's directed
    segments on the face are B's reversed (no cracks, one orientation)"""
    def on_face(c, axis, side):
        return sorted((a, b) for a, b in boundary(table[c]) if (axis, side) in face_of(a) and (axis, side) in face_of(b))

    def signs(c, axis, side):
        u, v = [a for a in range(3) if a != axis]
        out = []
        for a in (0, 1):
            for b in (0, 1):
                k = [0, 0, 0]; k[axis], k[u], k[v] = side, a, b
                out.append((c >> (k[0] + 2 * k[1] + 4 * k[2])) & 1)
        return tuple(out)

    def across(e, axis):
        """the same edge seen from the cube on the other side of the face: the lower corner's `axis` coordinate flips"""
        lower, ax = M.edge_of(e)
        lower = lower.copy(); lower[axis] ^= 1
        return M.edge_id(lower, ax)

    segs = {(c, axis, side): on_face(c, axis, side) for c in range(256) for axis in range(3) for side in (0, 1)}
    by_signs = {}
    for c in range(256):
        for axis in range(3):
            for side in (0, 1):
                by_signs.setdefault((axis, side, signs(c, axis, side)), []).append(c)
    checks = 0
    for A in range(256):
        for axis in range(3):
            for side in (0, 1):
                mine = sorted((across(b, axis), across(a, axis)) for a, b in segs[(A, axis, side)])
                for B in by_signs[(axis, 1 - side, signs(A, axis, side))]:
                    assert segs[(B, axis, 1 - side)] == mine, (A, B, axis, side)
                    checks += 1
    print("%d face pairs" % checks)
    assert checks == 256 * 6 * 16


def test_winding_of_the_single_corner_cases(table, winding_sign):
    """one inside corner: the triangle's normal points away from it (towards increasing tsdf) for winding_sign = +1"""
    for i in range(8):
        tris = table[1 << i]
        assert len(tris) == 1
        corner = M.corner_offset(i).astype(float)
        p = []
        for e in tris[0]:
            lower, axis = M.edge_of(e)
            m = lower.astype(float); m[axis] = 0.5
            p.append(m)
        n = np.cross(p[1] - p[0], p[2] - p[0])
        away = (p[0] + p[1] + p[2]) / 3.0 - corner
        assert np.sign(n @ away) == winding_sign, i
