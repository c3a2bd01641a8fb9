"""The numpy specification of the TriangleMesh operations (tests/trimesh_spec.py) against the compiled reference, recorded in
tests/golden/trimesh.npz by tests/golden/gen_trimesh.py: every case and program of tests/trimesh_cases.py, bit for bit and
row for row (counts, HasX(), removed rows, the SHA-256 of the rows, and the rows themselves where the fixture holds them).
No GPU."""
import hashlib
import os

import numpy as np
import pytest

import trimesh_cases as cases
import trimesh_spec as T

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trimesh.npz"))


def test_the_fixture_covers_every_program_and_nothing_else():
    want = {"%s_%d" % item for item in cases.items()}
    have = {k.rsplit("_", 1)[0] for k in FIX.files if k.endswith("_counts")}
    assert want == have


@pytest.mark.parametrize("name,p", cases.items())
def test_the_specification_equals_the_reference(name, p):
    m, removed = cases.spec(name, p)
    key = "%s_%d_" % (name, p)
    counts = [len(m["vertices"]), len(m["triangles"]), m["vertex_normals"] is not None, m["vertex_colors"] is not None,
              m["triangle_normals"] is not None]
    assert counts == FIX[key + "counts"].tolist()
    assert list(removed) == FIX[key + "removed"].tolist()
    full = key + "vertices" in FIX.files
    assert full == (counts[0] + counts[1] <= cases.FULL_ROWS)
    if full:
        for k in T.ATTRS:
            assert (m[k] is not None) == (key + k in FIX.files), k
            if m[k] is not None:
                got, want = cases.bits(m[k]), FIX[key + k]
                assert got.dtype == want.dtype and got.shape == want.shape, k
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert len(bad) == 0, (k, bad[:5], m[k][bad[:3]])
    assert hashlib.sha256(cases.raw_rows(m)).digest() == FIX[key + "sha"].tobytes()


def test_the_rotation_key_ties():
    """the rule of TriangleMesh.cpp:235-251 on the shapes where <= decides"""
    k = T.triangle_key
    assert k((0, 1, 2)) == k((1, 2, 0)) == k((2, 0, 1)) == (0, 1, 2)
    assert k((0, 2, 1)) == (0, 2, 1)
    assert k((0, 1, 0)) == (0, 1, 0) and k((0, 0, 1)) == (0, 0, 1) and k((1, 0, 0)) == (0, 0, 1)
