"""Point -> mesh distance (the body of feh::MeasureSurfaceError, include/geometry.h:117-141) on hostile meshes.

tests/golden/mesh_hostile.npz (tests/golden/gen_hostile.py) holds what the COMPILED libigl
(igl::AABB::squared_distance) returned, and for the first queries of every family the EXACT squared distance
(tests/exact_geometry.py: rational arithmetic on the f64 inputs).  Families: needle soups of thickness 1 .. 1e-12
and 0 times their length at offsets 0 and 100, a flat grid, the same queried in its own plane, a bumpy grid, the
same rotated and moved by 1e3, 200 faces with one centroid, two giant faces over 1,152 small ones, a far
unreferenced vertex, duplicated and zero-area faces, vertices at +-1e6, face counts at the edges of the search
structure (kLeaf = 4, the 64-face switch, powers of two) and query counts at the edges of the launch (64 lanes,
the 4096-query sorted path).  Queries lie on faces, edges and vertices, 1e-9 .. 1 extents off the surface, 1e3
extents away, and come with exact duplicates.

Bars (none of them a tolerance):
  * d2 is bit-equal to libigl's on EVERY row -- oracle and GPU;
  * face and closest point are bit-equal to the oracle's on every row (GPU), and to libigl's wherever libigl's
    face is the oracle's.  Where the faces differ the tie must be real (the oracle's distance to libigl's face
    alone is the same d2, bit for bit) and the oracle's face the lowest index at that d2; the share of such rows
    may not exceed what the generator saw;
  * against the exact yardstick the oracle is never further from the truth than libigl, query by query;
  * brute force, BVH and "auto" agree bit for bit, with and without NaN / inf query rows.

How far the shared f64 arithmetic (Ericson's region walk) is from the exact distance on needles is MEASURED, not
asserted: `needle_table` in the fixture, quoted in DESIGN.md."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import exact_geometry  # noqa: E402
import gen_hostile  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "mesh_hostile.npz"))
FAMILIES = gen_hostile.MESH_FAMILIES
MODES = ("brute", "bvh", "auto")

_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = gen_hostile.mesh_case(name)
    return _cache[name]


def F_(x):
    return Fraction(float(x))


# ---------------------------------------------------------------------------------------------------------
# the exact yardstick itself
# ---------------------------------------------------------------------------------------------------------
def test_exact_voronoi_regions_of_the_unit_right_triangle():
    a, b, c = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    Q = Fraction
    cases = [((-1, -1, 0.5), Q(9, 4)),           # vertex a
             ((2, -1, 0), Q(2)),                 # vertex b
             ((-1, 2, 0), Q(2)),                 # vertex c
             ((0.5, -1, 0), Q(1)),               # edge ab
             ((-1, 0.5, 0), Q(1)),               # edge ca
             ((1, 1, 0), Q(1, 2)),               # edge bc
             ((0.25, 0.25, 3.0), Q(9)),          # interior
             ((0.75, 0.75, 0.5), Q(1, 8) + Q(1, 4)),        # edge bc, off the plane
             ((0.25, 0.25, 0), Q(0))]
    for p, d in cases:
        assert exact_geometry.point_triangle_sqdist(p, a, b, c) == d, p
    # inputs are taken as the f64 they are: 0.1 is not 1/10
    assert exact_geometry.point_triangle_sqdist((0.1, 0.1, 1), a, b, c) == 1
    assert exact_geometry.point_triangle_sqdist((-0.1, 0.5, 0), a, b, c) == F_(0.1) ** 2


def test_exact_zero_area_faces():
    p = (0.5, 1.0, 0.0)
    assert exact_geometry.point_triangle_sqdist(p, (0, 0, 0), (0, 0, 0), (0, 0, 0)) == Fraction(5, 4)       # a point
    assert exact_geometry.point_triangle_sqdist(p, (0, 0, 0), (2, 0, 0), (0, 0, 0)) == 1                    # a segment
    assert exact_geometry.point_triangle_sqdist(p, (0, 0, 0), (2, 0, 0), (1, 0, 0)) == 1                    # collinear
    assert exact_geometry.point_triangle_sqdist((3, 1, 0), (0, 0, 0), (2, 0, 0), (1, 0, 0)) == 2            # past its end
    assert exact_geometry.point_segment_sqdist((3, 1, 0), (0, 0, 0), (2, 0, 0)) == 2
    d2, faces = exact_geometry.point_mesh_sqdist([p], [[0, 0, 0], [2, 0, 0], [1, 0, 0], [0, 5, 5]],
                                                 [[0, 1, 2], [3, 3, 3], [0, 0, 1], [2, 1, 0]])
    assert d2 == [1] and faces == [[0, 2, 3]]              # every face that attains the minimum


def test_exact_is_invariant_under_vertex_permutation():
    rng = np.random.default_rng(3)
    for _ in range(40):
        a, b, c, p = rng.standard_normal((4, 3)) * rng.choice([1e-6, 1.0, 1e6])
        if rng.random() < 0.3:
            c = a + (b - a) * rng.random() + rng.standard_normal(3) * 1e-13        # a needle
        d = exact_geometry.point_triangle_sqdist(p, a, b, c)
        for x, y, z in ((a, c, b), (b, a, c), (b, c, a), (c, a, b), (c, b, a)):
            assert exact_geometry.point_triangle_sqdist(p, x, y, z) == d


def test_exact_agrees_with_the_oracle_on_a_well_shaped_mesh(oracle):
    V, F, P = case("bumpy_grid")
    P = P[:60]
    d2, face, _ = oracle.point_mesh_sqdist(P, V, F)
    ex, faces = exact_geometry.point_mesh_sqdist(P, V, F)
    ex_all, faces_all = exact_geometry.point_mesh_sqdist(P[:6], V, F, prefilter=False)
    assert ex_all == ex[:6] and faces_all == faces[:6]     # the prefilter drops no face that matters
    scale = gen_hostile.coordinate_scale(P, V, F)          # max |coordinate| of the mesh and of the query
    for i in range(len(P)):
        # a few units of eps * max|coordinate| on the DISTANCE: |d2 - ex| <= units * eps * scale * (2 d + ...)
        d = np.sqrt(d2[i])
        bound = 8 * gen_hostile.EPS * scale[i]
        assert abs(F_(d2[i]) - ex[i]) <= F_(bound * (2 * d + bound)), i
        assert face[i] in faces[i] or abs(F_(d2[i]) - ex[i]) > 0


# ---------------------------------------------------------------------------------------------------------
# CPU: the oracle against libigl (recorded, and live where oracle/_ref is built) and against the yardstick
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_fixture_inputs_regenerate_bit_for_bit(name):
    V, F, P = case(name)
    assert np.array_equal(gen_hostile.crcs(V, F, P), G[name + "_crc"])
    assert len(G[name + "_d2"]) == len(P) and len(G[name + "_ex"]) == gen_hostile.n_exact(name)
    assert len(np.unique(P, axis=0)) < len(P)            # exact duplicates among the queries


def test_fixture_covers_the_structure_edges():
    assert [len(case("nf%d" % n)[1]) for n in gen_hostile.NF_EDGES] == list(gen_hostile.NF_EDGES)
    assert {1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097} <= set(gen_hostile.NF_EDGES)
    assert gen_hostile.NP_EDGES == (1, 63, 64, 65, 4095, 4096, 4097) and len(case("np_edges")[2]) == 4097
    V, F, P = case("planar_inplane")
    assert np.ptp(V[:, 2]) == 0 and (P[:, 2] == V[0, 2]).all()
    assert np.abs(case("pm1e6")[0]).min() > 9e5
    V, F, _ = case("far_vertex")
    assert np.abs(V).max() == 1e9 and np.abs(V[np.unique(F)]).max() <= 1.0
    V, F, _ = case("dup_zero_area")
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    assert (np.cross(b - a, c - a) == 0).all(1).sum() >= 40 and len(np.unique(F, axis=0)) < len(F)
    V, F, _ = case("shared_centroid")
    assert np.abs(V[F].mean(1) - [0.3, 0.2, 0.1]).max() < 1e-14


def _check_against_igl(oracle, name, igl_d2, igl_face, igl_cl):
    V, F, P = case(name)
    d2, face, cl = oracle.point_mesh_sqdist(P, V, F)
    assert np.array_equal(d2, igl_d2)                    # every row, no excuses
    diff = np.nonzero(face != igl_face)[0]
    agree = face == igl_face
    assert np.array_equal(cl[agree], igl_cl[agree])
    assert np.mean((cl != igl_cl).any(1)) <= G[name + "_ties"][1]
    assert np.mean(face != igl_face) <= G[name + "_ties"][0]
    for i in diff:
        # the tie is real: libigl's face alone gives the same d2 ...
        one = oracle.point_mesh_sqdist(P[i:i + 1], V, F[igl_face[i]:igl_face[i] + 1])[0][0]
        assert one == d2[i], (name, i)
        # ... and the oracle's face is the lowest index that does: the faces before it are strictly farther
        assert face[i] < igl_face[i]
        if face[i] > 0:
            before = oracle.point_mesh_sqdist(P[i:i + 1], V, F[:face[i]])[0][0]
            assert before > d2[i], (name, i)
    return d2


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_matches_recorded_igl(oracle, name):
    _check_against_igl(oracle, name, G[name + "_d2"], G[name + "_face"], G[name + "_cl"])


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_matches_live_igl(oracle, ref, name):
    V, F, P = case(name)
    d2, face, cl = ref.point_mesh_sqdist(P, V, F)
    assert np.array_equal(d2, G[name + "_d2"]) and np.array_equal(face, G[name + "_face"])   # the fixture is current
    _check_against_igl(oracle, name, d2, face, cl)


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_is_never_further_from_the_truth_than_igl(oracle, name):
    """|d2_oracle - d2_exact| <= |d2_igl - d2_exact| per query, in exact arithmetic on the recorded values; and the
    recorded yardstick is what tests/exact_geometry.py computes (a sample of it: Fractions are slow)."""
    V, F, P = case(name)
    ex = G[name + "_ex"]
    d2 = oracle.point_mesh_sqdist(P[:len(ex)], V, F)[0]
    for i in range(len(ex)):
        assert abs(F_(d2[i]) - F_(ex[i])) <= abs(F_(G[name + "_d2"][i]) - F_(ex[i])), (name, i)
    k = np.arange(0, len(ex), max(len(ex) // 4, 1))[:4]
    live, faces = exact_geometry.point_mesh_sqdist(P[k], V, F)
    assert [float(x) for x in live] == list(ex[k])
    assert all(len(f) >= 1 for f in faces)


# a face whose first two vertices coincide: igl::point_simplex_squared_distance guards the edge-ab region with a != b
# (0 / 0 otherwise), and so must every restatement -- found by the +-1e6 family (row 98, face [135, 135, 181])
AB_V = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [5.0, 5.0, 5.0], [5.0, 6.0, 5.0], [6.0, 5.0, 5.0]])
AB_F = np.array([[3, 4, 5], [0, 1, 2], [0, 0, 2], [1, 0, 2]], np.int32)
AB_P = np.array([[0.5, 1.0, 0.0], [0.25, 0.0, 0.5], [-1.0, 0.0, 0.0], [2.0, 1.0, 0.0]])
AB_D2 = np.array([1.0, 0.25, 1.0, 2.0])


def test_oracle_face_with_coincident_first_vertices(oracle):
    ex, faces = exact_geometry.point_mesh_sqdist(AB_P, AB_V, AB_F)
    assert [float(e) for e in ex] == list(AB_D2) and all(f == [1, 2, 3] for f in faces)
    d2, face, cl = oracle.point_mesh_sqdist(AB_P, AB_V, AB_F)
    assert np.array_equal(d2, AB_D2) and (face == 1).all()
    assert np.array_equal(cl, [[0.5, 0, 0], [0.25, 0, 0], [0, 0, 0], [1, 0, 0]])


def test_needle_table_is_what_the_fixture_holds():
    """The one measured quantity: libigl's distance error on needles against the exact distance, recomputed from the
    recorded d2 and exact values (NOT from any implementation under test, and not compared with a constant)."""
    table = G["needle_table"]
    assert [r[0] for r in table] == list(gen_hostile.NEEDLE_THICKNESS)
    assert np.array_equal(gen_hostile.needle_table(G), table)          # every column, exactly


# ---------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------
def _all_modes(ctx, P, V, F):
    out = {}
    try:
        for m in MODES:
            ctx.set_mesh_search(m)
            out[m] = tuple(np.copy(x) for x in ctx.point_mesh_distance(P, V, F))
    finally:
        ctx.set_mesh_search("auto")
    return out


def _same3(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", FAMILIES)
def test_gpu_matches_oracle_and_igl(gpu_ctx_auto, oracle, name):
    V, F, P = case(name)
    od2, oface, ocl = oracle.point_mesh_sqdist(P, V, F)
    got = _all_modes(gpu_ctx_auto, P, V, F)
    for m in MODES:
        d2, face, cl = got[m]
        assert np.array_equal(d2, G[name + "_d2"]), m                # libigl's d2, every row
        assert np.array_equal(d2, od2), m
        assert np.array_equal(face, oface), m                        # lowest face index on exact ties
        assert np.array_equal(cl, ocl), m
        agree = face == G[name + "_face"]
        assert np.mean(face != G[name + "_face"]) <= G[name + "_ties"][0]       # (the generator's own expression)
        assert np.array_equal(cl[agree], G[name + "_cl"][agree]), m
    assert _same3(got["bvh"], got["brute"]) and _same3(got["auto"], got["brute"])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_gpu_face_with_coincident_first_vertices(gpu_ctx_auto, oracle):
    exp = oracle.point_mesh_sqdist(AB_P, AB_V, AB_F)
    got = _all_modes(gpu_ctx_auto, AB_P, AB_V, AB_F)
    for m in MODES:
        assert np.array_equal(got[m][0], AB_D2) and _same3(got[m], exp), m


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("np_", gen_hostile.NP_EDGES)
def test_gpu_query_counts_at_the_launch_edges(gpu_ctx_auto, oracle, np_):
    V, F, P = case("np_edges")
    P = P[:np_]
    od2, oface, ocl = oracle.point_mesh_sqdist(P, V, F)
    got = _all_modes(gpu_ctx_auto, P, V, F)
    for m in MODES:
        assert np.array_equal(got[m][0], G["np_edges_d2"][:np_]), m
        assert _same3(got[m], (od2, oface, ocl)), m
        agree = got[m][1] == G["np_edges_face"][:np_]
        assert np.array_equal(got[m][2][agree], G["np_edges_cl"][:np_][agree]), m


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", FAMILIES)
def test_gpu_non_finite_query_rows(gpu_ctx_auto, name):
    """NaN and +-inf query rows (tests/test_cloud_distance.py::test_nan_rows is the model): the two searches agree
    on them, and every finite row is what it is without them."""
    V, F, P = case(name)
    bad = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.nan] * 3, [np.inf, 0, 0], [0, -np.inf, 0],
                    [np.inf, np.inf, np.inf], [-np.inf, np.inf, 0.5], [np.inf, np.nan, 0]])
    at = np.sort(np.random.default_rng(len(P)).integers(0, len(P) + 1, len(bad)))
    Q = np.insert(P, at, bad, axis=0)
    finite = np.isfinite(Q).all(1)
    assert finite.sum() == len(P) and np.array_equal(Q[finite], P)
    clean = _all_modes(gpu_ctx_auto, P, V, F)
    dirty = _all_modes(gpu_ctx_auto, Q, V, F)
    for m in MODES:
        assert _same3(dirty[m], dirty["brute"]), m                   # on every row, the non-finite ones included
        assert _same3(tuple(x[finite] for x in dirty[m]), clean[m]), m
        assert not np.isfinite(dirty[m][0][~finite]).any()           # no finite distance from a non-finite query


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_gpu_bvh_equals_brute_force_on_200k_needles(gpu_ctx_auto):
    V, F, P = gen_hostile.large_case()
    assert len(F) >= 200000 and len(P) == 100000
    assert np.array_equal(gen_hostile.crcs(V, F, P), G["large_crc"])
    got = {}
    try:
        for m in ("bvh", "brute"):
            gpu_ctx_auto.set_mesh_search(m)
            got[m] = tuple(np.copy(x) for x in gpu_ctx_auto.point_mesh_distance(P, V, F))
    finally:
        gpu_ctx_auto.set_mesh_search("auto")
    bad = np.nonzero((got["bvh"][0] != got["brute"][0]) | (got["bvh"][1] != got["brute"][1]))[0]
    print("200k needles: %d of %d rows differ between BVH and brute force" % (len(bad), len(P)), bad[:10],
          got["bvh"][1][bad[:10]], got["brute"][1][bad[:10]])
    assert _same3(got["bvh"], got["brute"])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("pair", sorted(gen_hostile.MSE_PAIRS))
def test_gpu_measure_surface_error_equals_igl(gpu_ctx_auto, oracle, pair):
    """test_mesh.py::test_gpu_measure_surface_error with libigl's distances in place of the oracle's: the samples are
    the device's Philox draws (restated in gen_hostile.philox_uniforms, checked here), the distances libigl's."""
    Vs, Fs, Vt, Ft, pts, n, seed = gen_hostile.mse_samples(oracle, pair)
    assert np.array_equal(gen_hostile.crcs(pts), G["mse_%s_crc" % pair])
    assert np.array_equal(gpu_ctx_auto.sample_mesh(Vs, Fs, n, quirks=False, seed=seed), pts)
    exp = oracle.error_metric(np.sqrt(G["mse_%s_d2" % pair]))
    for m in MODES:
        gpu_ctx_auto.set_mesh_search(m)
        try:
            got = gpu_ctx_auto.measure_surface_error(Vs, Fs, Vt, Ft, n, quirks=False, seed=seed)
        finally:
            gpu_ctx_auto.set_mesh_search("auto")
        for k in exp:
            assert got[k] == exp[k], (m, k)
