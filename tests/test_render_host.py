"""visma_icp_render_host -- the renderer's arithmetic (render_math.hpp) on the host, the very functions the kernels run --
against tests/render_spec.py, bit for bit on depth, index, mask and edges over every scene of tests/render_cases.py; every
invalid argument refused with nothing written; LinearizeDepth.  No GPU."""
import numpy as np
import pytest

import render_cases as cases
import render_spec as S


@pytest.mark.parametrize("name", cases.NAMES)
def test_render_host_equals_the_specification(lib, name):
    c = cases.CASES[name]
    got = cases.host(lib, c)
    want = cases.spec_of(name)
    for g, w, what in zip(got, want, ("depth", "index", "mask", "edges")):
        assert g.dtype == w.dtype and g.shape == w.shape == (c["h"], c["w"]), what
        assert cases.bits(g).tobytes() == cases.bits(w).tobytes(), what


def test_the_cases_are_not_vacuous():
    covered = {n: int((cases.spec_of(n)[2] == 255).sum()) for n in cases.NAMES}
    assert covered["empty_mesh"] == 0 and covered["no_vertices"] == 0
    assert covered["sphere_1x1"] == 1 and covered["sphere_anchor"] == 144
    assert covered["crowd"] == 64 * 48 and covered["inside_box"] == 32 * 24
    idx = cases.spec_of("crowd")[1]
    assert (idx == 0).sum() > 1000 and len(np.unique(idx)) > 50           # the large triangle and many sub-pixel ones
    # planes: the straddling triangle and the one with a vertex behind the camera are seen (they hide the ordinary one); the
    # one behind the camera and the one beyond z_far are not
    assert set(np.unique(cases.spec_of("planes")[1]).tolist()) == {-1, 0, 1}
    assert set(np.unique(cases.spec_of("at_zero")[1]).tolist()) == {-1, 0}
    # degenerate: only the real triangle draws
    assert set(np.unique(cases.spec_of("degenerate")[1]).tolist()) == {-1, 0}
    assert set(np.unique(cases.spec_of("in_plane")[1]).tolist()) == {-1, 1}
    assert any(cases.spec_of(n)[3].any() for n in ("sphere_64x48", "sphere_close_64x48", "crowd"))
    d = cases.spec_of("sphere_anchor_depth_buffer")[0]
    assert d.max() == 1.0 and 0.0 < d.min() < 1.0


def test_the_large_scenes_are_not_vacuous():
    """What the scenes of the large path (render.hip: items of CHUNK box pixels) are there for, asserted on the spec: the
    straddling triangle's box is the whole image, it becomes the number of items its scene is named for, and in every scene
    of several items it is the visible triangle at a box pixel of a later item.  A walk that took every item for the first
    (first = 0) would never offer it there."""
    straddler = 80
    want_items = {"chunk_8x8": 0, "chunk_13x5": 1, "chunk_65x63": 1, "chunk_64x64": 1, "chunk_241x17": 2, "chunk_97x67": 2,
                  "chunk_130x100": 4}
    want_area = {"chunk_8x8": cases.SMALL_AREA, "chunk_13x5": cases.SMALL_AREA + 1, "chunk_65x63": cases.CHUNK - 1,
                 "chunk_64x64": cases.CHUNK, "chunk_241x17": cases.CHUNK + 1, "chunk_97x67": cases.CHUNK + 2403,
                 "chunk_130x100": 3 * cases.CHUNK + 712}
    assert list(cases.CHUNK_SCENES) == list(want_items)
    for name, c in cases.CHUNK_SCENES.items():
        w, h = c["w"], c["h"]
        box = cases.boxes(c)[straddler]
        assert box == (0, 0, w - 1, h - 1) and cases.box_area(box) == w * h == want_area[name], name
        assert cases.items(box) == want_items[name], name
        index = cases.spec_of(name)[1]
        at = np.flatnonzero(index.reshape(-1) == straddler)           # (the box is the image: row-major box positions)
        assert len(at) > 0 and len(np.unique(index)) > 5, name        # the sphere in front of it is seen as well
        if want_items[name] > 1:
            assert at.max() >= (want_items[name] - 1) * cases.CHUNK, name
            assert all(((at >= k * cases.CHUNK) & (at < (k + 1) * cases.CHUNK)).any() for k in range(want_items[name])), name
    assert (2403 // 256, 2403 % 256) == (9, 99)                       # chunk_97x67: nine full rounds, a break at lane 99
    # many_large: 760 triangles in three tiles, 600 of two items each between small and culled ones
    c, kinds = cases.CASES["many_large"], cases.MANY_LARGE_KINDS
    box = cases.boxes(c)
    count = np.array([cases.items(b) for b in box])
    assert len(box) == 760 == len(kinds) and -(-len(box) // cases.TILE) == 3
    assert (count[kinds == "large"] == 2).all() and (kinds == "large").sum() == 600 and count.sum() == 1200
    assert (count[kinds != "large"] == 0).all() and all(box[t] is None for t in np.flatnonzero(kinds == "culled"))
    small = [cases.box_area(box[t]) for t in np.flatnonzero(kinds == "small")]
    assert len(small) == 100 and max(small) <= cases.SMALL_AREA and sum(a > 0 for a in small) > 90
    per_tile = [set(kinds[k * cases.TILE:(k + 1) * cases.TILE].tolist()) for k in range(3)]
    assert all(s == {"large", "small", "culled"} for s in per_tile)   # interleaved
    seen = np.unique(cases.spec_of("many_large")[1])
    seen = seen[seen >= 0]
    for k in range(3):
        assert ((kinds[seen] == "large") & (seen // cases.TILE == k)).sum() >= 3, k
    assert (kinds[seen] == "small").sum() > 20 and not (kinds[seen] == "culled").any()
    assert (cases.spec_of("many_large")[2] == 255).all()


def test_the_stride_scene_on_the_host(lib):
    """2048 x 256 + 300 triangles (tests/test_render.py has what they are for): on the host, a triangle beyond 2048 x 256 and
    a large one from a compaction tile beyond 1024 are seen, and the culled crowd draws nothing: the picture is the one of the
    200 other triangles alone."""
    c, large, small = cases.stride()
    assert len(c["F"]) == cases.STRIDE_TRIANGLES == 2048 * 256 + 300 and len(c["V"]) == 700
    assert (large >= cases.STRIDE).sum() == 6 and (small >= cases.STRIDE).sum() == 10 and len(large) == 80 and len(small) == 120
    depth, index, mask, edges = cases.stride_host(lib)
    seen = np.unique(index[index >= 0])
    assert np.isin(seen, np.concatenate([large, small])).all()
    assert seen.max() > cases.STRIDE
    assert (np.isin(seen, large) & (seen // cases.TILE > 1024)).any()
    assert (np.isin(seen, large) & (seen >= cases.STRIDE)).any() and (np.isin(seen, small) & (seen >= cases.STRIDE)).any()
    assert np.isin(seen, large).sum() >= 10 and np.isin(seen, small).sum() >= 30 and (mask == 255).all()
    # the 200 alone, through the spec: the same picture, the indices renumbered
    kept = np.sort(np.concatenate([large, small]))
    d, i, m, e = cases.spec(cases.with_(c, F=c["F"][kept]))
    assert np.array_equal(np.where(i >= 0, kept[i], -1), index)
    assert cases.bits(d).tobytes() == cases.bits(depth).tobytes() and e.tobytes() == edges.tobytes()


@pytest.mark.parametrize("name,change", cases.INVALID)
def test_render_host_refuses(lib, name, change):
    c = cases.with_(cases.CASES["sphere_anchor"], **change)
    with pytest.raises(lib.IcpError) as e:
        cases.host(lib, c)
    assert e.value.code == 1


def test_render_host_writes_nothing_when_it_refuses(lib):
    import ctypes as C
    c = cases.CASES["sphere_anchor"]
    L = lib.load()
    V, F, K, E = c["V"], c["F"], np.array(c["K"]), c["E"].reshape(-1)
    n = c["w"] * c["h"]
    depth, index = np.full(n, 7.0, np.float32), np.full(n, 7, np.int32)
    mask, edges = np.full(n, 7, np.uint8), np.full(n, 7, np.uint8)
    dp, ip, fp, u8 = (C.POINTER(t) for t in (C.c_double, C.c_int32, C.c_float, C.c_uint8))
    p = lambda a, t: a.ctypes.data_as(t)

    def call(w=c["w"], h=c["h"], K=K, E=E, zn=0.05, zf=10.0, enc=0, F=F):
        return L.visma_icp_render_host(p(V, dp), len(V), p(F, ip), len(F), w, h, p(K, dp), p(E, dp), zn, zf, enc, p(depth, fp), p(index, ip),
                                       p(mask, u8), p(edges, u8))

    bad_F = F.copy(); bad_F[3, 1] = len(V)
    neg_F = F.copy(); neg_F[0, 0] = -1
    for kw in (dict(w=0), dict(h=-1), dict(zn=0.0), dict(zf=0.01), dict(enc=5), dict(K=np.array([20.3, 0.0, 1.0, 1.0])),
               dict(E=np.full(16, np.nan)), dict(F=bad_F), dict(F=neg_F)):
        assert call(**kw) == 1, kw
        assert (depth == 7.0).all() and (index == 7).all() and (mask == 7).all() and (edges == 7).all(), kw
    assert call() == 0 and (mask != 7).all()
    # each output may be NULL
    assert L.visma_icp_render_host(p(V, dp), len(V), p(F, ip), len(F), c["w"], c["h"], p(K, dp), p(E, dp), 0.05, 10.0, 0, None, None, None,
                                   None) == 0


def test_render_edges_host_equals_the_specification(lib):
    rng = np.random.default_rng(3)
    d = rng.uniform(0.5, 0.8, (12, 16)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.2] = 0.0
    d[3, 3], d[7, 9], d[5, 5] = np.nan, np.inf, -1.0
    assert lib.render_edges_host(d).tobytes() == S.edges(d).tobytes()
    assert S.edges(d).any()
    for shape in ((1, 1), (10, 40), (11, 11)):
        x = rng.uniform(0.1, 3.0, shape).astype(np.float32)
        assert lib.render_edges_host(x).tobytes() == S.edges(x).tobytes()
    # the images tests/test_render.py uploads
    d = cases.hostile_depth()
    assert lib.render_edges_host(d).tobytes() == S.edges(d).tobytes() and S.edges(d).any()
    for w, h in cases.EDGE_SHAPES:
        x = cases.stepped_depth(w, h, 5)
        assert lib.render_edges_host(x).tobytes() == S.edges(x).tobytes(), (w, h)
        assert S.edges(x).any() == (w > 10 and h > 10), (w, h)
    assert S.edges(cases.stepped_depth(11, 11, 5))[5, 5] == 255


def test_linearize_depth(lib):
    for zn, zf in ((0.05, 10.0), (0.1, 2.0)):
        for zb in (0.0, 0.25, 0.5, 0.9, 0.999, 1.0):
            assert lib.linearize_depth(zb, zn, zf) == S.linearize_depth(zb, zn, zf)
        assert lib.linearize_depth(0.0, zn, zf) == pytest.approx(zn, rel=1e-15)
        assert lib.linearize_depth(1.0, zn, zf) == pytest.approx(zf, rel=1e-15)
    # RenderDepth's encoding is what it inverts
    d = cases.host(lib, cases.CASES["sphere_anchor_depth_buffer"])[0]
    m = cases.host(lib, cases.CASES["sphere_anchor"])[0]
    on = m > 0
    back = np.array([lib.linearize_depth(float(z), 0.05, 10.0) for z in d[on]])
    assert np.all(np.abs(back - m[on]) <= 2.0 ** -23 * m[on].astype(np.float64) ** 2 * 9.95 + 1e-6)
