"""open3d::VoxelDownSample (O3D/Core/Geometry/DownSample.cpp:179-220) on hostile clouds.

tests/golden/voxel_hostile.npz (tests/golden/gen_hostile.py) holds what the COMPILED Open3D returned for
clouds built to break a restatement: points exactly on voxel faces and one ulp either side of them, negative
and far coordinates, 20,000 points of mixed magnitude in one voxel, identical points, signed zeros and
denormals, a flat axis, one and two points, an extent just inside and just over the reference's only limit
(voxel * INT_MAX < extent), the two clouds of 1e20 and 1e27 grid cells that the library used to refuse, and
point counts at the block edges of the scan that numbers the voxels (2047, 2048, 2049, 2^20 + 1).  Normals
carry NaN rows and rows with one NaN component.  The inputs are regenerated from their recipes and checked
against the fixture's CRCs.

Every comparison is bit for bit (NaN equal to NaN): the oracle and the GPU against the recorded rows after a
lexicographic sort (the reference emits its hash map's order), the GPU against the oracle in the oracle's own
order (ascending (ix, iy, iz)).

Non-finite coordinates are out of scope: the reference casts floor(NaN) to int, which is undefined."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_hostile  # noqa: E402
from gen_hostile import lexsorted  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "voxel_hostile.npz"))
FAMILIES = gen_hostile.VOXEL_FAMILIES


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


_cache = {}


def case(name):
    if name not in _cache:
        _cache.clear()                                   # (one 2^20-point cloud at a time)
        _cache[name] = gen_hostile.voxel_case(name)
    return _cache[name]


def recorded(name):
    return G[name + "_p"], G[name + "_n"], G[name + "_c"]


def live_checks():
    """tests/golden/live_checks.npz as it is: (xyz, normals with NaN rows, [(voxel, points, normals)])."""
    g = np.load(os.path.join(HERE, "golden", "live_checks.npz"))
    return g["voxel_xyz"], g["voxel_normals"], [(float(g["voxel_size_%d" % i][0]), g["voxel_p_%d" % i], g["voxel_n_%d" % i])
                                                for i in range(3)]


@pytest.mark.parametrize("name", FAMILIES)
def test_fixture_inputs_regenerate_bit_for_bit(name):
    p, nrm, col, voxel = case(name)
    assert np.array_equal(gen_hostile.crcs(p, nrm, col), G[name + "_crc"])
    assert voxel == float(G[name + "_voxel"])
    assert np.isfinite(p).all() and np.isnan(nrm).any()


def test_fixture_covers_what_it_claims():
    for name in FAMILIES:
        p, _, _, voxel = case(name)
        n_out = len(G[name + "_p"])
        ext = (p.max(0) - p.min(0)).max() + voxel
        cells = np.prod(np.floor((p.max(0) - p.min(0) + 0.5 * voxel) / voxel) + 2.0)
        assert (cells >= 4e18) == (name in gen_hostile.VOXEL_WIDE or name == "over_limit"), (name, cells)
        if name == "over_limit":
            assert voxel * gen_hostile.INT_MAX < ext and n_out == 0
        else:
            assert voxel * gen_hostile.INT_MAX >= ext and 0 < n_out <= len(p)
    assert len(G["one_voxel_20k_p"]) == 1 and len(G["identical_3000_p"]) == 1 and len(G["n2_p"]) == 2
    assert 3000 < len(G["wide_2e-4_p"]) < len(G["wide_1e-6_p"]) == 3500          # the tight cluster splits as the voxel shrinks
    p = case("faces")[0]
    on_face = ((p + 0.125) / 0.25 == np.round((p + 0.125) / 0.25)).all(1)
    assert on_face.sum() >= 200 and (~on_face).sum() >= 200


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_matches_recorded_reference(oracle, name):
    p, nrm, col, voxel = case(name)
    got = oracle.voxel_down_sample(p, voxel, nrm, col)
    exp = recorded(name)
    assert len(got[0]) == len(exp[0])
    if len(exp[0]):
        got = lexsorted(*got)
    assert same(got[0], exp[0]) and same(got[1], exp[1]) and same(got[2], exp[2])
    only = oracle.voxel_down_sample(p, voxel)[0]         # points alone: the same points
    assert same(lexsorted(only)[0] if len(only) else only, exp[0])


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_matches_live_reference(oracle, ref, name):
    p, nrm, col, voxel = case(name)
    got = oracle.voxel_down_sample(p, voxel, nrm, col)
    exp = ref.voxel_down_sample(p, voxel, nrm, col)
    assert len(got[0]) == len(exp[0])
    if len(exp[0]):
        got, exp = lexsorted(*got), lexsorted(*exp)
    assert same(got[0], exp[0]) and same(got[1], exp[1]) and same(got[2], exp[2])
    assert same(exp[0], G[name + "_p"])                  # the fixture is what the reference still returns


# ---------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", FAMILIES)
def test_gpu_matches_oracle_and_reference(gpu_ctx_auto, oracle, name):
    ctx = gpu_ctx_auto
    p, nrm, col, voxel = case(name)
    exp = recorded(name)
    o = oracle.voxel_down_sample(p, voxel, nrm, col)
    # points + normals + colours
    got = ctx.voxel_down_sample(p, voxel, nrm, col)
    assert same(got[0], o[0]) and same(got[1], o[1]) and same(got[2], o[2])            # the oracle's order
    if len(exp[0]):
        got = lexsorted(*got)
    assert same(got[0], exp[0]) and same(got[1], exp[1]) and same(got[2], exp[2])      # Open3D's rows
    # points alone
    got = ctx.voxel_down_sample(p, voxel)
    assert got[1] is None and got[2] is None
    assert same(got[0], o[0])
    assert same(lexsorted(got[0])[0] if len(exp[0]) else got[0], exp[0])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", FAMILIES)
def test_gpu_voxel_target_made_on_the_device(lib, oracle, name):
    """visma_icp_set_clouds_f64_voxel_target + visma_icp_get_voxel_target: the same points as the oracle, in its order
    (over_limit: an empty target, nt == 0, as the reference returns an empty cloud)."""
    p, _, _, voxel = case(name)
    o = oracle.voxel_down_sample(p, voxel)[0]
    ctx = lib.Context(0)
    try:
        nt = ctx.set_clouds_f64_voxel_target(p[:64], p, voxel)
        assert nt == len(o) == len(G[name + "_p"])
        assert (nt == 0) == (name == "over_limit")
        got = ctx.get_voxel_target(nt)
    finally:
        ctx.close()
    assert got.shape == (nt, 3) and same(got, o)
    assert same(lexsorted(got)[0] if nt else got, G[name + "_p"])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_gpu_live_checks_with_nan_normals(gpu_ctx_auto, oracle):
    """The cloud of tests/golden/live_checks.npz (every 97th normal NaN), until now run on the CPU oracle only."""
    xyz, nrm, cases = live_checks()
    assert np.isnan(nrm).any()
    for voxel, rp, rn in cases:
        got = gpu_ctx_auto.voxel_down_sample(xyz, voxel, nrm, None)
        o = oracle.voxel_down_sample(xyz, voxel, nrm, None)
        assert got[2] is None and same(got[0], o[0]) and same(got[1], o[1])
        a, b = lexsorted(got[0], got[1]), lexsorted(rp, rn)
        assert same(a[0], b[0]) and same(a[1], b[1])
