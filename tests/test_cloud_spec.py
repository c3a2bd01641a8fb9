"""The numpy specification of the PointCloud operations (tests/cloud_spec.py) against the compiled reference, recorded in
tests/golden/cloud.npz by tests/golden/gen_cloud.py: every case and program of tests/cloud_cases.py in the reference's own
(serial) summation order, bit for bit (counts, HasX(), the SHA-256 of rows and results, and both in full where the fixture
holds them); and the distance between that order and the library's chunked one.  No GPU."""
import hashlib
import os

import numpy as np
import pytest

import cloud_cases as cases
import cloud_spec as S

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud.npz"))
SUMS = tuple("sums%d" % n for n in cases.SUM_SIZES)


def test_the_fixture_covers_every_program_and_nothing_else():
    want = {"%s_%d" % item for item in cases.items()}
    have = {k.rsplit("_", 1)[0] for k in FIX.files if k.endswith("_counts")}
    assert want == have
    assert set(cases.NAMES) == set(cases.load())


@pytest.mark.parametrize("name,p", cases.items())
def test_the_specification_equals_the_reference(name, p):
    c, results = cases.spec(name, p)                         # chunk=None: the reference's order
    res = cases.flat_results(results)
    key = "%s_%d_" % (name, p)
    counts = [len(c["points"]), c["normals"] is not None, c["colors"] is not None, len(res)]
    assert counts == FIX[key + "counts"].tolist()
    assert (key + "points" in FIX.files) == (counts[0] <= cases.FULL_ROWS)
    if counts[0] <= cases.FULL_ROWS:
        for k in S.ATTRS:
            assert (c[k] is not None) == (key + k in FIX.files), k
            if c[k] is not None:
                got, want = cases.bits(c[k]), FIX[key + k]
                assert got.dtype == want.dtype and got.shape == want.shape, k
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert len(bad) == 0, (k, bad[:5], c[k][bad[:3]])
    assert (key + "results" in FIX.files) == (0 < len(res) <= cases.FULL_ROWS)
    if key + "results" in FIX.files:
        bad = np.nonzero(cases.bits(res) != FIX[key + "results"])[0]
        assert len(bad) == 0, (bad[:5], res[bad[:5]])
    assert hashlib.sha256(cases.raw_rows(c, results)).digest() == FIX[key + "sha"].tobytes()


def gamma(k):
    u = 2.0 ** -53
    return k * u / (1.0 - k * u)


@pytest.mark.parametrize("name", SUMS)
def test_chunked_and_serial_cumulants(name):
    """Two orders of one sum over the same rounded terms t_i differ by at most 2 gamma(n - 1) sum |t_i| (each is within
    gamma(n - 1) sum |t_i| of the exact sum: Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, which holds
    for any order of the n - 1 additions).  Derived, not measured.  Up to one chunk the two orders are the same order."""
    c, _ = cases.load()[name]
    n = len(c["points"])
    serial, chunked = S.mean_and_covariance(c)[2], S.mean_and_covariance(c, cases.CHUNK)[2]
    t = np.abs(S.cumulant_terms(c["points"])).astype(np.longdouble).sum(axis=0)      # (a bound on the bound: rounded up below)
    bound = 2.0 * gamma(n - 1) * np.asarray(t * (1.0 + 2.0 ** -50), np.float64)
    diff = np.abs(serial.astype(np.longdouble) - chunked.astype(np.longdouble)).astype(np.float64)
    print(name, "|serial - chunked| / bound:", (diff / bound).tolist())
    assert (diff <= bound).all(), (diff, bound)
    if n <= cases.CHUNK:
        assert serial.tobytes() == chunked.tobytes()
        for p in (0, 1):
            a, b = cases.spec(name, p), cases.spec(name, p, cases.CHUNK)
            assert cases.raw_rows(*a) == cases.raw_rows(*b)


def test_the_inverse_is_eigens():
    """InverseImpl.h:126-169 on a matrix with an exact inverse, and no invertibility test on a singular one"""
    m = np.array([[2.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 0.5]])
    assert S.inverse3(m).tolist() == [[0.5, 0.0, 0.0], [0.0, 0.25, 0.0], [0.0, 0.0, 2.0]]
    assert not np.isfinite(S.inverse3(np.zeros((3, 3)))).any()
