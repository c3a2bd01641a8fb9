"""The numpy specification of the Image operations (tests/image_spec.py) against the compiled reference, recorded in
tests/golden/image.npz by tests/golden/gen_image.py: every case of tests/image_cases.py bit for bit (formats, the SHA-256 of
all registers and results, and both in full where the fixture holds them), every NaN as one pattern; and the cases in which
the reference has undefined behaviour against what include/visma_icp.h states.  No GPU."""
import os

import numpy as np
import pytest

import image_cases as cases
import image_spec as S

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image.npz"))


def test_the_fixture_covers_every_case_and_nothing_else():
    have = {k[:-len("_info")] for k in FIX.files if k.endswith("_info")}
    assert have == set(cases.NAMES)
    assert not set(cases.NAMES) & set(cases.SPEC_ONLY)
    for k in FIX.files:
        name = next(n for n in sorted(cases.NAMES, key=len, reverse=True) if k.startswith(n + "_"))
        rest = k[len(name) + 1:]
        assert rest in ("info", "sha", "results") or (rest.startswith("px") and rest[2:].isdigit()), k


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_specification_equals_the_reference(name):
    regs, results = cases.spec(name)
    assert cases.infos(regs).tolist() == FIX[name + "_info"].tolist()
    for k, r in enumerate(regs):
        key = "%s_px%d" % (name, k)
        assert (key in FIX.files) == (0 < r.nbytes <= cases.FULL_BYTES), key
        if key in FIX.files:
            got, want = cases.bits(r), FIX[key]
            assert got.dtype == want.dtype and got.shape == want.shape, key
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (key, bad[:5].tolist(), [r[tuple(i)] for i in bad[:5]])
    assert (name + "_results" in FIX.files) == (len(results) > 0)
    if len(results):
        bad = np.nonzero(cases.bits(results) != FIX[name + "_results"])[0]
        assert len(bad) == 0, (bad[:5], results[bad[:5]])
    assert cases.digest(regs, results).tobytes() == FIX[name + "_sha"].tobytes()


def test_from_float_saturates_outside_the_casts_domain():
    """visma_icp.h: NaN and negatives give 0, values beyond the maximum the maximum"""
    inputs, _ = cases.case("from_float_saturated")
    regs, _ = cases.spec("from_float_saturated")
    assert not S.in_cast_domain(inputs[0], 1)[0, :7].any() and not S.in_cast_domain(inputs[1], 2)[0, :7].any()
    assert regs[2].dtype == np.uint8 and regs[2][0].tolist() == [0, 0, 0, 255, 255, 0, 255, 0]
    assert regs[3].dtype == np.uint16 and regs[3][0].tolist() == [0, 0, 0, 65535, 65535, 0, 65535, 65535]


def test_nyu_saturates_at_65535_which_the_truncation_zeroes():
    """visma_icp.h: swapped raw values 1088 .. 1092 are beyond 65535 mm: saturated, then 65.535 m >= 7 m gives 0"""
    inputs, _ = cases.case("nyu_saturated")
    assert S.nyu_defined(inputs[1])[0].tolist() == [False] * 5 + [True]
    assert S.decode_nyu(inputs[1])[0].tolist() == [65535] * 5 + [63873]
    regs, _ = cases.spec("nyu_saturated")
    assert regs[3].dtype == np.float32 and not regs[3].any()
    assert regs[1].tobytes() == inputs[1].tobytes()          # the input is left as it is


def test_float_value_at_answers_false_where_the_reference_is_undefined():
    """visma_icp.h: an image narrower or lower than 2 pixels, and a NaN coordinate: (false, 0)"""
    _, results = cases.spec("value_at_undefined")
    ok = results.reshape(3, 2, 4)[:, 0]
    value = results.reshape(3, 2, 4)[:, 1]
    assert not ok[0].any() and not ok[1].any() and ok[2].tolist() == [1, 1, 0, 0]
    assert value[2].tolist() == [1.0, 1.0, 0.0, 0.0] and not value[:2].any()
