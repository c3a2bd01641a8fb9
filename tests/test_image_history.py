"""One resident Image and one context through a mixed history of calls against fresh ones (tests/history.py): the in-place
operations, filters of different lengths (the cached weight buffer of the image changes size), pyramids of different depths, a
hand-off into a volume between two filters and an odometry prepare between two pyramids.  A call's result depends on the
image's pixels and the call's arguments, never on what the object -- its grow-only scratch buffers, its weight buffer -- or
the context computed before.  GPU against GPU: raw bytes."""
import numpy as np
import pytest

import image_cases as cases
import image_spec as S
import odometry_scene
import tsdf_scene
from history import replay


class Slot:
    """the one context of a history and its one image"""

    def __init__(self, lib, first):
        self.ctx = lib.Context(0)
        self.image = self.ctx.image(first)

    def put(self, a):
        self.image.close()
        self.image = self.ctx.image(a)

    def close(self):
        self.ctx.close()


def taken(images):
    out = [(i.info(), i.get()) for i in images]
    for i in images:
        i.close()
    return out


@pytest.mark.gpu
def test_image_history(lib):
    frames, k = tsdf_scene.frames(64, 48, 1)
    depth, rgb, gray, E = frames[0]
    sg, sd, tg, td, ko = odometry_scene.frames(64, 48)
    first = np.ascontiguousarray(depth)
    states = {}
    long_a = [((i * 11) % 7 - 3) / 13.0 for i in range(31)]
    long_b = cases.TAPS71

    def in_place(slot):
        slot.image.linear_transform(0.37, 0.05)
        slot.image.clip_intensity(0.2, 0.9)
        states["clipped"] = slot.image.get()
        return states["clipped"]

    def filters(slot):
        out = taken([slot.image.filter_horizontal(long_a), slot.image.filter("gaussian7"), slot.image.filter_separable(long_b, long_a),
                     slot.image.filter_horizontal(cases.TAPS9), slot.image.filter_separable([0.3], long_b)])
        return out

    def deep_pyramid(slot):
        return taken(slot.image.pyramid(6, True))

    def integrate_between_filters(slot):
        a = taken([slot.image.filter("gaussian5")])
        vol = slot.ctx.tsdf_uniform(2.0, 32, 0.1, lib.TSDF_COLOR_GRAY32, origin=(-1.0, -1.0, -1.0))
        with slot.ctx.image(depth) as d, slot.ctx.image(gray) as g:
            vol.integrate(d, g, k, E)
        v = vol.volume()
        vol.close()
        b = taken([slot.image.filter_separable(long_a, [1.0]), slot.image.flip(), slot.image.downsample()])
        return a, v, b

    def prepare_between_pyramids(slot):
        a = taken(slot.image.pyramid(2, False))
        imgs = [slot.ctx.image(x) for x in (sg, sd, tg, td)]
        slot.ctx.odometry_prepare(*imgs, ko, option=lib.odometry_option(iterations=(1, 1)))
        levels = taken([slot.ctx.image_from_odometry(w, l) for l in range(2) for w in range(8)])
        for i in imgs:
            i.close()
        b = taken(slot.image.pyramid(4, True))
        ok, value = slot.image.float_value_at([(1.5, 2.25), (63.0, 47.0), (64.0, 1.0)])
        return a, levels, b, ok, value

    fresh = replay(lambda: Slot(lib, first), [
        ("linear_transform and clip_intensity", None, in_place),
        ("filters of 31, 7, 71 x 31, 9 and 1 x 71 taps", lambda slot: slot.put(states["clipped"]), filters),
        ("a pyramid of six levels", lambda slot: slot.put(states["clipped"]), deep_pyramid),
        ("an integration between two filters", lambda slot: slot.put(states["clipped"]), integrate_between_filters),
        ("an odometry prepare between two pyramids", lambda slot: slot.put(states["clipped"]), prepare_between_pyramids)])
    # the history is not vacuous, and its first steps are the specification's
    want = S.clip_intensity(S.linear_transform(first, 0.37, 0.05), 0.2, 0.9)
    assert fresh[0].tobytes() == want.tobytes() and want.min() == np.float32(0.2) and want.max() == np.float32(0.9)
    assert [i for i, _ in fresh[2]] == [(64 >> l, 48 >> l, 1, 4) for l in range(6)]
    assert cases.bits(fresh[1][2][1]).tobytes() == cases.bits(S.filter_separable(want, long_b, long_a)).tobytes()
    assert fresh[3][1][1].any() and len(fresh[4][1]) == 16 and fresh[4][3].tolist() == [True, True, False]
