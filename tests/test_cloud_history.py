"""One resident Cloud through a mixed history of calls against fresh clouds (tests/history.py): crop, then transform, then
estimate_normals, then append, then select.  A call's result depends on the cloud's rows and the call's arguments, never on
what the object -- its grow-only scratch buffers, its compaction tables, the buffers it swapped -- held before.  GPU against
GPU: raw bytes."""
import numpy as np
import pytest

import cloud_cases as cases
import cloud_spec as S
from history import replay


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


class Slot:
    """the one cloud of a history: the operations that make a new cloud put it in the old one's place"""

    def __init__(self, ctx, c):
        self.ctx = ctx
        self.cloud = ctx.cloud(c["points"], c["normals"], c["colors"])

    def put(self, c):
        self.cloud.close()
        self.cloud = self.ctx.cloud(c["points"], c["normals"], c["colors"])

    def replace(self, fresh):
        self.cloud.close()
        self.cloud = fresh

    def close(self):
        self.cloud.close()


def first_cloud():
    """3,000 points of a bumpy sheet (more than one compaction tile, fewer than a chunk) with colours, a NaN point among them"""
    rng = np.random.default_rng(71)
    n = 3001
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    p = np.stack([xy[:, 0], xy[:, 1], 0.15 * np.sin(4.0 * xy[:, 0]) + 0.1 * np.cos(3.0 * xy[:, 1])], axis=1)
    p[1234] = (0.1, np.nan, 0.0)
    return S.cloud(p, None, rng.uniform(size=(n, 3)))


def state(cloud):
    return cloud.get(), cloud.size(), cloud.bounds(), cloud.mean_and_covariance()


@pytest.mark.gpu
def test_cloud_history(lib, ctx):
    first = first_cloud()
    T = cases._pose(72)
    other = S.cloud(np.random.default_rng(73).normal(size=(300, 3)), np.random.default_rng(74).normal(size=(300, 3)),
                    np.random.default_rng(75).uniform(size=(300, 3)))
    lo, hi = (-0.8, -0.6, -1.0), (0.7, 0.9, 1.0)
    # the logical states along the history: the specification where it has the operation, the library's own read-back after
    # estimate_normals (which the specification does not restate: it is pinned to the host-array entry point elsewhere)
    states = {}

    def crop(slot):
        slot.replace(slot.cloud.crop(lo, hi))
        states["cropped"] = slot.cloud.get()
        return state(slot.cloud)

    def transform(slot):
        slot.cloud.transform(T)
        states["moved"] = slot.cloud.get()
        return state(slot.cloud)

    def normals(slot):
        slot.cloud.estimate_normals(knn=10, radius=0.2)
        states["with_normals"] = slot.cloud.get()
        return state(slot.cloud)

    def append(slot):
        with ctx.cloud(other["points"], other["normals"], other["colors"]) as more:
            slot.cloud.append(more)
        slot.cloud.append(slot.cloud)
        states["appended"] = slot.cloud.get()
        return state(slot.cloud)

    def select(slot):
        n = len(slot.cloud)
        idx = (np.arange(2 * n, dtype=np.int64) * 7) % n
        slot.replace(slot.cloud.select(idx))
        down = slot.cloud.voxel_down_sample(0.1)
        try:
            return state(slot.cloud), state(down), slot.cloud.mahalanobis_distance()
        finally:
            down.close()

    fresh = replay(lambda: Slot(ctx, first), [
        ("crop", None, crop),
        ("transform", lambda slot: slot.put(states["cropped"]), transform),
        ("estimate_normals", lambda slot: slot.put(states["moved"]), normals),
        ("append, another cloud and itself", lambda slot: slot.put(states["with_normals"]), append),
        ("select, then voxel_down_sample of the result", lambda slot: slot.put(states["appended"]), select)])
    # the history is not vacuous: rows were dropped, moved, given normals, multiplied
    n0 = len(first["points"])
    counts = [len(fresh[0][0]["points"]), len(fresh[3][0]["points"]), len(fresh[4][0][0]["points"])]
    print("cloud history: %d points, cropped %d, appended %d, selected %d, down-sampled %d" % (n0, counts[0], counts[1], counts[2], len(fresh[4][1][0]["points"])))
    assert 256 < counts[0] < n0 and counts[1] == 2 * (counts[0] + 300) and counts[2] == 2 * counts[1]
    want = S.crop(first, lo, hi)
    assert fresh[0][0]["points"].tobytes() == want["points"].tobytes() and fresh[0][0]["colors"].tobytes() == want["colors"].tobytes()
    assert fresh[1][0]["points"].tobytes() != fresh[0][0]["points"].tobytes()
    assert fresh[1][0]["normals"] is None and fresh[2][0]["normals"] is not None and fresh[3][0]["normals"] is not None
    assert 0 < len(fresh[4][1][0]["points"]) < counts[2]
