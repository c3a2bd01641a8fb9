"""What tests/test_colormap_warp.py and tests/test_colormap_warp_gpu.py share, computed once per process and left unchanged:
the fixture, the scene as the generator saw it, and the specification's runs on it."""
import functools
import hashlib
import os

import numpy as np

import colormap_spec as S
import colormap_warp_scene as scene
import colormap_warp_spec as WS

HERE = os.path.dirname(os.path.abspath(__file__))
ANCHORS = (5, 16)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(HERE, "golden", "colormap_warp.npz"))
    return {k: g[k] for k in g.files}


def spec_option(anchors, **kw):
    o = S.default_option()
    o["maximum_allowable_depth"] = scene.scene.MAX_DEPTH
    o["number_of_vertical_anchors"] = anchors
    o["non_rigid_anchor_point_weight"] = float(golden()["a%d_weight" % anchors])
    o.update(kw)
    return o


@functools.lru_cache(maxsize=None)
def inputs():
    """the scene as the generator saw it (digests checked): depths, colors, extrinsics, intrinsic, vertices"""
    g = golden()
    depths, colors, E, K = scene.frames()
    V = scene.vertices()
    assert np.array_equal(sha(depths), g["depths_sha"]) and np.array_equal(sha(colors), g["colors_sha"])
    assert np.array_equal(sha(V), g["vertices_sha"]) and np.array_equal(E, g["extrinsics0"]) and np.array_equal(K, g["intrinsic"])
    return depths, colors, E, K, V


@functools.lru_cache(maxsize=None)
def spec(anchors):
    """the specification on the fixture case: the initial state (state, proxy0, colors0), per iteration k = 1 .. 8 its cell rows
    and their bounds BEFORE the step and what the step reported (rows[k - 1], bounds[k - 1], hist[k - 1] = rr, rr_reg, count
    per camera, flows_before[k - 1]), the states after 1, 2 and 8 (E1, F1, ...), colors8"""
    depths, colors, E, K, V = inputs()
    st = WS.State(V, depths, colors, E, K, spec_option(anchors))
    run = WS.State(V, depths, colors, E, K, spec_option(anchors))
    o = dict(state=st, proxy0=st.proxy(), colors0=st.colours(), rows=[], bounds=[], hist=[], flows_before=[])
    for k in range(1, 9):
        rows, bounds = run.cell_sums()
        o["rows"].append(rows); o["bounds"].append(bounds); o["flows_before"].append(run.flows.copy())
        o["hist"].append(run.step(rows=rows))
        if k in (1, 2, 8):
            o["E%d" % k], o["F%d" % k] = run.E.copy(), run.flows.copy()
    o["colors8"] = run.colours()
    return o
