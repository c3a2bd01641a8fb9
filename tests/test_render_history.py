"""One context through a mixed history of renders against fresh ones (tests/history.py): images of different sizes (the
key buffer and the set-up scratch grow), a scene of large triangles behind one of small ones (the item lists of the large
path change size), 600 large triangles and a 130 x 100 image between small renders (the item lists grow to 1200 rows and are
then under-filled), both encodings, a Purge and a filter between two renders (other objects' scratch), a mesh from a volume.
A render depends on the mesh, the camera and the pose, never on what the context's grow-only scratch held before.  GPU against
GPU: raw bytes."""
import numpy as np
import pytest

import render_cases as cases
import tsdf_scene
from history import replay


def render(ctx, c, purge=False):
    with ctx.trimesh(c["V"], c["F"]) as mesh:
        if purge:
            mesh.purge()
        d, i, m = mesh.render(c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"], c["encoding"])
        metric = d if c["encoding"] == 0 else mesh.render(c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"])[0]
        e = ctx.render_edges(metric)
        out = tuple(x.get() for x in (d, i, m, e))
        for x in (d, i, m, e, metric):                      # (close() of a closed image does nothing)
            x.close()
    return out


@pytest.mark.gpu
def test_render_history(lib):
    frames, k = tsdf_scene.frames(64, 48, 1)
    depth, rgb, gray, E = frames[0]

    def small(ctx): return render(ctx, cases.CASES["sphere_17x13"])
    def crowd(ctx): return render(ctx, cases.CASES["crowd_depth_buffer"])
    def close_up(ctx): return render(ctx, cases.CASES["sphere_close_64x48"])
    def tiny(ctx): return render(ctx, cases.CASES["sphere_1x1"]) + render(ctx, cases.CASES["empty_mesh"])
    def many_large(ctx): return render(ctx, cases.CASES["many_large"])
    def four_items(ctx): return render(ctx, cases.CASES["chunk_130x100"])

    def purge_and_filter_between(ctx):
        a = render(ctx, cases.CASES["tie_two_copies"], purge=True)
        with ctx.image(depth) as img, img.filter("gaussian5") as f:
            blurred = f.get()
        return a, blurred, render(ctx, cases.CASES["inside_box"])

    def from_a_volume(ctx):
        vol = ctx.tsdf_uniform(2.0, 32, 0.1, lib.TSDF_COLOR_NONE, origin=(-1.0, -1.0, -1.0))
        vol.integrate(depth, None, k, E)
        vol.extract_triangle_mesh()
        with vol.triangle_mesh() as mesh:
            imgs = mesh.render(64, 48, k, E)
            out = tuple(x.get() for x in imgs)
        vol.close()
        return out

    fresh = replay(lambda: lib.Context(0), [
        ("a 17 x 13 render", None, small),
        ("one large triangle over 2048 small ones, depth-buffer encoding", None, crowd),
        ("a close sphere: every triangle on the large path", None, close_up),
        ("1 x 1 and an empty mesh", None, tiny),
        ("600 large triangles in three tiles: the item lists grow to 1200 rows", None, many_large),
        ("a Purge and a filter between two renders", None, purge_and_filter_between),
        ("130 x 100, 84 items: the key buffer grows, the item lists are under-filled", None, four_items),
        ("a mesh from a volume", None, from_a_volume),
        ("the 17 x 13 render again", None, small)])
    # the history is not vacuous, and its steps are the host's
    for got, name in ((fresh[0], "sphere_17x13"), (fresh[1], "crowd_depth_buffer"), (fresh[2], "sphere_close_64x48"),
                      (fresh[4], "many_large"), (fresh[6], "chunk_130x100")):
        for g, w in zip(got, cases.host(lib, cases.CASES[name])):
            assert cases.bits(g).tobytes() == cases.bits(w).tobytes()
    assert (fresh[7][2] == 255).sum() > 300 and (fresh[5][0][2] == 255).sum() == 81
