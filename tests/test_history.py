"""Every object that lives across calls, driven through a history of calls of different sizes (tests/history.py): each call's
result on the object with the history is, byte for byte, the result on an object made fresh and brought to the same logical
state by the shortest route.  What the other test files leave out: they make an object, run one shape on it and close it, and
a buffer fresh from the allocator is very often all zeros and exactly the call's size -- a kernel that relies on zeroed
scratch, a count taken from a capacity, or rows of an earlier, larger call read as the current one's show only on an object
that has done something else before.

A fresh object could share a bug with the reused one, so the fresh results are also held against the numpy specification of
the feature's own test file, with that file's comparison and bound (imported, not restated).  Of the context's one-shot
calls only the odometry has such a specification here; the others are compared GPU against GPU alone, and a bug that a
fresh and a reused context share stays the business of the feature's own test file.

CPU: the conditions that keep a history from being vacuous -- the large step at least four times the small one, the small
one not empty, the heap path taken, the pool growing, Purge shrinking the mesh -- are asserted on the specification's results
alone (test_*_is_not_vacuous), and again by each GPU test before it looks at a GPU result."""
import ctypes as C
import functools

import numpy as np
import pytest

import colormap_scene as cm_scene
import colormap_spec as CS
import kdtree_spec as KS
import odometry_scene as odo_scene
import odometry_spec as OS
import test_colormap as CT
import test_kdtree as KT
import test_trimesh as MT
import test_tsdf_mesh as VM
import trimesh_cases as mesh_cases
import trimesh_spec as T
import tsdf_mesh_cases as tsdf_cases
import tsdf_scene
import tsdf_spec as VS
from history import difference, replay
from kdtree_spec import HYBRID, KNN, LDS_MAX, RADIUS


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def same_bytes(a, b):
    return difference(a, b) is None


# ---------------------------------------------------------------------------
# KDTree
# ---------------------------------------------------------------------------
KD_K = 200              # > LDS_MAX: the lists live in a global heap
KD_TREES = (2000, 65)


def kd_steps(n):
    """-> the tree and [(name, queries, (type, cap, radius))]"""
    tree = KS.cloud(n)
    q513, q257, q65, q1 = (KS.queries_around(tree, nq, 20 + nq) for nq in (513, 257, 65, 1))
    miss = KS.queries_around(tree, 300, 24)[1::3]           # inside the box and no points of the tree: nothing within 1e-7
    none = np.zeros((0, 3))
    return tree, [("knn %d x 513 (heap)" % KD_K, q513, (KNN, KD_K, 0.0)),
                  ("knn 1 x 1", q1, (KNN, 1, 0.0)),
                  ("hybrid cap 5 x 257", q257, (HYBRID, 5, 0.1)),
                  ("radius, total 0", miss, (RADIUS, 0, 1e-7)),
                  ("radius, large total", q513, (RADIUS, 0, 0.3)),
                  ("radius, small total", q65, (RADIUS, 0, 0.03)),
                  ("knn %d x 513 again" % KD_K, q513, (KNN, KD_K, 0.0)),
                  ("knn, nq = 0", none, (KNN, 4, 0.0)),
                  ("radius, nq = 0", none, (RADIUS, 0, 0.3)),
                  ("knn 12 x 257", q257, (KNN, 12, 0.0))]


def kd_rows(s, result):
    """the entries a search lists"""
    return int(result[0][-1]) if s[0] == RADIUS else int(result[2].sum())


@functools.lru_cache(maxsize=None)
def kd_spec(n):
    """the specification's result of every step, computed once; the history's conditions asserted on it"""
    tree, steps = kd_steps(n)
    want = [KT.spec_of(tree, q, s) for _, q, s in steps]
    rows = [kd_rows(s, w) for (_, _, s), w in zip(steps, want)]
    if n > LDS_MAX:
        assert min(KD_K, n) > LDS_MAX                               # the heap path is taken
    else:
        assert KD_K > n and (want[0][2] == n).all()                 # k > n: every list is shorter than its row, the rest is padding
    assert rows[0] >= 4 * rows[1] and rows[1] > 0, rows             # knn: large, then small
    assert rows[2] > 0 and rows[3] == 0, rows                       # a positive total, then the zero case
    assert rows[4] >= 4 * rows[5] and rows[5] > 0, rows             # radius: large, then small
    assert rows[6] >= rows[0] and rows[7] == 0 and rows[8] == 0 and rows[9] > 0, rows
    return tree, steps, want, rows


class Recorded:
    """what test_kdtree.check calls a tree for, answering with a recorded result"""

    def __init__(self, result):
        self.result = result

    def search_knn(self, *args):
        return self.result

    search_hybrid = search_radius = search_knn


@pytest.mark.parametrize("n", KD_TREES)
def test_kdtree_history_is_not_vacuous(n):
    rows = kd_spec(n)[3]
    print("kdtree %d: rows per step %s" % (n, rows))


@pytest.mark.gpu
@pytest.mark.parametrize("n", KD_TREES)
def test_kdtree_history(ctx, n):
    tree, steps, want, rows = kd_spec(n)
    L = ctx.L

    def call_of(q, s):
        def call(kd):
            got = KT.run(kd, q, s)
            if s[0] == RADIUS and got[0][-1] == 0:                  # the zero case: its result downloads into nothing
                return got + (L.visma_icp_kdtree_get_radius_result(kd._t, None, None),)
            return got
        return call

    fresh = replay(lambda: ctx.kdtree(tree), [(name, None, call_of(q, s)) for name, q, s in steps])
    for (name, q, s), f, w in zip(steps, fresh, want):
        if s[0] == RADIUS and w[0][-1] == 0:
            assert f[3] == 0, name
        KT.check(Recorded(f[:3]), tree, q, s, want=w)               # idx, d2 bits, cnt / offsets, the -1 / +inf padding


# ---------------------------------------------------------------------------
# TSDF
# ---------------------------------------------------------------------------
TSDF_VARIANTS = [(False, VS.COLOR_NONE), (False, VS.COLOR_RGB8), (True, VS.COLOR_NONE), (True, VS.COLOR_RGB8)]
TSDF_IDS = ["uniform-none", "uniform-rgb8", "scalable-none", "scalable-rgb8"]


def tsdf_script(scalable):
    """-> the case (tests/tsdf_mesh_cases.py: u32 / s0, the scene's four 40 x 30 frames) and the history: ("integrate",
    [frame, ...]) | ("extract",) | ("reset",), a frame = (depth, rgb, intrinsic, extrinsic)"""
    case = tsdf_cases.load("s0" if scalable else "u32")
    k = np.asarray(case["intrinsic"], np.float64)
    h, w = case["frames"][0][0].shape
    large = [(fr[0], fr[1], k, fr[3]) for fr in case["frames"]]
    # the same frames, every second pixel in both directions: pixel (u, v) of the small image is pixel (2u, 2v) of the large
    small = [(np.ascontiguousarray(fr[0][::2, ::2]), np.ascontiguousarray(fr[1][::2, ::2]), k / 2.0, fr[3]) for fr in case["frames"]]
    k_off = k + [0.0, 0.0, 1.5, -2.25]                               # the large size, another principal point
    depth, rgb, _ = tsdf_scene.render(w, h, 2, k_off)
    moved = (depth, rgb, k_off, tsdf_scene.extrinsic(2))
    assert small[0][0].shape == (h // 2, w // 2) and moved[0].shape == large[0][0].shape
    script = [("integrate", [large[0]]), ("extract",), ("integrate", [small[1]]), ("extract",), ("integrate", [moved]), ("extract",),
              ("reset",), ("extract",), ("integrate", [small[3]]), ("extract",), ("integrate", large + [small[1], moved]), ("extract",)]
    return case, script


def tsdf_states(script):
    """-> for every step the frames integrated since the last reset, before the step and after it"""
    before, after, since = [], [], []
    for op, *arg in script:
        before.append(list(since))
        if op == "reset":
            since = []
        elif op == "integrate":
            since = since + list(arg[0])
        after.append(list(since))
    return before, after


def spec_integrated(case, color_type, frames):
    if case["scalable"]:
        vol = VS.new_scalable(case["voxel_length"], case["sdf_trunc"], color_type, case["R"], case["stride"])
    else:
        vol = VS.new_volume(case["length"], case["R"], case["sdf_trunc"], color_type, case["origin"])
    for depth, rgb, k, E in frames:
        (VS.scalable_integrate if case["scalable"] else VS.integrate)(vol, depth, rgb if color_type == VS.COLOR_RGB8 else None, k, E)
    return vol


def pool_growths(initial, unit_counts):
    """A MODEL of tsdf.hip's pool, not a measurement (the C ABI does not report the capacity): tsdf_device_integrate calls
    pool_resize(D, std::max(need, 2 * D->capacity)) when a frame needs more units than the pool holds, and the pool starts at
    max(initial_units, 1).  If that policy changes, this function has to follow it, or the history may stop reallocating
    mid-way without any test noticing.  -> the steps (indices into unit_counts) at which the pool grows"""
    cap, out = max(initial, 1), []
    for i, need in enumerate(unit_counts):
        if need is not None and need > cap:
            cap = max(need, 2 * cap)
            out.append(i)
    return out


@functools.lru_cache(maxsize=None)
def tsdf_spec_history(scalable, color_type):
    """the specification's volume, point cloud and voxel cloud at every extraction of the history, computed once; the
    history's conditions asserted on it.  -> case, script, {step: (volume, pc, vx)}, rows, initial_units"""
    case, script = tsdf_script(scalable)
    _, after = tsdf_states(script)
    spec, rows, units = {}, {}, []
    for i, (op, *arg) in enumerate(script):
        vol = spec_integrated(case, color_type, after[i]) if op != "reset" else None
        units.append(len(vol["units"]) if scalable and op == "integrate" else None)
        if op == "extract":
            pc = (VS.scalable_extract_point_cloud if scalable else VS.extract_point_cloud)(vol)
            vx = (VS.scalable_extract_voxel_point_cloud if scalable else VS.extract_voxel_point_cloud)(vol)
            spec[i] = (vol, pc, vx)
            rows[i] = len(pc[0])
    first, large, zero, small, last = rows[1], rows[5], rows[7], rows[9], rows[11]
    assert zero == 0 and small > 0 and large >= 4 * small and last >= max(first, large), rows
    assert rows[3] > 0
    initial = 0
    if scalable:
        initial = max(2, units[0] // 4)                              # below the first frame's unit count (tests/test_tsdf.py)
        grows = pool_growths(initial, units)
        assert 2 * initial < units[0] and grows[0] == 0 and any(g > 1 for g in grows), (units, grows)   # ... and again after the first extraction
    return case, script, spec, rows, initial


class Vol:
    """a volume and the device-to-device mesh copies taken from it"""

    def __init__(self, vol):
        self.vol, self.kept = vol, []

    def close(self):
        try:
            for m in self.kept:
                m.close()
        finally:
            self.vol.close()


def tsdf_contents(vol):
    """the voxels: (tsdf, weight, color) of a uniform volume; (units, tsdf, weight, color) unit by unit of a scalable one"""
    if not vol.scalable:
        return tuple(vol.volume())
    units = vol.units()
    per = [vol.volume(k) for k in units.tolist()]
    R3, has = vol.resolution ** 3, vol.color_type != VS.COLOR_NONE
    stack = lambda j, tail: np.stack([p[j] for p in per]) if per else np.zeros((0, R3) + tail, np.float32)
    return units, stack(0, ()), stack(1, ()), (stack(2, (3,)) if has else None)


def tsdf_integrate(v, frames):
    for depth, rgb, k, E in frames:
        h, w = depth.shape
        v.vol.integrate(depth, rgb if v.vol.color_type == VS.COLOR_RGB8 else None, k, E, intrinsic_size=(w, h))


def tsdf_extract(v, keep=False):
    """the three extractions and the mesh as a TriMesh of its own (kept open if asked)"""
    vol = v.vol
    out = dict(contents=tsdf_contents(vol), pc=vol.extract_point_cloud(), vx=vol.extract_voxel_point_cloud(), mesh=vol.extract_triangle_mesh())
    copy = vol.triangle_mesh()
    try:
        out["copy"], out["copy_size"] = copy.get(), copy.size()
    finally:
        if keep:
            v.kept.append(copy)
        else:
            copy.close()
    return out


class RecordedVolume:
    """what test_tsdf_mesh.check_against_spec asks a volume, answering with a recorded extraction"""

    def __init__(self, vol, recorded):
        for k in ("resolution", "color_type", "scalable", "voxel_length", "sdf_trunc", "length", "origin"):
            setattr(self, k, getattr(vol, k))
        self.recorded = recorded

    def units(self):
        return self.recorded["contents"][0]

    def volume(self, key=None):
        c = self.recorded["contents"]
        if not self.scalable:
            return c
        i = c[0].tolist().index(list(key))
        return c[1][i], c[2][i], (None if c[3] is None else c[3][i])

    def extract_triangle_mesh(self):
        return self.recorded["mesh"]


def tsdf_check_against_spec(probe, scalable, color_type, got, spec, label):
    """an extraction against the specification, the way tests/test_tsdf.py (test_larger_shape_equals_the_specification,
    test_scalable_volumes_equal_the_reference) and tests/test_tsdf_mesh.py (check_against_spec) do it"""
    from test_tsdf import same_bits
    vol, pc, vx = spec
    c = got["contents"]
    if scalable:
        keys = sorted(vol["units"])
        assert np.array_equal(c[0], np.array(keys, np.int32).reshape(-1, 3)), label
        for i, key in enumerate(keys):
            u = vol["units"][key]
            assert same_bits(c[1][i], u["tsdf"]) and same_bits(c[2][i], u["weight"]), (label, key)
            assert u["color"] is None or same_bits(c[3][i], u["color"]), (label, key)
    else:
        assert same_bits(c[0], vol["tsdf"]) and same_bits(c[1], vol["weight"]), label
        assert (c[2] is None and vol["color"] is None) or same_bits(c[2], vol["color"]), label
    pts, nrm, col = got["pc"]
    assert same_bits(pts, pc[0]), label
    assert (col is None and color_type == VS.COLOR_NONE) or same_bits(col, pc[2]), label
    dn = float(np.max(np.abs(nrm - pc[1]), initial=0.0))
    assert dn <= VS.NORMAL_TOL and same_bits(nrm, pc[1]), (label, dn)
    assert same_bits(got["vx"][0], vx[0]) and same_bits(got["vx"][1], vx[1]), label
    v, col, t = VM.check_against_spec(RecordedVolume(probe, got), label)
    # the device-to-device copy is the extracted mesh: no normals, the volume's colours
    copy = got["copy"]
    assert got["copy_size"][:2] == (len(v), len(t)) and copy["vertices"].tobytes() == v.tobytes() and copy["triangles"].tobytes() == t.tobytes()
    assert copy["vertex_normals"] is None and copy["triangle_normals"] is None
    if col is None or not len(v):
        assert copy["vertex_colors"] is None, label
    else:
        assert copy["vertex_colors"].tobytes() == col.tobytes(), label
    return len(pts), len(v), len(t)


@pytest.mark.parametrize("scalable,color_type", TSDF_VARIANTS, ids=TSDF_IDS)
def test_tsdf_history_is_not_vacuous(scalable, color_type):
    rows = tsdf_spec_history(scalable, color_type)[3]
    print("tsdf %s: point cloud rows per extraction %s" % ("scalable" if scalable else "uniform", rows))


@pytest.mark.gpu
@pytest.mark.parametrize("scalable,color_type", TSDF_VARIANTS, ids=TSDF_IDS)
def test_tsdf_history(ctx, scalable, color_type):
    """The shortest route to a step's state is a fresh volume and the frames since the last reset: the fresh volume is NOT
    reset first, so a reset that left something behind shows against a volume that never held anything."""
    case, script, spec, rows, initial = tsdf_spec_history(scalable, color_type)
    before, _ = tsdf_states(script)

    def make():
        if scalable:
            return Vol(ctx.tsdf_scalable(case["voxel_length"], case["sdf_trunc"], color_type, case["R"], case["stride"], initial_units=initial))
        return Vol(ctx.tsdf_uniform(case["length"], case["R"], case["sdf_trunc"], color_type, case["origin"]))

    def step(i, op, arg):
        to_state = lambda v: tsdf_integrate(v, before[i])
        if op == "integrate":
            def call(v):
                tsdf_integrate(v, arg[0])
                return tsdf_contents(v.vol)
        elif op == "reset":
            def call(v):
                v.vol.reset()
                return tsdf_contents(v.vol)
        else:
            def call(v):
                return tsdf_extract(v, keep=(i == 1))               # the first extraction's copy stays open to the end
        return ("%d: %s" % (i, op), to_state, call)

    steps = [step(i, op, arg) for i, (op, *arg) in enumerate(script)]

    # the copy taken at the first extraction, downloaded again after everything else: what a fresh volume in the first
    # extraction's state gives, and what it gave then
    def first_state(v):
        tsdf_integrate(v, before[1])
        tsdf_extract(v, keep=True)

    def first_copy(v):
        return v.kept[0].get(), v.kept[0].size()
    steps.append(("the first extraction's copy, again", first_state, first_copy))

    fresh = replay(make, steps)
    probe = make()
    try:
        for i in sorted(spec):
            counts = tsdf_check_against_spec(probe.vol, scalable, color_type, fresh[i], spec[i], "step %d" % i)
            assert counts[0] == rows[i]
            print("step %d: %d points, %d vertices, %d triangles" % ((i,) + counts))
            if rows[i] == 0:                                         # the zero case: sizes 0, every array empty
                assert counts == (0, 0, 0) and len(fresh[i]["vx"][0]) == 0 and fresh[i]["copy_size"][:2] == (0, 0)
                assert not scalable or len(fresh[i]["contents"][0]) == 0
    finally:
        probe.close()
    assert same_bytes(fresh[-1], (fresh[1]["copy"], fresh[1]["copy_size"]))


# ---------------------------------------------------------------------------
# TriMesh
# ---------------------------------------------------------------------------
def big16():
    """trimesh_cases.big at one sixteenth: a 100 x 100 grid, every third triangle repeated as a rotation, and a band of 188
    vertices no triangle uses in its middle"""
    gv, gt = mesh_cases._grid(100, step=1.0 / 64.0, seed=2)
    band = np.stack([np.arange(188) * 0.25, np.full(188, -5.0), np.zeros(188)], axis=1)
    at = 5000
    v = np.concatenate([gv[:at], band, gv[at:]])
    gt = np.where(gt >= at, gt + len(band), gt)
    rep = np.roll(gt[::3], 1, axis=1)
    t = np.concatenate([gt[:12500], rep, gt[12500:]])
    return T.mesh(v, t)


def tenth_of_the_box(m):
    """an axis-aligned box around the middle of the mesh with a tenth of its bounding box's volume"""
    lo, hi = m["vertices"].min(0), m["vertices"].max(0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * 0.1 ** (1.0 / 3.0)
    return tuple(mid - half), tuple(mid + half)


BAND = 400              # vertices of a selected band: several rows of the cropped grid, so triangles lie inside one
HEAD = [("cvn", 1), ("ctn", 1), ("purge",), ("cvn", 1), ("rdv",), ("rdt",), ("transform", mesh_cases._pose(6))]


@functools.lru_cache(maxsize=None)
def mesh_program(which):
    """-> the first mesh, the program, the specification's state before and after every operation and its removed counts,
    the triangle counts of the large and the small mesh.  ("crop10",): crop to a tenth of the box at that point; ("half",):
    select every second band of BAND vertices (every second single vertex would keep no triangle of a grid); ("adopt", mesh, indices): go on with a mesh selected from another one."""
    if which == "shrinking":
        first = big16()
        program = HEAD + [("crop10",), ("cvn", 1), ("purge",), ("half",), ("rnmv",), ("norm",)]
    else:
        first = mesh_cases.load()["tile257"][0]
        large = big16()
        program = HEAD + [("adopt", large, np.arange(len(large["vertices"]))[np.arange(len(large["vertices"])) % 9 != 4])] + HEAD
    state, states, concrete = T.copy(first), [], []
    for op in program:
        if op[0] == "crop10":
            op = ("crop",) + tenth_of_the_box(state)
        elif op[0] == "half":
            op = ("select", np.nonzero((np.arange(len(state["vertices"])) // BAND) % 2 == 0)[0])
        before = state
        if op[0] == "adopt":
            state, removed = T.select(op[1], op[2]), []
        else:
            state, removed = T.run(state, [op])
        for m in (before, state):                                    # no NaN: a state uploaded is the state on the device, to the bit
            assert all(m[k] is None or m[k].dtype != np.float64 or not np.isnan(m[k]).any() for k in T.ATTRS)
        concrete.append(op)
        states.append((before, state, list(removed)))
    nt = [len(after["triangles"]) for _, after, _ in states]
    if which == "shrinking":
        assert program[2] == ("purge",) and 4 * (len(first["triangles"]) - nt[2]) >= len(first["triangles"])   # Purge removes a quarter
        large, small = nt[6], nt[7]
        assert large >= 4 * small and small > 0, (large, small)
        assert program[10] == ("half",) and 0 < nt[10] < small and nt[11] > 0 and nt[12] > 0, nt      # no step on an empty mesh
        assert len(states[10][1]["vertices"]) < len(states[10][0]["vertices"])
    else:
        small, large = nt[6], nt[7]
        assert large >= 4 * small and small > 0 and nt[-1] >= 4 * small, (large, small)
    return first, concrete, states, (large, small)


class Slot:
    """the mesh a program is at: select, crop and adopt put a new one in its place"""

    def __init__(self, ctx, m):
        self.ctx, self.mesh = ctx, MT.upload(ctx, m)

    def put(self, mesh):
        old, self.mesh = self.mesh, mesh
        if old is not None:
            old.close()

    def close(self):
        self.put(None)


def mesh_apply(slot, op):
    """one operation of a program on the slot's mesh -> the removed counts, what get() and size() return afterwards"""
    mesh, removed = slot.mesh, []
    name, arg = op[0], op[1:]
    if name == "ctn":
        mesh.compute_triangle_normals(bool(arg[0]))
    elif name == "cvn":
        mesh.compute_vertex_normals(bool(arg[0]))
    elif name == "norm":
        mesh.normalize_normals()
    elif name == "rdv":
        removed.append(mesh.remove_duplicated_vertices())
    elif name == "rdt":
        removed.append(mesh.remove_duplicated_triangles())
    elif name == "rnmv":
        removed.append(mesh.remove_non_manifold_vertices())
    elif name == "purge":
        removed.extend(mesh.purge())
    elif name == "transform":
        mesh.transform(arg[0])
    elif name == "select":
        slot.put(mesh.select(arg[0]))
    elif name == "crop":
        slot.put(mesh.crop(arg[0], arg[1]))
    elif name == "adopt":
        parent = MT.upload(slot.ctx, arg[0])
        try:
            slot.put(parent.select(arg[1]))
        finally:
            parent.close()
    else:
        raise ValueError(name)
    return tuple(removed), slot.mesh.get(), slot.mesh.size()


MESH_PROGRAMS = ("shrinking", "growing")


@pytest.mark.parametrize("which", MESH_PROGRAMS)
def test_trimesh_history_is_not_vacuous(which):
    first, program, states, (large, small) = mesh_program(which)
    print("trimesh %s: %d triangles at first, large %d, small %d, at the end %d" % (which, len(first["triangles"]), large, small,
                                                                                  len(states[-1][1]["triangles"])))


@pytest.mark.gpu
@pytest.mark.parametrize("which", MESH_PROGRAMS)
def test_trimesh_history(ctx, which):
    """one mesh through a long program; after every operation get() and the removed counts are the specification's at that
    point, and what a mesh uploaded in the state before the operation gives"""
    first, program, states, _ = mesh_program(which)

    def step(i, op):
        return ("%d: %s" % (i, op[0]), lambda slot: slot.put(MT.upload(ctx, states[i][0])), lambda slot: mesh_apply(slot, op))

    fresh = replay(lambda: Slot(ctx, first), [step(i, op) for i, op in enumerate(program)])
    for i, ((removed, got, size), (_, want, want_removed)) in enumerate(zip(fresh, states)):
        label = (which, i, program[i][0])
        assert list(removed) == want_removed, label
        assert size[:2] == (len(want["vertices"]), len(want["triangles"])), label
        MT.same(got, want, label)


# ---------------------------------------------------------------------------
# ColorMap, rigid and non-rigid
# ---------------------------------------------------------------------------
CM_ANCHORS = 5
PAIR_BLOCK = 256        # kPairThreads: prepare gives every camera ceil(longest visible list / 256) workgroups


def cm_option(non_rigid):
    import colormap_warp_cases as warp_cases
    if non_rigid:
        return warp_cases.spec_option(CM_ANCHORS)
    return CT.spec_option()


def cm_inputs():
    """the scene of tests/colormap_scene.py (83 x 61, six cameras, 3,201 vertices; the non-rigid fixture's too) and the
    history: per step the frame behind every image, the vertices, and whether poses (and fields) go back to the first ones"""
    depths, colors, E, K = cm_scene.frames()
    V = cm_scene.vertices()
    steps = [dict(name="all vertices", frames=[0, 1, 2, 3, 4, 5], V=V, start_over=True),
             dict(name="a quarter of the vertices", frames=[0, 1, 2, 3, 4, 5], V=np.ascontiguousarray(V[::4]), start_over=False),
             dict(name="all vertices, image 0 replaced", frames=[3, 1, 2, 3, 4, 5], V=V, start_over=False),
             dict(name="the first images and poses again", frames=[0, 1, 2, 3, 4, 5], V=V, start_over=True)]
    return depths, colors, E, K, steps


def cm_spec_state(non_rigid, step, depths, colors, poses, K, flows=None):
    """the specification's prepared state of a step at the given poses (and fields)"""
    import colormap_warp_spec as WS
    f = step["frames"]
    cls = WS.State if non_rigid else CS.State
    st = cls(step["V"], depths[f], colors[f], poses, K, cm_option(non_rigid))
    if non_rigid and flows is not None:
        st.flows = np.array(flows, np.float64).reshape(st.flows.shape).copy()
    return st


def cm_poses_at_prepare(step, E, carried):
    """the poses a step's prepare sees: the first ones, or the carried ones with the replaced image's own"""
    poses = np.array(E[step["frames"]] if step["start_over"] else carried, np.float64).copy()
    for i, f in enumerate(step["frames"]):
        if f != i:
            poses[i] = E[f]
    return poses


@functools.lru_cache(maxsize=None)
def cm_spec_history(non_rigid):
    """the specification alone through the history: the visible counts of every step, with the history's conditions"""
    depths, colors, E, K, steps = cm_inputs()
    carried, flows, counts = None, None, []
    for step in steps:
        poses = cm_poses_at_prepare(step, E, carried)
        st = cm_spec_state(non_rigid, step, depths, colors, poses, K, None if step["start_over"] else flows)
        counts.append([len(x) for x in st.lists])
        st.run(2)
        carried, flows = st.E.copy(), (st.flows.copy() if non_rigid else None)
    total = [sum(c) for c in counts]
    blocks = [-(-max(c) // PAIR_BLOCK) for c in counts]
    assert total[0] >= 4 * total[1] and total[1] > 0 and total[2] >= total[0] and counts[3] == counts[0], counts
    assert blocks[1] < blocks[0] and blocks[2] == blocks[0], (counts, blocks)          # the quarter crosses multiples of the pair pass's block
    return counts, blocks


@pytest.mark.parametrize("non_rigid", [False, True], ids=["rigid", "non-rigid"])
def test_colormap_history_is_not_vacuous(non_rigid):
    counts, blocks = cm_spec_history(non_rigid)
    print("colormap: visible counts per step %s, workgroups per camera %s" % (counts, blocks))


@pytest.mark.gpu
@pytest.mark.parametrize("non_rigid", [False, True], ids=["rigid", "non-rigid"])
def test_colormap_history(lib, ctx, non_rigid):
    import test_colormap_warp_gpu as WT
    spec_counts, spec_blocks = cm_spec_history(non_rigid)
    depths, colors, E, K, steps = cm_inputs()
    n, h, w = depths.shape
    option = lib.color_map_option(**{k: v for k, v in cm_option(non_rigid).items() if k != "non_rigid_camera_coordinate"})
    carry = {}

    def make():
        return (ctx.color_map_non_rigid if non_rigid else ctx.color_map)(w, h, n, K, option)

    def flow0(m):
        aw, ah, step = m.anchor_shape()
        i, j = np.meshgrid(np.arange(aw), np.arange(ah))               # anchor (i, j) points at (i step, j step)
        return np.tile(np.stack([i * step, j * step], -1).reshape(-1), (n, 1))

    def record(m, k):
        counts = m.prepare()
        out = dict(counts=counts, visible=[m.visible(c) for c in range(n)], proxy=m.proxy(),
                   sums=m.cell_sums() if non_rigid else m.sums(), residual=m.run(2), extrinsics=m.extrinsics(), colors=m.colors())
        if non_rigid:
            out["flow"], out["cell_sums_after"] = m.flow(), m.cell_sums()
        carry[k] = (out["extrinsics"], out.get("flow"))            # (the poses and fields the next step starts from)
        return out

    def step_of(k):
        step, prev = steps[k], steps[k - 1] if k else None

        def to_state(m):                                               # the images, poses, vertices and fields before the step
            for i, f in enumerate(prev["frames"]):
                m.set_image(i, depths[f], colors[f], carry[k - 1][0][i])
            m.set_vertices(prev["V"])
            if non_rigid:
                m.set_flow(carry[k - 1][1])

        def call(m):
            for i, f in enumerate(step["frames"]):
                if prev is None or prev["frames"][i] != f:
                    m.set_image(i, depths[f], colors[f], E[f])
            if prev is None or prev["V"] is not step["V"]:
                m.set_vertices(step["V"])
            if step["start_over"] and prev is not None:
                m.set_extrinsics(E)
                if non_rigid:
                    m.set_flow(flow0(m))
            return record(m, k)
        return (step["name"], to_state if k else None, call)

    fresh = replay(make, [step_of(k) for k in range(len(steps))])
    assert same_bytes(fresh[3], fresh[0])                               # the first state again: the first result again
    # the large step, the small one after it and the large one again, against the specification at the library's own poses
    for k in (0, 1, 2):
        step, got = steps[k], fresh[k]
        poses = cm_poses_at_prepare(step, E, fresh[k - 1]["extrinsics"] if k else None)
        flows = None if (not non_rigid or step["start_over"]) else fresh[k - 1]["flow"]
        st = cm_spec_state(non_rigid, step, depths, colors, poses, K, flows)
        assert np.array_equal(got["counts"], [len(x) for x in st.lists]), k
        assert all(np.array_equal(got["visible"][c], st.lists[c]) for c in range(n)), k
        assert -(-int(got["counts"].max()) // PAIR_BLOCK) == spec_blocks[k]
        p = st.proxy()
        assert np.array_equal(CT.bits(got["proxy"]), CT.bits(p)), k
        if non_rigid:
            rows, bounds = st.cell_sums()
            WT.check_cell_sums(got["sums"], rows, bounds)
            st.flows = got["flow"].copy()
        else:
            CT.check_sums(got["sums"], st, p)
        st.E = got["extrinsics"].copy()
        assert np.abs(got["colors"] - st.colours()).max() <= 1e-15, k
        print("%s: visible %s" % (step["name"], got["counts"].tolist()))


# ---------------------------------------------------------------------------
# the context's one-shot calls: they share the engine's neighbour search and scratch
# ---------------------------------------------------------------------------
ODO_ITERATIONS = (2, 2, 2)


def box_cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3)) * [1.0, 0.8, 0.5]


def unit_rows(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def odometry_frames():
    """the frame pair of tests/odometry_scene.py at 100 x 75 (the fixture's size) and every second pixel of it, 50 x 38"""
    large = odo_scene.frames(100, 75)
    small = tuple(np.ascontiguousarray(a[::2, ::2]) for a in large[:4]) + (large[4] / 2.0,)
    return large, small


@functools.lru_cache(maxsize=None)
def odometry_spec_runs():
    """the specification's runs of both pairs; the large pair has at least four times the small one's pairs"""
    opt = dict(OS.default_option(), iterations=list(ODO_ITERATIONS))
    runs = [OS.rgbd_odometry(*fr, np.eye(4), OS.HYBRID, opt) for fr in odometry_frames()]
    assert runs[0][0] and runs[1][0] and runs[0][3]["info_K"] >= 4 * runs[1][3]["info_K"] > 0
    return opt, runs


def context_calls(lib):
    """-> [(name, rows, call)]: call(ctx) -> a tuple of arrays; rows: the rows the call works on (None: not a size step)"""
    large, small = odometry_frames()
    option = lib.odometry_option(ODO_ITERATIONS)
    p3000, p1000, p200, p1500 = box_cloud(3000, 1), box_cloud(1000, 2), box_cloud(200, 3), box_cloud(1500, 4)
    n1000, n1500, c1500 = unit_rows(1000, 5), unit_rows(1500, 6), np.random.default_rng(7).random((1500, 3))
    fa33, fb33, fa5, fb5 = (np.random.default_rng(8 + i).random(s) for i, s in enumerate(((257, 33), (513, 33), (20, 5), (10, 5))))
    v20000, vn, vc = box_cloud(20000, 12), unit_rows(20000, 13), np.random.default_rng(14).random((20000, 3))
    v50 = box_cloud(50, 15)
    nan_rows = np.full((30, 3), np.nan)
    src, tgt, few_s, few_t = box_cloud(3000, 16), box_cloud(5000, 17), box_cloud(20, 18), box_cloud(30, 19)
    gv, gt = mesh_cases._grid(20, step=0.05, seed=6)
    two_v, two_t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], np.float64), np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    q2000, q10 = box_cloud(2000, 20), box_cloud(10, 21)
    from visma_amd import synth
    pair = synth.make_pair(300, 1000, seed_t=11, seed_s=12)

    def odometry(fr):
        def call(c):
            r = c.rgbd_odometry(*fr, np.eye(4), lib.ODOMETRY_HYBRID, option)
            return int(r.success), r.T, r.information, int(r.information_pairs), r.pairs
        return call

    def mesh_distance(method, P, V, F):
        def call(c):
            c.set_mesh_search(method)
            try:
                return tuple(a.copy() for a in c.point_mesh_distance(P, V, F))
            finally:
                c.set_mesh_search("auto")
        return call

    def information(c):
        c.set_clouds_f64(pair[0], pair[1])
        M, k = c.information_matrix(None, pair[3])
        return M, int(k)

    calls = [("normals, 3,000 points, knn 30", 3000, lambda c: (c.estimate_normals(p3000, knn=30),)),
             ("fpfh, 1,000 points, radius", 1000, lambda c: (c.compute_fpfh(p1000, n1000, knn=100, radius=0.2),)),
             ("normals, 200 points, knn 5", 200, lambda c: (c.estimate_normals(p200, knn=5),)),
             ("colour gradient, 1,500 points", 1500, lambda c: (c.color_gradient(p1500, n1500, c1500, 0.15, max_nn=30),)),
             ("normals by radius", 3000, lambda c: (c.estimate_normals(p3000, knn=None, radius=0.1),)),
             ("match, dim 33, 257 x 513", 513, lambda c: c.match_features(fa33, fb33)),
             ("match, dim 5, 20 x 10", 10, lambda c: c.match_features(fa5, fb5)),
             ("voxels of 20,000 points", 20000, lambda c: c.voxel_down_sample(v20000, 0.05, vn, vc)),
             ("voxels of 50 points", 50, lambda c: c.voxel_down_sample(v50, 0.05, vn[:50], vc[:50])),
             ("voxels of rows that are all NaN", 30, lambda c: c.voxel_down_sample(nan_rows, 0.05, vn[:30], vc[:30])),
             ("voxels of 20,000 points again", 20000, lambda c: c.voxel_down_sample(v20000, 0.05, vn, vc)),
             ("cloud distance, 3,000 -> 5,000", 3000, lambda c: (c.point_cloud_distance(src, tgt).copy(),)),
             ("cloud distance, 20 -> 30", 20, lambda c: (c.point_cloud_distance(few_s, few_t).copy(),)),
             ("neighbour distance, 3,000", 3000, lambda c: (c.nearest_neighbor_distance(src).copy(),)),
             ("neighbour distance, 20", 20, lambda c: (c.nearest_neighbor_distance(few_s).copy(),))]
    for method in ("brute", "bvh"):
        calls += [("mesh distance (%s), 800 triangles" % method, len(gt), mesh_distance(method, q2000, gv, gt)),
                  ("mesh distance (%s), two triangles" % method, len(two_t), mesh_distance(method, q10, two_v, two_t))]
    calls += [("information matrix", None, information),
              # (their rows are the pairs the specification finds: odometry_spec_runs)
              ("odometry, 100 x 75", None, odometry(large)), ("odometry, 50 x 38", None, odometry(small)),
              ("odometry, 100 x 75 again", None, odometry(large))]
    return calls


def test_context_history_is_not_vacuous(lib):
    """every family of calls has a large step at least four times the small one after it; the neighbour lists of the FPFH
    step are longer than 30"""
    calls = context_calls(lib)
    rows = {name: r for name, r, _ in calls}
    for large, small in (("normals, 3,000 points, knn 30", "normals, 200 points, knn 5"), ("match, dim 33, 257 x 513", "match, dim 5, 20 x 10"),
                         ("voxels of 20,000 points", "voxels of 50 points"), ("cloud distance, 3,000 -> 5,000", "cloud distance, 20 -> 30"),
                         ("neighbour distance, 3,000", "neighbour distance, 20"), ("mesh distance (brute), 800 triangles", "mesh distance (brute), two triangles"),
                         ("mesh distance (bvh), 800 triangles", "mesh distance (bvh), two triangles")):
        assert rows[large] >= 4 * rows[small] > 0, (large, small)
    assert rows["voxels of 20,000 points again"] >= rows["voxels of 20,000 points"]
    p = box_cloud(1000, 2)
    within = (KS.spec_pairs(p, p, KS.HYBRID, 0.2)[1].sum(1))
    assert np.median(within) > 30 and within.max() > 100, (np.median(within), within.max())     # lists longer than 30, some cut at 100
    odometry_spec_runs()


@pytest.mark.gpu
def test_context_history(lib):
    """every one-shot call on one context, one after the other, against the same call on a context that has done nothing"""
    import test_odometry as OT
    opt, spec_runs = odometry_spec_runs()
    calls = context_calls(lib)
    fresh = replay(lambda: lib.Context(0), [(name, None, call) for name, _, call in calls])
    by_name = dict(zip([name for name, _, _ in calls], fresh))
    for name in ("voxels of 20,000 points", "voxels of 50 points"):
        assert len(by_name[name][0]) > 0 and by_name[name][1] is not None and by_name[name][2] is not None
    # (rows that are all NaN: what comes out is not specified -- the reference casts floor(NaN) to int --, only that it does not
    # depend on the calls before)
    # the large pair and the small one after it against the specification (tests/test_odometry.py: test_hybrid_run_...)
    for name, (ok, T, M, ex) in (("odometry, 100 x 75", spec_runs[0]), ("odometry, 50 x 38", spec_runs[1])):
        success, got_T, info, info_pairs, pairs = by_name[name]
        assert success and pairs.tolist() == ex["counts"], name
        assert OT.rel(got_T, T) <= OT.TOL_T, name
        bound = OS.information_bound(ex["info_K"], ex["info_S"])
        assert info_pairs == ex["info_K"] == info[5, 5] and np.array_equal(info, info.T) and np.all(np.abs(info - M) <= bound), name


@pytest.mark.gpu
def test_context_calls_leave_the_registration_alone(lib):
    """the yardstick pattern of tests/test_tsdf.py (test_repeats_reset_two_volumes_and_icp_around): a pass, every one-shot call,
    then the SAME pass reduced again and its correspondences read again -- no call in between that would run the pass anew --,
    then a pass at a second pose: each equal, to the bit, to a context that ran the registration calls alone.  Last, the
    information matrix at the first pose, which is a registration call itself (it runs a pass on the context's clouds): after
    it the pass is a new one, so it comes after the check of the old one."""
    from visma_amd import synth
    src, tgt, _, r = synth.make_pair(2000, 8000, seed_t=13, seed_s=14)
    T0 = np.eye(4)
    T1 = tsdf_scene.rigid((0.01, -0.02, 0.015), (0.004, -0.003, 0.002))
    calls = [c for c in context_calls(lib) if c[0] != "information matrix"]     # (that step sets clouds of its own)

    def record(c):
        return (c.reduce(),) + tuple(c.get_correspondences())

    def registration(c, between):
        c.set_clouds_f64(src, tgt)
        c.nn_pass(T0, r)
        out = [record(c)]
        between(c)
        out.append(record(c))                                         # the same pass: no nn_pass, no call that makes one, since
        c.nn_pass(T1, r)
        out.append(record(c))
        M, k = c.information_matrix(T0, r)
        out.append((M, int(k)) + record(c))
        return out

    def every_call(c):
        for _, _, call in calls:
            call(c)

    plain = lib.Context(0)
    try:
        want = registration(plain, lambda c: None)
    finally:
        plain.close()
    busy = lib.Context(0)
    try:
        got = registration(busy, every_call)
    finally:
        busy.close()
    assert len(want[0][1]) > 500 and len(want[2][1]) > 500
    # (a second reduce of one pass searches warm, from the first one's winners, and need not equal the first to the bit: it is
    # held against the OTHER context's second reduce, as every step here is)
    for k, name in enumerate(("the first pass", "the same pass again, after every other call", "a pass at a second pose",
                              "the information matrix and its pass")):
        diff = difference(got[k], want[k])
        assert diff is None, "%s: %s" % (name, diff)


# ---------------------------------------------------------------------------
# zero after non-zero, by name: the sizes are 0, the downloads take NULL or empty arrays, the next call with rows equals fresh
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scalable", [False, True], ids=["uniform", "scalable"])
def test_an_extraction_without_rows_after_one_with_rows(ctx, scalable):
    """... and, for the scalable volume, no units after reset()"""
    case, script, spec, rows, initial = tsdf_spec_history(scalable, VS.COLOR_RGB8)
    frame = script[0][1]
    L, h = ctx.L, ctx._h
    i64 = C.c_int64

    def make():
        if scalable:
            return Vol(ctx.tsdf_scalable(case["voxel_length"], case["sdf_trunc"], VS.COLOR_RGB8, case["R"], case["stride"], initial_units=initial))
        return Vol(ctx.tsdf_uniform(case["length"], case["R"], case["sdf_trunc"], VS.COLOR_RGB8, case["origin"]))

    def filled(v):
        tsdf_integrate(v, frame)
        return tsdf_extract(v)

    def emptied(v):
        v.vol.reset()
        out = tsdf_extract(v)
        n, nv, nt = i64(-1), i64(-1), i64(-1)
        codes = [L.visma_icp_tsdf_extract_point_cloud(h, v.vol._v, C.byref(n)), L.visma_icp_tsdf_get_point_cloud(h, v.vol._v, None, None, None, 0),
                 L.visma_icp_tsdf_extract_voxel_point_cloud(h, v.vol._v, C.byref(n)), L.visma_icp_tsdf_get_voxel_point_cloud(h, v.vol._v, None, None, 0),
                 L.visma_icp_tsdf_extract_triangle_mesh(h, v.vol._v, C.byref(nv), C.byref(nt)),
                 L.visma_icp_tsdf_get_triangle_mesh(h, v.vol._v, None, None, None, 0, 0)]
        if scalable:
            codes.append(L.visma_icp_tsdf_get_units(h, v.vol._v, None, 0, C.byref(n)))
        return out, codes, [n.value, nv.value, nt.value]

    fresh = replay(make, [("a frame, extracted", None, filled), ("reset, extracted", lambda v: tsdf_integrate(v, frame), emptied),
                          ("a frame again, extracted", None, filled)])
    assert len(fresh[0]["pc"][0]) == rows[1] > 0 and len(fresh[0]["mesh"][2]) > 0
    out, codes, sizes = fresh[1]
    assert not any(codes) and sizes == [0, 0, 0], (codes, sizes)
    assert [len(a) for a in out["pc"]] == [0, 0, 0] and [len(a) for a in out["vx"]] == [0, 0] and [len(a) for a in out["mesh"]] == [0, 0, 0]
    assert out["copy_size"][:2] == (0, 0)
    if scalable:
        assert len(out["contents"][0]) == 0
    else:
        assert not out["contents"][1].any()
    assert same_bytes(fresh[2], fresh[0])


@pytest.mark.gpu
def test_a_radius_search_that_finds_nothing_after_one_that_finds_something(ctx):
    tree, steps, want, rows = kd_spec(2000)
    (_, q_some, s_some), (_, q_none, s_none) = steps[4], steps[3]
    assert rows[4] > 0 and rows[3] == 0

    def nothing(kd):
        off, idx, d2 = kd.search_radius(q_none, s_none[2])
        return off, idx, d2, ctx.L.visma_icp_kdtree_get_radius_result(kd._t, None, None)

    fresh = replay(lambda: ctx.kdtree(tree), [("a large total", None, lambda kd: kd.search_radius(q_some, s_some[2])), ("total 0", None, nothing),
                                              ("a large total again", None, lambda kd: kd.search_radius(q_some, s_some[2]))])
    off, idx, d2, rc = fresh[1]
    assert rc == 0 and not off.any() and len(off) == len(q_none) + 1 and len(idx) == 0 and len(d2) == 0
    assert fresh[0][0][-1] == rows[4] and same_bytes(fresh[2], fresh[0])
    KT.check(Recorded(fresh[2]), tree, q_some, s_some, want=want[4])


@pytest.mark.gpu
@pytest.mark.parametrize("non_rigid", [False, True], ids=["rigid", "non-rigid"])
def test_a_prepare_in_which_no_vertex_is_visible(lib, ctx, non_rigid):
    depths, colors, E, K, steps = cm_inputs()
    n, h, w = depths.shape
    V = steps[0]["V"]
    behind = np.ascontiguousarray(V[:700] * [1.0, 1.0, 0.0] + [0.0, 0.0, -3.0])         # behind every camera
    st = cm_spec_state(non_rigid, dict(frames=steps[0]["frames"], V=behind), depths, colors, E, K)
    assert not any(len(x) for x in st.lists)                                            # (the specification sees none either)
    option = lib.color_map_option(**{k: v for k, v in cm_option(non_rigid).items() if k != "non_rigid_camera_coordinate"})

    def make():
        m = (ctx.color_map_non_rigid if non_rigid else ctx.color_map)(w, h, n, K, option)
        for i in range(n):
            m.set_image(i, depths[i], colors[i], E[i])
        return m

    def run_on(vertices):
        def call(m):
            m.set_vertices(vertices)
            counts = m.prepare()
            out = dict(counts=counts, visible=[m.visible(c) for c in range(n)], proxy=m.proxy(), step=m.step_non_rigid() if non_rigid else m.step(),
                       colors=m.colors())
            m.set_extrinsics(E)                                                          # the poses of the next step: the first ones
            if non_rigid:
                out["flow"] = m.flow()
                m.set_flow(np.tile(st.flow_init, (n, 1)))
            return out
        return call

    fresh = replay(make, [("all vertices", None, run_on(V)), ("vertices no camera sees", None, run_on(behind)), ("all vertices again", None, run_on(V))])
    zero = fresh[1]
    assert not zero["counts"].any() and all(len(x) == 0 for x in zero["visible"])
    assert not zero["step"][-1].any() and not zero["step"][0].any()                      # count 0, rr 0.0 for every camera
    assert fresh[0]["counts"].sum() > 2000 and same_bytes(fresh[2], fresh[0])


@pytest.mark.gpu
def test_a_crop_that_keeps_nothing_then_purge(ctx):
    first = big16()
    far = ((50.0, 50.0, 50.0), (60.0, 60.0, 60.0))
    box = ((0.3, 0.3, -1.0), (0.9, 0.9, 1.0))                            # (the grid spans [0, 1.5625]^2; the unused band lies at y = -5)
    want = T.crop(first, *box)
    assert len(T.crop(first, *far)["vertices"]) == 0 and len(want["triangles"]) > 1000

    def cropped(lo, hi):
        def call(slot):
            child = slot.mesh.crop(lo, hi)
            try:
                removed = child.purge()
                got, size = child.get(), child.size()
                none = ctx.L.visma_icp_trimesh_get(ctx._h, child._m, None, None, None, None, None, size[0], size[1])
            finally:
                child.close()
            return removed, got, size, none
        return call

    fresh = replay(lambda: Slot(ctx, first), [("a crop with rows", None, cropped(*box)), ("a crop that keeps nothing", None, cropped(*far)),
                                              ("a crop with rows again", None, cropped(*box))])
    removed, got, size, none = fresh[1]
    assert removed == (0, 0, 0, 0) and size == (0, 0, 0) and none == 0
    assert got["vertices"].shape == (0, 3) and got["triangles"].shape == (0, 3) and got["vertex_normals"] is None
    assert same_bytes(fresh[2], fresh[0])
    MT.same(fresh[2][1], want, "crop")
