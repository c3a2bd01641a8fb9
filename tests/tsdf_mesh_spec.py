"""A numpy specification of TSDF ExtractTriangleMesh (marching cubes) as include/visma_icp.h defines it: the case rule, the
vertex arithmetic of Open3D's UniformTSDFVolume / ScalableTSDFVolume ::ExtractTriangleMesh, and this library's order.

  cubes      uniform: every (x, y, z) in [0, R - 2]^3; scalable: every voxel of every unit, the corners beyond the unit read
             from the unit next door, a missing unit reads weight 0.  A cube is VALID iff its eight weights are != 0.  A
             corner is INSIDE iff tsdf < 0 (-0.0 is outside).  There is no tsdf range test.
  case       bit i of a cube's case: the corner at offset (i & 1, (i >> 1) & 1, (i >> 2) & 1) is inside
  edges      a cube edge is (lower corner, axis); its id is 4 axis + j, j = the lower corner's two other coordinates, the
             earlier axis as bit 0: x edges at (y, z), y edges at (x, z), z edges at (x, y)
  vertices   one per voxel edge (lower voxel, axis) whose ends differ in sign and which lies on a valid cube: f64,
             p = half + vl * index per component, p[axis] += f0 * vl / (f0 + f1), f = |(double)tsdf|; uniform: + origin;
             colour (f1 c0 + f0 c1) / (f0 + f1), c = (double)colour (/ 255.0 for RGB8)
  order      vertices by (unit, x, y, z, axis) of the edge's lower voxel, units in lexicographic index order; triangles by
             cube in the same order, within a cube in the order of the case rule

The case rule (case_table): on each of the six faces the cut edges are joined into segments that each cut off one group of
inside corners connected along the face's edges (a face whose signs alternate has two such groups of one corner); seen from
outside the cube a segment runs with the inside corners on one fixed side (WINDING_SIGN decides which); every cut edge then
ends one segment and begins one, the segments close into loops; loops in the order of their lowest edge id, each started
there, fanned from its start."""
import numpy as np

import tsdf_spec as S

F32, F64 = np.float32, np.float64
# the sign of normal . (direction of increasing tsdf) of every triangle: measured on the reference's meshes by
# tests/golden/gen_tsdf_mesh.py (stored as winding_sign in tests/golden/tsdf_mesh.npz, compared by the tests)
WINDING_SIGN = 1


def corner_offset(i):
    return np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1])


def edge_id(lower, axis):
    """lower: the lower corner's offset (its `axis` component 0)"""
    others = [a for a in range(3) if a != axis]
    return 4 * axis + int(lower[others[0]]) + 2 * int(lower[others[1]])


def edge_of(eid):
    """-> lower corner offset, axis"""
    axis, j = divmod(eid, 4)
    others = [a for a in range(3) if a != axis]
    lower = np.zeros(3, int)
    lower[others[0]], lower[others[1]] = j & 1, j >> 1
    return lower, axis


EDGE_LOWER = np.array([edge_of(e)[0] for e in range(12)])
EDGE_AXIS = np.array([edge_of(e)[1] for e in range(12)])


def cut_edges(case):
    out = []
    for e in range(12):
        lo = EDGE_LOWER[e]; hi = lo.copy(); hi[EDGE_AXIS[e]] = 1
        b0 = (case >> (lo[0] + 2 * lo[1] + 4 * lo[2])) & 1
        b1 = (case >> (hi[0] + 2 * hi[1] + 4 * hi[2])) & 1
        if b0 != b1:
            out.append(e)
    return out


def face_segments(case, axis, side, winding_sign=WINDING_SIGN):
    """the directed segments [(from edge id, to edge id)] on the face `axis` = `side` of a cube of that case"""
    u, v = [a for a in range(3) if a != axis]
    normal = np.zeros(3); normal[axis] = 1.0 if side else -1.0

    def corner(a, b):
        c = np.zeros(3, int); c[axis], c[u], c[v] = side, a, b
        return c

    def inside(a, b):
        c = corner(a, b)
        return bool((case >> (c[0] + 2 * c[1] + 4 * c[2])) & 1)

    def edge_along(ax, fixed):                       # the face edge along `ax` (u or v), the other coordinate = fixed
        c = corner(0, fixed) if ax == u else corner(fixed, 0)
        return edge_id(c, ax)

    def midpoint(e):
        m = EDGE_LOWER[e].astype(float); m[EDGE_AXIS[e]] = 0.5
        return m

    # the groups of inside corners connected along the face's edges
    ins = [(a, b) for a in (0, 1) for b in (0, 1) if inside(a, b)]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2 and ins[0][0] != ins[1][0] and ins[0][1] != ins[1][1]:
        groups = [[ins[0]], [ins[1]]]
    else:
        groups = [ins]
    out = []
    for g in groups:
        # the face edges that leave the group: one end in it, the other not
        ends = []
        for b in (0, 1):
            if ((0, b) in g) != ((1, b) in g):
                ends.append(edge_along(u, b))
        for a in (0, 1):
            if ((a, 0) in g) != ((a, 1) in g):
                ends.append(edge_along(v, a))
        assert len(ends) == 2
        p1, p2 = midpoint(ends[0]), midpoint(ends[1])
        c = corner(*g[0]).astype(float)
        turn = float(np.dot(np.cross(p2 - p1, c - p1), normal))
        assert turn != 0.0
        # normals towards increasing tsdf (winding_sign = +1): the inside corners lie where turn < 0
        if turn * winding_sign > 0:
            ends.reverse()
        out.append((ends[0], ends[1]))
    return out


def case_triangles(case, winding_sign=WINDING_SIGN):
    """-> [(e0, e1, e2)] the triangles of a case as edge ids"""
    nxt = {}
    for axis in range(3):
        for side in (0, 1):
            for a, b in face_segments(case, axis, side, winding_sign):
                assert a not in nxt
                nxt[a] = b
    cut = cut_edges(case)
    assert sorted(nxt) == cut and sorted(nxt.values()) == cut
    seen, tris = set(), []
    for e in cut:
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        assert len(loop) >= 3
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


_TABLES = {}


def case_table(winding_sign=WINDING_SIGN):
    """-> n (256) triangles per case, edges (256 x max x 3) edge ids, -1 beyond n"""
    if winding_sign not in _TABLES:
        rows = [case_triangles(c, winding_sign) for c in range(256)]
        most = max(len(r) for r in rows)
        n = np.array([len(r) for r in rows])
        edges = np.full((256, most, 3), -1, np.int64)
        for c, r in enumerate(rows):
            if r:
                edges[c, :len(r)] = np.array(r)
        _TABLES[winding_sign] = (n, edges)
    return _TABLES[winding_sign]


# ---------------------------------------------------------------------------
# extraction
# ---------------------------------------------------------------------------
def _extract_dense(f, w, c, base_ok, R, index0, vl, color_type, origin, winding_sign, with_edges=False):
    """f, w (X x Y x Z fp32), c (X x Y x Z x 3 or None): voxels, padded so that every cube base and every neighbour of a
    vertex edge is inside; base_ok: which voxels are cube bases; index0: the global voxel index of voxel (0, 0, 0);
    unit key of a voxel = floor(global index / R)"""
    X, Y, Z = f.shape
    inside = f < F32(0.0)
    live = w != F32(0.0)
    # cubes, keyed by their base voxel
    valid = base_ok.copy()
    case = np.zeros((X, Y, Z), np.int64)
    for i in range(8):
        d = corner_offset(i)
        sl = tuple(slice(d[a], (X, Y, Z)[a] - 1 + d[a]) for a in range(3))
        valid[:-1, :-1, :-1] &= live[sl]
        case[:-1, :-1, :-1] |= inside[sl].astype(np.int64) << i
    valid[-1, :, :] = False; valid[:, -1, :] = False; valid[:, :, -1] = False
    case[~valid] = 0
    # vertex edges (lower voxel, axis)
    carries = np.zeros((X, Y, Z, 3), bool)
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        up = np.roll(inside, -1, axis)
        cut = inside != up
        idx = [slice(None)] * 3; idx[axis] = -1
        cut[tuple(idx)] = False
        around = np.zeros((X, Y, Z), bool)
        for du in (0, 1):
            for dv in (0, 1):
                sh = np.roll(np.roll(valid, du, u), dv, v)
                if du:
                    i2 = [slice(None)] * 3; i2[u] = 0; sh[tuple(i2)] = False
                if dv:
                    i2 = [slice(None)] * 3; i2[v] = 0; sh[tuple(i2)] = False
                around |= sh
        carries[..., axis] = cut & around
    vx, vy, vz, va = np.nonzero(carries)
    g = np.stack([vx, vy, vz], 1) + np.asarray(index0, np.int64)[None, :]
    unit, local = np.floor_divide(g, R), np.mod(g, R)
    order = np.lexsort((va, local[:, 2], local[:, 1], local[:, 0], unit[:, 2], unit[:, 1], unit[:, 0]))
    vx, vy, vz, va, g = vx[order], vy[order], vz[order], va[order], g[order]
    nv = len(vx)
    vid = np.full((X, Y, Z, 3), -1, np.int64)
    vid[vx, vy, vz, va] = np.arange(nv)
    half = vl * 0.5
    pts = half + vl * g.astype(F64)
    up = np.stack([vx, vy, vz], 1); up[np.arange(nv), va] += 1
    f0 = np.abs(f[vx, vy, vz].astype(F64)); f1 = np.abs(f[up[:, 0], up[:, 1], up[:, 2]].astype(F64))
    with np.errstate(all="ignore"):
        pts[np.arange(nv), va] += f0 * vl / (f0 + f1)
        if origin is not None:
            pts = pts + np.asarray(origin, F64)[None, :]
        colors = None
        if color_type != S.COLOR_NONE:
            c0 = c[vx, vy, vz].astype(F64); c1 = c[up[:, 0], up[:, 1], up[:, 2]].astype(F64)
            if color_type == S.COLOR_RGB8:
                c0 = c0 / 255.0; c1 = c1 / 255.0
            colors = (f1[:, None] * c0 + f0[:, None] * c1) / (f0 + f1)[:, None]
    # triangles
    n_of, edges_of = case_table(winding_sign)
    bx, by, bz = np.nonzero(valid & (n_of[case] > 0))
    gb = np.stack([bx, by, bz], 1) + np.asarray(index0, np.int64)[None, :]
    unit, local = np.floor_divide(gb, R), np.mod(gb, R)
    order = np.lexsort((local[:, 2], local[:, 1], local[:, 0], unit[:, 2], unit[:, 1], unit[:, 0]))
    b = np.stack([bx, by, bz], 1)[order]
    E = edges_of[case[b[:, 0], b[:, 1], b[:, 2]]]                     # cubes x max x 3
    keep = E[..., 0] >= 0
    Ec = np.where(E >= 0, E, 0)
    lower = b[:, None, None, :] + EDGE_LOWER[Ec]
    tri = vid[lower[..., 0], lower[..., 1], lower[..., 2], EDGE_AXIS[Ec]][keep]
    assert (tri >= 0).all()
    tri = tri.astype(np.int32).reshape(-1, 3)
    if with_edges:
        # per vertex: the direction of increasing tsdf along its edge (+axis where the lower end is inside)
        rising = np.zeros((nv, 3))
        rising[np.arange(nv), va] = np.where(inside[vx, vy, vz], 1.0, -1.0)
        return pts, colors, tri, rising
    return pts, colors, tri


def extract_uniform(vol, winding_sign=WINDING_SIGN, with_edges=False):
    """vol: a tsdf_spec volume dict -> vertices (n x 3 f64), colors (n x 3 f64 or None), triangles (m x 3 int32)"""
    R = vol["R"]
    pad = lambda a: np.pad(a.reshape((R, R, R) + a.shape[1:]), [(1, 1)] * 3 + [(0, 0)] * (a.ndim - 1))
    f, w = pad(vol["tsdf"]), pad(vol["weight"])
    c = pad(vol["color"]) if vol["color_type"] != S.COLOR_NONE else None
    base_ok = np.zeros(f.shape, bool)
    if R >= 2:
        base_ok[1:R, 1:R, 1:R] = True                                  # [0, R - 2]^3
    return _extract_dense(f, w, c, base_ok, 1 << 40, (-1, -1, -1), vol["voxel_length"], vol["color_type"], vol["origin"], winding_sign, with_edges)


def extract_scalable(svol, winding_sign=WINDING_SIGN, with_edges=False):
    """svol: a tsdf_spec scalable volume dict (units: {index: volume})"""
    if not svol["units"]:
        return np.zeros((0, 3)), (None if svol["color_type"] == S.COLOR_NONE else np.zeros((0, 3))), np.zeros((0, 3), np.int32)
    R = svol["R"]
    f, w, c, present, lo = S._dense(svol)
    base_ok = np.repeat(np.repeat(np.repeat(present, R, 0), R, 1), R, 2)
    return _extract_dense(f, w, c, base_ok, R, lo * R, svol["voxel_length"], svol["color_type"], None, winding_sign, with_edges)


# ---------------------------------------------------------------------------
# what the tests measure of a mesh
# ---------------------------------------------------------------------------
def sort_rows_bits(*arrays):
    """rows of the (n x 3 f64) arrays side by side, sorted lexicographically by their bits"""
    a = np.concatenate([np.ascontiguousarray(x, F64) for x in arrays], 1)
    bits = a.view(np.uint64)
    order = np.lexsort(tuple(bits[:, k] for k in range(bits.shape[1] - 1, -1, -1)))
    return a[order]


def directed_edges(tri):
    t = np.asarray(tri, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def mesh_stats(vertices, tri):
    """-> euler (V - E + F over the vertices used), boundary (the undirected edges used by exactly one triangle, as sorted
    rows of the two ends' positions, 6 f64), repeated (directed edges that occur more than once)"""
    d = directed_edges(tri)
    und = np.sort(d, 1)
    uniq, counts = np.unique(und, axis=0, return_counts=True) if len(und) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    used = np.unique(np.asarray(tri)) if len(tri) else np.zeros(0, np.int64)
    euler = len(used) - len(uniq) + len(tri)
    b = uniq[counts == 1]
    ends = np.stack([vertices[b[:, 0]], vertices[b[:, 1]]], 1) if len(b) else np.zeros((0, 2, 3))
    # the two ends in the order of their bits, then the rows
    rows = []
    for p, q in ends:
        rows.append(np.concatenate([p, q]) if tuple(p.view(np.uint64)) <= tuple(q.view(np.uint64)) else np.concatenate([q, p]))
    rows = np.array(rows, F64).reshape(-1, 6)
    if len(rows):
        bits = rows.view(np.uint64)
        rows = rows[np.lexsort(tuple(bits[:, k] for k in range(5, -1, -1)))]
    dd, dc = np.unique(d, axis=0, return_counts=True) if len(d) else (d, np.zeros(0, np.int64))
    return int(euler), rows, int(np.count_nonzero(dc > 1))


def winding_dots(vertices, tri, rising):
    """per triangle of non-zero area: normal . (the sum of its three vertices' directions of increasing tsdf, each along
    the vertex's voxel edge from the inside end to the outside end); also the number of triangles of zero area"""
    a, b, c = vertices[tri[:, 0]], vertices[tri[:, 1]], vertices[tri[:, 2]]
    n = np.cross(b - a, c - a)
    keep = np.linalg.norm(n, axis=1) > 0
    d = rising[tri[:, 0]] + rising[tri[:, 1]] + rising[tri[:, 2]]
    return (n * d).sum(1)[keep], int(np.count_nonzero(~keep))
