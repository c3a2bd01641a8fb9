// mc_table.h -- the 256 marching-cubes cases of ExtractTriangleMesh, computed from a rule (no literal table).  Built on the
// host, no HIP header: tsdf.hip copies the table to the device, aux_api.cpp answers visma_icp_marching_cubes_case from it.
//
//  corners   bit i of a case: the corner at offset (i & 1, (i >> 1) & 1, (i >> 2) & 1) is inside (tsdf < 0)
//  edges     (lower corner, axis) has id 4 axis + j; j = the lower corner's two other coordinates, the earlier axis as
//            bit 0: ids 0 .. 3 the x edges at (y, z) = (0,0) (1,0) (0,1) (1,1), 4 .. 7 the y edges at (x, z), 8 .. 11 the z
//            edges at (x, y)
//  faces     on each of the six faces the cut edges are joined into segments, each cutting off one group of inside corners
//            connected along the face's edges -- a face with four cut edges (signs alternating) has two groups of one
//            corner.  Seen from outside the cube a segment runs with its inside corners on its right (kMcWindingSign = +1:
//            normals towards increasing tsdf, the reference's winding).  The rule reads a face's four signs only, so
//            the two cubes of a face agree on it: no cracks.
//  loops     every cut edge ends one segment and begins one: the segments close into loops.  Loops in the order of their
//            lowest edge id, each started there and fanned from its start: (l0, l1, l2), (l0, l2, l3), ...
// At most five triangles per case (computed and checked when the table is built; tests/test_mc_table.py).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define VISMA_MC_HD __host__ __device__
#else
#define VISMA_MC_HD
#endif

namespace visma {

constexpr int kMcMaxTriangles = 5;
constexpr int kMcWindingSign = 1;

struct McCase {
    uint8_t n;                                           // triangles
    uint8_t edge[3 * kMcMaxTriangles];                   // their edge ids
};
struct McTable { McCase c[256]; };

VISMA_MC_HD inline int mc_edge_id(int lower_corner, int axis)
{
    const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
    return 4 * axis + ((lower_corner >> u) & 1) + 2 * ((lower_corner >> v) & 1);
}
// -> the lower corner (as a corner number) of edge `id`; its axis is id / 4
VISMA_MC_HD inline int mc_edge_lower(int id)
{
    const int axis = id >> 2, j = id & 3;
    const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
    return ((j & 1) << u) | ((j >> 1) << v);
}

inline McCase mc_build_case(int cs)
{
    int next[12];
    for (int e = 0; e < 12; e++) next[e] = -1;
    for (int n = 0; n < 3; n++) {
        const int u = n == 0 ? 1 : 0, v = n == 2 ? 1 : 2;
        for (int side = 0; side < 2; side++) {
            auto corner = [&](int a, int b) { return (side << n) | (a << u) | (b << v); };
            auto inside = [&](int a, int b) { return (cs >> corner(a, b)) & 1; };
            const int k = inside(0, 0) + inside(1, 0) + inside(0, 1) + inside(1, 1);
            if (k == 0 || k == 4) continue;
            // the segments as (edge along u at b, edge along v at a) or two parallel edges, and a corner to turn about: an
            // inside corner of the group (flip = 0) or, where three are inside, the outside one (flip = 1)
            int seg[2][5];                               // e1, e2, a, b, flip
            int segs = 0;
            auto corner_segment = [&](int a, int b, int flip) {
                seg[segs][0] = mc_edge_id(corner(0, b), u); seg[segs][1] = mc_edge_id(corner(a, 0), v);
                seg[segs][2] = a; seg[segs][3] = b; seg[segs][4] = flip;
                segs++;
            };
            if (k == 1 || k == 3) {
                for (int a = 0; a < 2; a++)
                    for (int b = 0; b < 2; b++)
                        if (inside(a, b) == (k == 1)) corner_segment(a, b, k == 3);
            } else if (inside(0, 0) == inside(1, 1)) {   // the signs alternate: one segment per inside corner
                for (int a = 0; a < 2; a++)
                    for (int b = 0; b < 2; b++)
                        if (inside(a, b)) corner_segment(a, b, 0);
            } else {
                const bool along_u = inside(0, 0) == inside(1, 0);         // the inside pair lies along u: the v edges are cut
                seg[0][0] = along_u ? mc_edge_id(corner(0, 0), v) : mc_edge_id(corner(0, 0), u);
                seg[0][1] = along_u ? mc_edge_id(corner(1, 0), v) : mc_edge_id(corner(0, 1), u);
                const int b_in = along_u ? (inside(0, 0) ? 0 : 1) : 0, a_in = along_u ? 0 : (inside(0, 0) ? 0 : 1);
                seg[0][2] = a_in; seg[0][3] = b_in; seg[0][4] = 0;
                segs = 1;
            }
            for (int s = 0; s < segs; s++) {
                // in doubled cube coordinates: edge midpoints p1, p2, the corner c; turn = ((p2 - p1) x (c - p1)) . normal
                int p[2][3], c[3];
                for (int t = 0; t < 2; t++) {
                    const int id = seg[s][t], lo = mc_edge_lower(id);
                    for (int d = 0; d < 3; d++) p[t][d] = 2 * ((lo >> d) & 1);
                    p[t][id >> 2] = 1;
                }
                const int cc = corner(seg[s][2], seg[s][3]);
                for (int d = 0; d < 3; d++) c[d] = 2 * ((cc >> d) & 1);
                const int ax = p[1][u] - p[0][u], ay = p[1][v] - p[0][v], bx = c[u] - p[0][u], by = c[v] - p[0][v];
                // (u, v, n) is right-handed for n = 0 and 2, left-handed for n = 1
                int turn = (ax * by - ay * bx) * (n == 1 ? -1 : 1) * (side ? 1 : -1);
                if (seg[s][4]) turn = -turn;
                const bool swap = turn * kMcWindingSign > 0;
                next[seg[s][swap ? 1 : 0]] = seg[s][swap ? 0 : 1];
            }
        }
    }
    McCase out = {};
    bool seen[12] = {};
    for (int e = 0; e < 12; e++) {
        if (next[e] < 0 || seen[e]) continue;
        int loop[12], len = 0;
        for (int at = e; at >= 0 && !seen[at]; at = next[at]) { seen[at] = true; loop[len++] = at; }
        for (int i = 1; i + 1 < len; i++) {
            if (out.n == kMcMaxTriangles) { out.n = 0xff; return out; }    // (never: checked by mc_table())
            out.edge[3 * out.n] = (uint8_t)loop[0]; out.edge[3 * out.n + 1] = (uint8_t)loop[i]; out.edge[3 * out.n + 2] = (uint8_t)loop[i + 1];
            out.n++;
        }
    }
    return out;
}

inline const McTable &mc_table()
{
    static const McTable table = [] {
        McTable t;
        for (int cs = 0; cs < 256; cs++) t.c[cs] = mc_build_case(cs);
        return t;
    }();
    return table;
}

}  // namespace visma
