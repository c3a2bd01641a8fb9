// render_math.hpp -- the arithmetic of the mesh renderer, host+device: render.hip's kernels and visma_icp_render_host run
// these very functions, so there is one copy of the rule (tests/render_spec.py is the same rule in numpy).  Everything is
// f64, one rounding per operation (the build's -ffp-contract=off), in the operation order written here.
//
// The rule is rasterisation in its ray form (homogeneous edge functions): a pixel's ray d = ((x - cx)/fx, (y - cy)/fy, 1)
// meets the plane of the camera-space triangle (A, B, C) at depth z = det / s, inside the triangle where the three edge
// values e_i = n_i . d have one sign.  Nothing is clipped: a vertex behind the camera is like any other.  Vertices are
// projected only for the triangle's screen box (render_setup), which is part of the rule.  The cross products are written so that B x A is exactly -(A x B): two triangles that share an edge see exactly
// negated edge values there, so with the inclusive comparison no pixel between them is lost (and one on the edge is in both:
// the key decides).
//
// The per-pixel winner is the smallest 64-bit key (bits of (float)z << 32) | triangle: z > 0, so the fp32 bits order as the
// depths do; the nearest triangle after the rounding to fp32 wins, the lowest index among equals.  A minimum over integers
// does not depend on the order the candidates arrive in.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "so3.h"

namespace visma {

struct RenderCamera {
    int w, h;
    double fx, fy, cx, cy, z_near, z_far;
};

constexpr unsigned long long kRenderNoKey = ~0ull;       // background: above every key (z is never a NaN in a key)
constexpr int kRenderMetric = 0, kRenderDepthBuffer = 1;  // visma_icp.h's VISMA_ICP_RENDER_*

// a triangle after set-up: the three edge normals, det, and the screen box it is drawn in (x1 < x0: nothing to do)
struct RenderTri {
    double n0[3], n1[3], n2[3], det;
    int x0, y0, x1, y1;
};

// P = R X + t, the operation order of row_kernels.h's Transform (w = 1: its product with the fourth column is exact)
VISMA_HD void render_camera_point(const double *T, const double *X, double *P)
{
    for (int r = 0; r < 3; r++) P[r] = ((T[4 * r] * X[0] + T[4 * r + 1] * X[1]) + T[4 * r + 2] * X[2]) + T[4 * r + 3];
}

VISMA_HD void render_cross(const double *u, const double *v, double *n)
{
    n[0] = u[1] * v[2] - u[2] * v[1];
    n[1] = u[2] * v[0] - u[0] * v[2];
    n[2] = u[0] * v[1] - u[1] * v[0];
}

VISMA_HD bool render_finite3(const double *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the box of a span of projected coordinates, padded by one pixel and clamped to [0, last]; false: empty
VISMA_HD bool render_span(double lo, double hi, int last, int *a, int *b)
{
    if (!(isfinite(lo) && isfinite(hi))) { *a = 0; *b = last; return true; }
    lo = floor(lo) - 1.0; hi = ceil(hi) + 1.0;
    if (hi < 0.0 || lo > (double)last) return false;
    *a = lo < 0.0 ? 0 : (int)lo;
    *b = hi > (double)last ? last : (int)hi;
    return true;
}

// Set-up of one triangle.  The box is PART OF THE RULE: a triangle is drawn only at the pixels of its box, and tests/render_spec.py
// computes the same box.  Nothing where a camera coordinate is not finite or no vertex lies at z >= z_near (the depth of a
// covered pixel lies between the vertices' depths); the whole image where one or two vertices lie at z >= z_near (the
// triangle straddles that plane); where all three do, the projected vertices u = fx (X / Z) + cx, v = fy (Y / Z) + cy, from
// floor(min) - 1 to ceil(max) + 1, clamped to the image (a non-finite projection: the whole span; a box wholly off the image:
// nothing).  In exact arithmetic the box changes no pixel, it contains every pixel the triangle covers.  In f64 it does: the
// edge values of a degenerate triangle are rounding noise, and z = det / s is noise over noise that can land inside
// [z_near, z_far] anywhere on the image.  Measured against exact rationals (tests/test_render_spec.py): a triangle whose
// vertices lie on a line through the camera centre drew 114 pixels of a 32 x 24 image without the box and 0 in exact
// arithmetic; of 1000 random triangles of that family 215 drew pixels outside their box; of 3000 scenes with every vertex a
// few ulps under z_near, 1078 drew pixels without the cull (det / s rounds up to z_near) and none in exact arithmetic.
VISMA_HD void render_setup(const double *A, const double *B, const double *C, const RenderCamera &c, RenderTri &t)
{
    t.x0 = t.y0 = 0; t.x1 = t.y1 = -1;
    render_cross(B, C, t.n0);
    render_cross(C, A, t.n1);
    render_cross(A, B, t.n2);
    t.det = (A[0] * t.n0[0] + A[1] * t.n0[1]) + A[2] * t.n0[2];
    if (!(render_finite3(A) && render_finite3(B) && render_finite3(C))) return;
    const int front = (A[2] >= c.z_near ? 1 : 0) + (B[2] >= c.z_near ? 1 : 0) + (C[2] >= c.z_near ? 1 : 0);
    if (front == 0) return;
    if (front < 3) { t.x1 = c.w - 1; t.y1 = c.h - 1; return; }
    const double ua = c.fx * (A[0] / A[2]) + c.cx, ub = c.fx * (B[0] / B[2]) + c.cx, uc = c.fx * (C[0] / C[2]) + c.cx;
    const double va = c.fy * (A[1] / A[2]) + c.cy, vb = c.fy * (B[1] / B[2]) + c.cy, vc = c.fy * (C[1] / C[2]) + c.cy;
    int x0, x1, y0, y1;
    if (!render_span(fmin(ua, fmin(ub, uc)), fmax(ua, fmax(ub, uc)), c.w - 1, &x0, &x1)) return;
    if (!render_span(fmin(va, fmin(vb, vc)), fmax(va, fmax(vb, vc)), c.h - 1, &y0, &y1)) return;
    t.x0 = x0; t.x1 = x1; t.y0 = y0; t.y1 = y1;
}

VISMA_HD long long render_box_area(const RenderTri &t)
{
    return t.x1 < t.x0 || t.y1 < t.y0 ? 0 : (long long)(t.x1 - t.x0 + 1) * (long long)(t.y1 - t.y0 + 1);
}

// the depth of the triangle's plane along the ray of pixel (x, y), and whether the ray passes inside (inclusive, both
// windings); *z is det / s whatever the answer
VISMA_HD bool render_inside(const RenderTri &t, const RenderCamera &c, int x, int y, double *z)
{
    const double dx = ((double)x - c.cx) / c.fx, dy = ((double)y - c.cy) / c.fy;
    const double e0 = (t.n0[0] * dx + t.n0[1] * dy) + t.n0[2];
    const double e1 = (t.n1[0] * dx + t.n1[1] * dy) + t.n1[2];
    const double e2 = (t.n2[0] * dx + t.n2[1] * dy) + t.n2[2];
    const double s = (e0 + e1) + e2;
    *z = t.det / s;
    const bool pos = e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0, neg = e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0;
    return s != 0.0 && (pos || neg);
}

VISMA_HD unsigned render_float_bits(float f)
{
    unsigned u;
    memcpy(&u, &f, sizeof(u));
    return u;
}
VISMA_HD float render_bits_float(unsigned u)
{
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
}

// the key of triangle `index` at pixel (x, y), or kRenderNoKey where it is not drawn there
VISMA_HD unsigned long long render_key(const RenderTri &t, const RenderCamera &c, int x, int y, unsigned index)
{
    double z;
    if (!render_inside(t, c, x, y, &z)) return kRenderNoKey;
    if (!(z >= c.z_near && z <= c.z_far)) return kRenderNoKey;
    return ((unsigned long long)render_float_bits((float)z) << 32) | (unsigned long long)index;
}

// the value OpenGL's depth buffer holds for the metric depth z (the inverse of LinearizeDepth, renderer.h), not quantised
VISMA_HD double render_depth_buffer(double z, double z_near, double z_far)
{
    return (0.5 * ((z_far + z_near) - ((2.0 * z_near) * z_far) / z)) / (z_far - z_near) + 0.5;
}
VISMA_HD double render_linearize_depth(double zb, double z_near, double z_far)
{
    return ((2.0 * z_near) * z_far) / ((z_far + z_near) - (2.0 * zb - 1.0) * (z_far - z_near));
}

// what the resolve writes for a pixel's winning key
VISMA_HD void render_resolve(unsigned long long key, const RenderTri *tris, const RenderCamera &c, int x, int y, int encoding,
                             float *depth, int32_t *index, uint8_t *mask)
{
    if (key == kRenderNoKey) {
        *depth = encoding == kRenderDepthBuffer ? 1.0f : 0.0f;
        *index = -1;
        *mask = 0;
        return;
    }
    const unsigned tri = (unsigned)(key & 0xffffffffull);
    *index = (int32_t)tri;
    *mask = 255;
    if (encoding == kRenderDepthBuffer) {
        double z;
        (void)render_inside(tris[tri], c, x, y, &z);
        *depth = (float)render_depth_buffer(z, c.z_near, c.z_far);
    } else {
        *depth = render_bits_float((unsigned)(key >> 32));
    }
}

// edge_detection.frag on the metric depth image: v = depth, -1 where there is none (depth not > 0); 0 in a border of five
// pixels and on a background centre; else 0.25 (|W - E| + |S - N| + |NW - SE| + |SW - NE|) through the ramp 0.05 .. 0.10
VISMA_HD uint8_t render_edge(const float *depth, int w, int h, int x, int y)
{
    if (x < 5 || x >= w - 5 || y < 5 || y >= h - 5) return 0;
    const float *p = depth + (long long)y * w + x;
#define RENDER_V(dx, dy) (p[(long long)(dy) * w + (dx)] > 0.0f ? (double)p[(long long)(dy) * w + (dx)] : -1.0)
    if (RENDER_V(0, 0) == -1.0) return 0;
    const double delta = 0.25 * (((fabs(RENDER_V(-1, 0) - RENDER_V(1, 0)) + fabs(RENDER_V(0, 1) - RENDER_V(0, -1))) +
                                  fabs(RENDER_V(-1, -1) - RENDER_V(1, 1))) + fabs(RENDER_V(-1, 1) - RENDER_V(1, -1)));
#undef RENDER_V
    double cval;
    if (!(delta >= 0.05)) cval = 0.0;                        // (a NaN, from infinite depths: no edge)
    else if (delta >= 0.10) cval = 1.0;
    else cval = (delta - 0.05) / 0.05;
    return (uint8_t)(int)floor(255.0 * cval + 0.5);
}

}  // namespace visma
