"""Exact point -> triangle and point -> mesh squared distance (test helper).

Every f64 input is taken as the rational number it is (`fractions.Fraction`), and the
distance is computed from the definition, not from Ericson's region walk: the foot
of the perpendicular if it falls inside the triangle, otherwise the nearest of the
three edge segments.  A face without area falls back to its segments, a face whose
vertices coincide to that single point.  No rounding happens anywhere, so the
result is the yardstick the f64 implementations (oracle, libigl, the HIP kernels)
are measured against -- slowly: about 20 us per face and query.
"""
from fractions import Fraction

import numpy as np


def _vec(p):
    return tuple(Fraction(float(x)) for x in p)


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def point_segment_sqdist(p, a, b):
    """Exact squared distance of p to the segment ab (a == b: to the point)."""
    p, a, b = _vec(p), _vec(a), _vec(b)
    return _segment(p, a, b)


def _segment(p, a, b):
    ab, ap = _sub(b, a), _sub(p, a)
    l2 = _dot(ab, ab)
    if l2 == 0:
        return _dot(ap, ap)
    t = _dot(ap, ab) / l2
    t = min(max(t, Fraction(0)), Fraction(1))
    d = (ap[0] - t * ab[0], ap[1] - t * ab[1], ap[2] - t * ab[2])
    return _dot(d, d)


def point_triangle_sqdist(p, a, b, c):
    """Exact squared distance (a Fraction) of p to the triangle abc."""
    return _triangle(_vec(p), _vec(a), _vec(b), _vec(c))


def _triangle(p, a, b, c):
    ab, ac, ap = _sub(b, a), _sub(c, a), _sub(p, a)
    n = _cross(ab, ac)
    nn = _dot(n, n)
    if nn != 0:
        # barycentric coordinates of the foot of the perpendicular, times nn (> 0)
        v = _dot(_cross(ap, ac), n)
        w = _dot(_cross(ab, ap), n)
        if v >= 0 and w >= 0 and v + w <= nn:
            h = _dot(ap, n)
            return h * h / nn
    return min(_segment(p, a, b), _segment(p, b, c), _segment(p, c, a))


def point_mesh_sqdist(P, V, F, prefilter=True):
    """Exact squared distance of every row of P to the mesh (V, F).

    Returns (d2, faces): d2[i] a Fraction, faces[i] the sorted list of ALL faces that attain it.
    prefilter: faces whose bounding box is provably farther than the nearest vertex of some face are
    skipped (a rigorous f64 bound with a 1e-9 relative margin on both sides; it changes no result)."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    V = np.asarray(V, np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    T = V[F]                                               # nf x 3 x 3
    lo, hi = T.min(1), T.max(1)
    Vq = [_vec(v) for v in V]
    d2, faces = [], []
    for p in P:
        cand = np.arange(len(F))
        if prefilter and len(F) > 8 and np.isfinite(p).all():
            gap = np.maximum(np.maximum(lo - p, p - hi), 0.0)
            lb = (gap * gap).sum(1)
            ub = ((T - p) ** 2).sum(2).min()                # squared distance to the nearest referenced vertex
            cand = np.nonzero(lb * (1.0 - 1e-9) <= ub * (1.0 + 1e-9))[0]
        pq = _vec(p)
        best, arg = None, []
        for f in cand:
            d = _triangle(pq, Vq[F[f, 0]], Vq[F[f, 1]], Vq[F[f, 2]])
            if best is None or d < best:
                best, arg = d, [int(f)]
            elif d == best:
                arg.append(int(f))
        d2.append(best)
        faces.append(arg)
    return d2, faces
