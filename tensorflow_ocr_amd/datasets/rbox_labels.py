"""Host side of EAST's RBOX ground truth (Zhou et al., CVPR 2017, section 3.3): one rotated rectangle per text
quadrangle, and the shrunk quadrangle the score map is drawn from.  Float64 on the host (NumPy at the boundaries,
plain Python floats inside: the arrays are 4 x 2, where NumPy's call overhead is the whole cost), no torch: the decode
workers and the host tests import it.

The reference tree keeps only the HELPERS of EAST's label generator (datasets/icdar.py:202-407: shrink_poly,
point_dist_to_line, fit_line, line_cross_point, line_verticle, rectangle_from_parallelogram, sort_rectangle); the loop
that called them was rewritten for link labels.  The algorithm here is therefore BUILD-DEFINED from those helpers and the
paper, and parity with an upstream run is unpinned.  The helpers are restated as closed forms on normalised lines
(a, b, c), a x + b y + c = 0 with a^2 + b^2 = 1, which has no special case for vertical edges (the reference's
slope / intercept fit does, and fails on them).

    fit_rectangle(poly)   [4,2] clockwise (y down) -> (rect float32 [4,2], angle) | None for a degenerate polygon
    rect_lines(rect)      the four edge lines r0r1 (top), r1r2 (right), r2r3 (bottom), r3r0 (left), float64 [4,3]
    shrink_poly(poly, r)  the quadrangle moved inwards by R r_i along its edges (a copy)
    shrink_radii(poly)    r_i = the shorter of the two edges at vertex i (icdar.py:497-500)

Angle convention: the rectangle's right-pointing axis r0 -> r1 is (cos a, -sin a) with y down, a in (-pi/4, pi/4]: the
one `synthetic.rbox_labels` writes and `tool/rbox.decode` inverts.
"""
import math

import numpy as np

PARALLEL_EPS = 1e-9      # |sin| of the angle between two unit normals below which two lines count as parallel


def _points(a):
    return [tuple(p) for p in np.asarray(a, np.float64).reshape(4, 2).tolist()]


def _line(p, q):
    """Normalised line through p and q, or None when they coincide."""
    dx, dy = q[0] - p[0], q[1] - p[1]
    n = math.hypot(dx, dy)
    if not (n > 0.0 and math.isfinite(n)):
        return None
    a, b = dy / n, -dx / n
    return (a, b, -(a * p[0] + b * p[1]))


def _parallel_through(line, p):
    return (line[0], line[1], -(line[0] * p[0] + line[1] * p[1]))


def _dist(line, p):
    """point_dist_to_line (icdar.py:269-271) for a normalised line."""
    return abs(line[0] * p[0] + line[1] * p[1] + line[2])


def _cross(l1, l2):
    """line_cross_point (icdar.py:283-302); None for parallel lines."""
    det = l1[0] * l2[1] - l2[0] * l1[1]
    if not abs(det) > PARALLEL_EPS:
        return None
    return ((l1[1] * l2[2] - l2[1] * l1[2]) / det, (l2[0] * l1[2] - l1[0] * l2[2]) / det)


def _foot(line, p):
    """line_verticle + line_cross_point (icdar.py:305-314): the foot of the perpendicular from p."""
    d = line[0] * p[0] + line[1] * p[1] + line[2]
    return (p[0] - d * line[0], p[1] - d * line[1])


def _area(q):
    s = 0.0
    for k in range(4):
        a, b = q[k], q[(k + 1) % 4]
        s += a[0] * b[1] - a[1] * b[0]
    return 0.5 * abs(s)


def _parallelograms(poly):
    """The 8 candidates: per start vertex, A keeps p1 and moves the forward edge, B keeps p0 and moves the backward one."""
    out = []
    for i in range(4):
        p0, p1, p2, p3 = (poly[(i + k) % 4] for k in range(4))
        edge, forward, backward = _line(p0, p1), _line(p1, p2), _line(p0, p3)
        if edge is None or forward is None or backward is None:
            return None
        opposite = _parallel_through(edge, p2 if _dist(edge, p2) > _dist(edge, p3) else p3)
        # A
        q2 = _cross(forward, opposite)
        if q2 is None:
            return None
        fo = _parallel_through(forward, p0 if _dist(forward, p0) > _dist(forward, p3) else p3)
        q0, q3 = _cross(fo, edge), _cross(fo, opposite)
        if q0 is None or q3 is None:
            return None
        out.append((q0, p1, q2, q3))
        # B
        q3 = _cross(backward, opposite)
        if q3 is None:
            return None
        bo = _parallel_through(backward, p1 if _dist(backward, p1) > _dist(backward, p2) else p2)
        q1, q2 = _cross(bo, edge), _cross(bo, opposite)
        if q1 is None or q2 is None:
            return None
        out.append((p0, q1, q2, q3))
    return out


def rectangle_from_parallelogram(poly):
    """icdar.py:317-372: float32 [4,2] or None.  The angle at p0 against pi/2 and the longer side choose which two
    vertices stay; the other two become feet of perpendiculars."""
    p0, p1, p2, p3 = _points(poly)
    ux, uy, vx, vy = p1[0] - p0[0], p1[1] - p0[1], p3[0] - p0[0], p3[1] - p0[1]
    n01, n03 = math.hypot(ux, uy), math.hypot(vx, vy)
    if not (n01 > 0.0 and n03 > 0.0):
        return None
    angle_p0 = math.acos(max(-1.0, min(1.0, (ux * vx + uy * vy) / (n01 * n03))))
    if n01 > n03:
        l23, l01 = _line(p2, p3), _line(p0, p1)
        if l23 is None or l01 is None:
            return None
        if angle_p0 < 0.5 * math.pi:
            rect = [p0, _foot(l01, p2), p2, _foot(l23, p0)]
        else:
            rect = [_foot(l01, p3), p1, _foot(l23, p1), p3]
    else:
        l12, l03 = _line(p1, p2), _line(p0, p3)
        if l12 is None or l03 is None:
            return None
        if angle_p0 < 0.5 * math.pi:
            rect = [p0, _foot(l12, p0), p2, _foot(l03, p2)]
        else:
            rect = [_foot(l03, p1), p1, _foot(l12, p3), p3]
    return np.array(rect, dtype=np.float32)


def sort_rectangle(rect):
    """icdar.py:375-407 on a float32 rectangle: (rect rolled so that r0 is its top-left corner, angle); the angle is nan
    when the lowest vertex and its clockwise predecessor coincide."""
    r = _points(rect)
    ys = [p[1] for p in r]
    lowest = ys.index(max(ys))
    if ys.count(ys[lowest]) == 2:
        sums = [p[0] + p[1] for p in r]
        i0 = sums.index(min(sums))
        return rect[[(i0 + k) % 4 for k in range(4)]], 0.0
    right = (lowest - 1) % 4
    num, den = -(r[lowest][1] - r[right][1]), r[lowest][0] - r[right][0]
    if den != 0.0:
        angle = math.atan(num / den)
    else:
        angle = math.copysign(math.pi / 2, num) if num != 0.0 else math.nan
    if angle / math.pi * 180 > 45:
        i0 = (lowest - 2) % 4                     # the lowest vertex is r2
        return rect[[(i0 + k) % 4 for k in range(4)]], -(math.pi / 2 - angle)
    i0 = (lowest + 1) % 4                         # the lowest vertex is r3
    return rect[[(i0 + k) % 4 for k in range(4)]], angle


def rect_lines(rect):
    """float64 [4,3]: the normalised lines of r0r1, r1r2, r2r3, r3r0, or None when a side has no length."""
    r = _points(rect)
    lines = [_line(r[k], r[(k + 1) % 4]) for k in range(4)]
    if any(l is None for l in lines):
        return None
    return np.array(lines, np.float64)


def fit_rectangle(poly):
    """poly float [4,2], clockwise with y down -> (rect float32 [4,2], angle float), or None for a degenerate polygon (a
    zero-length edge, an intersection of parallel lines, a non-finite value).  The smallest of the 8 parallelograms
    around the quadrangle (first wins a tie), started at its smallest x + y, squared up and sorted."""
    poly = _points(np.asarray(poly, np.float64).reshape(4, 2))
    if not all(math.isfinite(c) for p in poly for c in p):
        return None
    cands = _parallelograms(poly)
    if cands is None:
        return None
    areas = [_area(c) for c in cands]
    if not all(math.isfinite(a) for a in areas):
        return None
    par = cands[areas.index(min(areas))]
    sums = [p[0] + p[1] for p in par]
    i0 = sums.index(min(sums))
    rect = rectangle_from_parallelogram([par[(i0 + k) % 4] for k in range(4)])
    if rect is None or not np.isfinite(rect).all():
        return None
    rect, angle = sort_rectangle(rect)
    if not math.isfinite(angle) or rect_lines(rect) is None:
        return None
    return rect, float(angle)


def shrink_radii(poly):
    """icdar.py:497-500: per vertex the shorter of its two edges."""
    p = _points(np.asarray(poly, np.float64).reshape(4, 2))
    edge = [math.hypot(p[i][0] - p[(i + 1) % 4][0], p[i][1] - p[(i + 1) % 4][1]) for i in range(4)]
    return [min(edge[i], edge[(i - 1) % 4]) for i in range(4)]


def shrink_poly(poly, r, R=0.3):
    """icdar.py:202-266 on a copy: both ends of every edge move towards each other along the edge, vertex i by R r_i;
    the longer pair of edges first, each direction taken from the vertices as they stand at that moment."""
    p = [list(q) for q in _points(np.asarray(poly, np.float64).reshape(4, 2))]

    def length(i, j):
        return math.hypot(p[j][0] - p[i][0], p[j][1] - p[i][1])

    def pull(i, j):
        n = length(i, j)
        ux, uy = ((p[j][0] - p[i][0]) / n, (p[j][1] - p[i][1]) / n) if n > 0.0 else (1.0, 0.0)
        p[i][0] += R * r[i] * ux
        p[i][1] += R * r[i] * uy
        p[j][0] -= R * r[j] * ux
        p[j][1] -= R * r[j] * uy

    order = [(0, 1), (3, 2), (0, 3), (1, 2)] if length(0, 1) + length(2, 3) > length(0, 3) + length(1, 2) else \
        [(0, 3), (1, 2), (0, 1), (3, 2)]
    for i, j in order:
        pull(i, j)
    return np.array(p, np.float64)
