"""Plain Python / numpy references for the host half of find_chessboard_corners (board_detection.py:19-46): external
contours, contourArea, arcLength, approxPolyDP and the "largest four-cornered contour over 100000" rule.

Three layers, as for the HoughCircles checks:

1.  Definitions, wherever one exists.  Which components have an external contour, which pixels it holds, its area, its
    length: these follow from connectivity, the shoelace sum and Pick's theorem, and no border follower is needed to state
    them (external_border_sets, shoelace2, arc_length, filled_pixel_count).
2.  A second restatement, where the algorithm is the only definition.  The *order* of a contour's points is what border
    following produces, and the polygon is what OpenCV's Douglas-Peucker produces: there is nothing to derive them from,
    so moore_trace and approx_poly_closed state the two algorithms a second time, from their published descriptions
    (Suzuki & Abe 1985 as cv2.findContours applies it; cv2.approxPolyDP's closed-curve scheme), in another shape than the
    library's code: sets and coordinates, recursion, no marks written into the image.
3.  Known answers (tests/contour_cases.py).

Images are numpy arrays, non-zero = foreground.  Points are (x, y).  Nothing here imports the library, the oracle,
ref_logic or scipy.
"""
import math
from collections import deque

import numpy as np

SQRT2_F32 = float(np.float32(np.sqrt(np.float32(2.0))))     # cv2.arcLength takes each step's length in float32


# ---------------------------------------------------------------------------------------------------------------------
# layer 1: definitions
# ---------------------------------------------------------------------------------------------------------------------

N4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
N8 = N4 + ((1, 1), (1, -1), (-1, 1), (-1, -1))


def _padded(img):
    a = np.asarray(img) != 0
    p = np.zeros((a.shape[0] + 2, a.shape[1] + 2), bool)
    p[1:-1, 1:-1] = a
    return p


def _flood(free, seed, nbrs):
    """The pixels of the boolean map `free` (a list of lists) connected to seed through `nbrs`; free is consumed."""
    h, w = len(free), len(free[0])
    out = []
    q = deque([seed])
    free[seed[1]][seed[0]] = False
    while q:
        x, y = q.popleft()
        out.append((x, y))
        for dx, dy in nbrs:
            u, v = x + dx, y + dy
            if 0 <= u < w and 0 <= v < h and free[v][u]:
                free[v][u] = False
                q.append((u, v))
    return out


def outer_background(img):
    """Boolean map over the image padded by one zero pixel: the 4-connected background component that holds the padding."""
    p = _padded(img)
    out = np.zeros(p.shape, bool)
    for x, y in _flood((~p).tolist(), (0, 0), N4):
        out[y, x] = True
    return out


def components8(img):
    """The 8-connected foreground components, each a list of (x, y) in image coordinates whose first entry is the
    component's first pixel in raster order; the components themselves in raster order of that pixel."""
    a = np.asarray(img) != 0
    free = a.tolist()
    comps = []
    for y, x in zip(*np.nonzero(a)):            # raster order
        if free[y][x]:
            comps.append(_flood(free, (int(x), int(y)), N8))
    return comps


def external_border_sets(img):
    """[(component, border set)] for every component with a pixel 4-adjacent to the outer background, in raster order of
    the components' first pixels.  The border set is exactly the component's pixels with a 4-neighbour in the outer
    background: Suzuki-Abe's border point for 8-connected foreground.  A component inside a hole touches no outer
    background and does not appear."""
    outer = outer_background(img)
    res = []
    for comp in components8(img):
        border = {(x, y) for x, y in comp if any(outer[y + 1 + dy, x + 1 + dx] for dx, dy in N4)}
        if border:
            res.append((comp, border))
    return res


def shoelace2(pts):
    """sum(x_i y_{i+1} - x_{i+1} y_i) over the closed sequence, an exact integer: twice the signed area."""
    p = [(int(x), int(y)) for x, y in pts]
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(p, p[1:] + p[:1]))


def contour_area(pts):
    """cv2.contourArea: |shoelace| / 2, exact in double for any contour an image can hold."""
    return abs(shoelace2(pts)) / 2.0


def step_counts(pts):
    """(axial, diagonal) steps of the closed sequence; a sequence of fewer than two points has none."""
    p = [(int(x), int(y)) for x, y in pts]
    if len(p) < 2:
        return 0, 0
    ax = dg = 0
    for a, b in zip(p, p[1:] + p[:1]):
        d = abs(a[0] - b[0]) + abs(a[1] - b[1])
        assert d in (1, 2) and max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1, (a, b)
        ax += d == 1
        dg += d == 2
    return ax, dg


def arc_length(pts):
    """cv2.arcLength(closed=True) of an 8-connected contour: every step is 1 or float32(sqrt 2), summed in double."""
    ax, dg = step_counts(pts)
    return ax + dg * SQRT2_F32


def filled_pixel_count(comp, shape):
    """Pixels of the component with its holes filled: everything the component's own 4-connected outer background does
    not reach."""
    h, w = shape
    free = [[True] * (w + 2) for _ in range(h + 2)]
    for x, y in comp:
        free[y + 1][x + 1] = False
    return (h + 2) * (w + 2) - len(_flood(free, (0, 0), N4))


# ---------------------------------------------------------------------------------------------------------------------
# layer 2: the two algorithms, restated
# ---------------------------------------------------------------------------------------------------------------------

# the eight neighbours, counter-clockwise on the screen (y grows downwards), starting at the west one
RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def moore_trace(fg, start):
    """Moore-neighbour border following of the component of the pixel set `fg` whose first pixel in raster order is
    `start`.  The walk enters `start` from the west.  At every pixel the eight neighbours are examined counter-clockwise,
    beginning just after the pixel the walk came from, and the walk steps to the first one in fg; at the end of a
    one-pixel-wide line that is the pixel it came from, so such a line is traversed twice.  Suzuki-Abe's stopping rule:
    let `last` be the neighbour of `start` met last when going counter-clockwise from the west (the first one clockwise);
    the walk ends when it stands on `last` and its next step is `start`.  A component of one pixel is that pixel."""
    around = [(start[0] + dx, start[1] + dy) for dx, dy in RING]
    hits = [q for q in around if q in fg]
    if not hits:
        return [start]
    last = hits[-1]
    path = []
    cur, came = start, 0                        # `came`: ring index, seen from cur, of the pixel the walk came from
    while True:
        for t in range(1, 9):
            k = (came + t) % 8
            nxt = (cur[0] + RING[k][0], cur[1] + RING[k][1])
            if nxt in fg:
                break
        path.append(cur)
        if nxt == start and cur == last:
            return path
        cur, came = nxt, (k + 4) % 8


def external_contours(img):
    """The second restatement of cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE): moore_trace of every component that
    touches the outer background, listed from the component found last in raster order to the first."""
    out = []
    for comp, _ in external_border_sets(img):
        out.append(moore_trace(set(comp), comp[0]))
    return out[::-1]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def approx_poly_closed(pts, eps, clean_up=True):
    """cv2.approxPolyDP(pts, eps, closed=True), from OpenCV's description of it.

    Start search: beginning at point 0, three times over, take the point farthest from the current start (the first such
    in curve order) as the next start.  The third start S and the point F farthest from it cut the curve into S..F and
    F..S; when even F lies within eps of S the polygon is the single point S.
    Douglas-Peucker on each piece: the point farthest from the line through the piece's ends (the first such) splits the
    piece when it is farther than eps from that line; otherwise the piece contributes its first end.  Distances are
    compared squared: cross^2 <= eps^2 |chord|^2.
    Clean-up, one pass around the vertices in place (clean_up_pass)."""
    p = [(int(x), int(y)) for x, y in pts]
    n = len(p)
    if n == 0:
        return []
    e2 = float(eps) * float(eps)
    start = far = 0
    d2 = 0.0
    for _ in range(3):
        start = far
        best, far = 0.0, start
        for j in range(1, n):
            q = p[(start + j) % n]
            d = float((q[0] - p[start][0]) ** 2 + (q[1] - p[start][1]) ** 2)
            if d > best:
                best, far = d, (start + j) % n
        d2 = best
    if d2 <= e2:
        return [p[start]]
    out = []

    def piece(a, b):
        chord = float((p[b][0] - p[a][0]) ** 2 + (p[b][1] - p[a][1]) ** 2)
        best, split = 0.0, None
        i = (a + 1) % n
        while i != b:
            d = float(abs(_cross(p[a], p[b], p[i])))
            if d > best:
                best, split = d, i
            i = (i + 1) % n
        if split is None or best * best <= e2 * chord:
            out.append(p[a])
        else:
            piece(a, split)
            piece(split, b)

    piece(start, far)
    piece(far, start)
    return clean_up_pass(out, e2) if clean_up else out


def clean_up_pass(v, e2):
    """approxPolyDP's last pass over a closed polygon of three or more vertices.  Going once around, with A the last vertex
    kept, B the candidate and C the one after it: B is dropped when it lies within sqrt(1/2) eps of the line AC (squared:
    cross^2 <= 0.5 eps^2 |AC|^2), AC is not parallel to an axis, and (B - A) . (C - B) >= 0; A then moves to C, and two
    steps of the round are used up.  Otherwise A moves to B.  The pass stops at two vertices.  It runs in place: the kept
    vertices are written back over the start of the same array the round still reads from, as OpenCV does."""
    v = list(v)
    n = kept = len(v)
    if n < 3:
        return v
    a, b = v[n - 1], v[0]
    rd, wr, i = 1 % n, 0, 0
    while i < n and kept > 2:
        c = v[rd]
        rd = (rd + 1) % n
        dx, dy = c[0] - a[0], c[1] - a[1]
        dist = float(abs(_cross(a, b, c)))
        inner = (b[0] - a[0]) * (c[0] - b[0]) + (b[1] - a[1]) * (c[1] - b[1])
        if dist * dist <= 0.5 * e2 * float(dx * dx + dy * dy) and dx != 0 and dy != 0 and inner >= 0:
            kept -= 1
            v[wr] = a = c
            wr = (wr + 1) % n
            b = v[rd]
            rd = (rd + 1) % n
            i += 2
            continue
        v[wr] = a = b
        wr = (wr + 1) % n
        b = c
        i += 1
    return v[:kept]


# ---------------------------------------------------------------------------------------------------------------------
# invariants of the polygon that need no restatement
# ---------------------------------------------------------------------------------------------------------------------

def cyclic_subsequence_indices(poly, curve):
    """Indices into `curve` at which the vertices of `poly` occur, in order, going once around the closed curve from the
    first vertex's position; None when poly is no cyclic subsequence of curve."""
    c = [tuple(int(t) for t in q) for q in curve]
    v = [tuple(int(t) for t in q) for q in poly]
    n = len(c)
    if not v:
        return []
    for s in range(n):
        if c[s] != v[0]:
            continue
        idx, at = [s], 1
        for j in range(1, len(v)):
            while at < n and c[(s + at) % n] != v[j]:
                at += 1
            if at >= n:
                break
            idx.append((s + at) % n)
            at += 1
        else:
            return idx
    return None


def max_distance_to_bracket_lines(poly, curve, idx):
    """The largest distance from a point of the curve to the line through the two polygon vertices that bracket it
    (idx from cyclic_subsequence_indices).  A polygon of one vertex gives the largest distance to that vertex."""
    c = [(int(x), int(y)) for x, y in curve]
    n, m = len(c), len(idx)
    worst = 0.0
    for j in range(m):
        a, b = idx[j], idx[(j + 1) % m]
        pa, pb = c[a], c[b]
        length = math.hypot(pb[0] - pa[0], pb[1] - pa[1])
        i = a
        while True:
            d = abs(_cross(pa, pb, c[i])) / length if length > 0 else math.hypot(c[i][0] - pa[0], c[i][1] - pa[1])
            worst = max(worst, d)
            i = (i + 1) % n
            if i == b:
                break
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the decision rule
# ---------------------------------------------------------------------------------------------------------------------

def board_polygon(contours):
    """board_detection.py:30-46 on contours in cv2's order: a contour qualifies with contourArea strictly above 100000 and
    a four-vertex approxPolyDP(0.02 * arcLength); rectContour sorts the qualifying ones by area, largest first, with a
    stable sort, so among equal areas the one cv2 listed first stays first; getCornerPoints approximates that one again.
    Returns its four vertices, or None."""
    ok = [c for c in contours if contour_area(c) > 100000 and len(approx_poly_closed(c, 0.02 * arc_length(c))) == 4]
    ok = sorted(ok, key=contour_area, reverse=True)
    return approx_poly_closed(ok[0], 0.02 * arc_length(ok[0])) if ok else None
