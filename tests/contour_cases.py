"""Cases for the find_chessboard_corners checks (tests/test_contours_host.py, tests/test_gpu_corners.py): binary images for
the contour layers, rasterised polygons, the decision rule's known answers, and the shapes and contents of the pixel
stages.  Plain numpy, seeded; nothing is read from a file."""
import math

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# binary images for the contour layers
# ---------------------------------------------------------------------------------------------------------------------


def _smooth_noise(h, w, rng, passes):
    f = rng.random((h, w))
    for _ in range(passes):
        p = np.pad(f, 1, mode="edge")
        f = sum(p[i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0
    return f


def blob_cases():
    """Thresholded smooth noise, 24 x 24 to 96 x 96, three densities: the family the Pick identity is counted on."""
    out = []
    for n, (h, w) in enumerate(((24, 24), (31, 47), (48, 40), (64, 64), (77, 96), (96, 96))):
        for density in (0.25, 0.45, 0.65):
            rng = np.random.default_rng(4100 + 10 * n + int(density * 100))
            f = _smooth_noise(h, w, rng, 2 + n % 3)
            out.append(("blob_%dx%d_%d" % (h, w, int(density * 100)), (f <= np.quantile(f, density)).astype(np.uint8) * 255))
    return out


def _spiral(n):
    a = np.zeros((n, n), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    run = n - 1
    a[0, 0] = 255
    legs = 0
    while run > 0:                              # legs of n-1, n-1, n-1, n-3, n-3, n-5, n-5, ...: one pixel wide, one pixel apart
        for _ in range(run):
            x, y = x + dx, y + dy
            a[y, x] = 255
        dx, dy = -dy, dx
        legs += 1
        if legs >= 3 and (legs - 3) % 2 == 0:
            run -= 2
    return a


def shape_cases():
    """One-pixel-wide lines, crosses and spirals, staircases, components on every border, rings with blobs in their holes,
    diagonal touches, a full image, single pixels."""
    out = []
    z = lambda h, w: np.zeros((h, w), np.uint8)
    a = z(9, 12); a[4, 2:10] = 255; out.append(("hline", a))
    a = z(12, 9); a[2:10, 4] = 255; out.append(("vline", a))
    a = z(1, 7); a[:] = 255; out.append(("row_image", a))
    a = z(7, 1); a[:] = 255; out.append(("column_image", a))
    a = z(12, 12); a[np.arange(2, 10), np.arange(2, 10)] = 255; out.append(("diagonal", a))
    a = z(12, 12); a[np.arange(2, 10), 11 - np.arange(2, 10)] = 255; out.append(("antidiagonal", a))
    a = z(15, 15); a[7, 1:14] = 255; a[1:14, 7] = 255; out.append(("cross", a))
    a = z(15, 15); i = np.arange(1, 14); a[i, i] = 255; a[i, 14 - i] = 255; out.append(("x_cross", a))
    a = z(11, 11); a[5, 0:11] = 255; a[0:11, 5] = 255; out.append(("cross_to_borders", a))
    a = z(12, 14); a[3, 2:12] = 255; a[3:10, 7] = 255; out.append(("t_shape", a))
    out.append(("spiral_17", _spiral(17)))
    out.append(("spiral_24", _spiral(24)))
    a = z(20, 20)
    for k in range(8):
        a[2 + 2 * k:4 + 2 * k, 2 + 2 * k:4 + 2 * k] = 255
    out.append(("staircase_2x2", a))
    a = z(20, 24)
    for k in range(6):
        a[2 + 2 * k, 2 + 3 * k:6 + 3 * k] = 255
        a[3 + 2 * k, 5 + 3 * k] = 255
    out.append(("staircase_thin", a))
    a = z(16, 16)
    for k in range(7):
        a[14 - 2 * k:16 - 2 * k, 2 * k:2 * k + 3] = 255
    out.append(("staircase_up", a))
    a = z(14, 18); a[0, :] = 255; a[-1, 3:9] = 255; a[4:9, 0] = 255; a[6:12, -1] = 255; a[13, 17] = 255; out.append(("on_every_border", a))
    a = z(10, 10); a[0, 0] = a[0, 9] = a[9, 0] = a[9, 9] = 255; out.append(("corner_pixels", a))
    a = z(30, 34); a[2:28, 2:32] = 255; a[5:25, 5:29] = 0; a[8:12, 8:14] = 255; a[15:22, 16:26] = 255; a[17:20, 19:23] = 0
    a[18, 20] = 255; out.append(("ring_with_blobs", a))
    a = z(22, 22); a[1:21, 1:21] = 255; a[3:19, 3:19] = 0; a[5:17, 5:17] = 255; a[7:15, 7:15] = 0; a[10, 10] = 255
    out.append(("nested_rings", a))
    a = z(18, 18); a[1:17, 1] = 255; a[1:17, 16] = 255; a[16, 1:17] = 255; a[3:9, 6:11] = 255; a[12, 8] = 255
    out.append(("cup_with_blobs", a))                # open at the top: the blobs inside touch the outer background
    a = z(12, 12); a[2:6, 2:6] = 255; a[6:10, 6:10] = 255; out.append(("diagonal_touch", a))
    a = z(12, 12); a[2:6, 6:10] = 255; a[6:10, 2:6] = 255; out.append(("antidiagonal_touch", a))
    a = z(9, 9); a[1::2, 1::2] = 255; a[2::2, 2::2] = 255; out.append(("checker_diagonals", a))
    a = z(12, 12); a[2:10, 2:10] = 255; a[3:9, 3:9] = 0; a[2, 2] = 0; out.append(("ring_open_at_a_corner", a))
    out.append(("full", np.full((13, 17), 255, np.uint8)))
    out.append(("full_1x1", np.full((1, 1), 255, np.uint8)))
    out.append(("empty", z(6, 7)))
    a = z(7, 9); a[3, 4] = 255; out.append(("single_pixel", a))
    a = z(9, 9); a[1, 1] = a[1, 3] = a[3, 1] = a[7, 7] = a[4, 4] = 255; out.append(("single_pixels", a))
    a = z(8, 8); a[2, 2:4] = 255; out.append(("two_pixels", a))
    a = z(8, 8); a[2, 2] = a[3, 3] = 255; out.append(("two_pixels_diagonal", a))
    a = z(8, 8); a[2, 2] = a[2, 3] = a[3, 2] = 255; out.append(("three_pixels", a))
    a = z(8, 8); a[2, 3] = a[3, 2] = a[3, 3] = 255; out.append(("three_pixels_first_alone", a))
    a = z(10, 10); a[2, 5] = 255; a[3, 4] = a[3, 6] = 255; a[4, 3] = a[4, 7] = 255; a[5, 4] = a[5, 6] = 255; a[6, 5] = 255
    out.append(("diamond_outline", a))
    a = np.array([[7, 0, 1], [0, 200, 0], [255, 0, 3]], np.uint8); out.append(("non_zero_values", a))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# polygons
# ---------------------------------------------------------------------------------------------------------------------


def convex_mask(h, w, verts):
    """The pixels (integer points) inside or on the convex polygon with integer vertices `verts`, either orientation."""
    yy, xx = np.mgrid[:h, :w].astype(np.int64)
    n = len(verts)
    s = [(verts[(i + 1) % n][0] - verts[i][0]) * (yy - verts[i][1]) - (verts[(i + 1) % n][1] - verts[i][1]) * (xx - verts[i][0])
         for i in range(n)]
    return np.all([t >= 0 for t in s], axis=0) | np.all([t <= 0 for t in s], axis=0)


def polygon_cases():
    """Rasterised convex k-gons, k = 3..8, each at twelve rotations: (name, image, integer vertices).  The vertices lie on
    an ellipse whose axes change with k, so the polygons are neither regular nor aligned with the axes."""
    out = []
    size = 150
    for k in range(3, 9):
        for rot in range(12):
            phase = 2 * math.pi * rot / (12 * k) + 0.11 * k
            rx, ry = 66 - 2 * k, 48 + 2 * k
            verts = [(int(round(75 + rx * math.cos(phase + 2 * math.pi * i / k))), int(round(75 + ry * math.sin(phase + 2 * math.pi * i / k))))
                     for i in range(k)]
            out.append(("%d-gon_rot%d" % (k, rot), convex_mask(size, size, verts).astype(np.uint8) * 255, verts))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the decision rule's known answers
# ---------------------------------------------------------------------------------------------------------------------


def _disc(h, w, cx, cy, r):
    yy, xx = np.mgrid[:h, :w]
    return (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r


def decision_cases():
    """(name, image, expected): expected is None (nothing qualifies) or the set of the winning polygon's four vertices."""
    out = []
    a = np.zeros((260, 410), np.uint8); a[4:255, 3:404] = 255                      # 401 x 251 pixels: area 400 * 250
    out.append(("rect_area_100000_refused", a, None))
    a = np.zeros((260, 410), np.uint8); a[4:256, 3:404] = 255                      # 401 x 252 pixels: area 400 * 251
    out.append(("rect_area_100400_accepted", a, {(3, 4), (403, 4), (403, 255), (3, 255)}))
    a = np.zeros((330, 660), np.uint8); a[5:325, 4:324] = 255; a[5:325, 334:654] = 255   # same rows: the right one is found later
    out.append(("equal_squares_side_by_side", a, {(334, 5), (653, 5), (653, 324), (334, 324)}))
    a = np.zeros((660, 330), np.uint8); a[4:324, 5:325] = 255; a[334:654, 3:323] = 255
    out.append(("equal_squares_stacked", a, {(3, 334), (322, 334), (322, 653), (3, 653)}))
    a = _disc(400, 400, 200, 200, 190).astype(np.uint8) * 255                       # area about 113000
    out.append(("large_disc_refused", a, None))
    pent = [(int(round(230 + 220 * math.cos(0.3 + 2 * math.pi * i / 5))), int(round(230 + 220 * math.sin(0.3 + 2 * math.pi * i / 5)))) for i in range(5)]
    out.append(("large_pentagon_refused", convex_mask(460, 460, pent).astype(np.uint8) * 255, None))
    a = np.zeros((420, 760), np.uint8)
    a[_disc(420, 760, 205, 210, 200)] = 255                                          # area about 125000, no quadrilateral
    quad = [(430, 40), (745, 60), (735, 390), (420, 370)]                            # area about 103000
    a[convex_mask(420, 760, quad)] = 255
    out.append(("quad_beside_larger_disc", a, set(quad)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pixel stages (tests/test_gpu_corners.py)
# ---------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (7, 7), (13, 13), (31, 33), (32, 32), (33, 31), (64, 64), (65, 63), (97, 131)]  # (h, w)
SUBSET = [(1, 1), (2, 2), (3, 5), (13, 13), (33, 31), (65, 63)]
OTHER_K = (1, 3, 5, 9, 15)
OTHER_SIGMA = (0.0, 0.5, 1.0, 2.5)
CONTENTS = ("noise", "constant", "checker1", "checker2", "smooth")


def plane(kind, h, w, seed=0):
    rng = np.random.default_rng(9000 + 131 * h + w + seed)
    yy, xx = np.mgrid[:h, :w]
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "constant":
        return np.full((h, w), 255 if seed % 2 == 0 else 93, np.uint8)
    if kind == "checker1":
        return (((xx + yy) & 1) * 255).astype(np.uint8)
    if kind == "checker2":
        return ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)
    if kind == "smooth":
        return np.clip(127.5 + 90 * np.sin(xx / 5.3 + 0.4) * np.cos(yy / 7.1) + 30 * np.sin((xx + 2 * yy) / 11.0), 0, 255).astype(np.uint8)
    raise ValueError(kind)


def bgr(kind, h, w, seed=0):
    """Three different planes of the same kind (a constant image gets three different constants)."""
    if kind == "constant":
        return np.stack([np.full((h, w), v, np.uint8) for v in ((255, 255, 255) if seed % 2 == 0 else (12, 200, 97))], axis=-1)
    return np.stack([plane(kind, h, w, seed + 17 * c) for c in range(3)], axis=-1)


def impulse_positions(h, w):
    """Each corner, each edge midpoint and the centre, without repeats, as (y, x)."""
    ys, xs = sorted({0, h // 2, h - 1}), sorted({0, w // 2, w - 1})
    return [(y, x) for y in ys for x in xs]


def composite_frame():
    """About 420 x 400, BGR: a textured dark quadrilateral of area above 100000 drawn on a brighter textured table, so that
    the chain finds the quadrilateral's outline as one closed edge."""
    h, w = 400, 420
    rng = np.random.default_rng(77)
    f = np.empty((h, w, 3), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    for c in range(3):
        f[..., c] = np.clip(170 + 12 * np.sin(xx / 23.0 + c) + 9 * np.cos(yy / 17.0) + rng.integers(-3, 4, (h, w)), 0, 255)
    quad = [(30, 25), (395, 40), (385, 375), (20, 360)]
    m = convex_mask(h, w, quad)
    for c in range(3):
        f[..., c][m] = np.clip(60 + 10 * c + 8 * np.sin(xx / 9.0)[m] + rng.integers(-3, 4, int(m.sum())), 0, 255)
    return f, quad
