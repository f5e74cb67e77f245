"""Plain float64 restatements of the pixel operations the reference calls, written from the operations' definitions.

This module is the second opinion next to oracle/cbv_oracle.c.  It does not import the oracle, does not follow its
rounding order and does not use its tables: every function computes what the operation *is* (OpenCV's documented
formula and conventions) in numpy float64.  Where a stage is continuous the function returns the unrounded float64
result, so a checker can tell a rounding tie from an error; where the operation itself is defined on integers
(CLAHE's LUTs, the 15-bit gray form, the 8.8 Gaussian) the integer result is available too.

Images are numpy arrays: uint8 HxWx3 in BGR channel order, or HxW for one channel.
"""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------
# borders
# ---------------------------------------------------------------------------------------------------------------


def reflect101_index(p, n):
    """cv::BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba): the edge sample is not repeated.  Periodic with period
    2(n-1); a length-1 axis maps everything to 0."""
    p = np.asarray(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    q = np.mod(p, period)
    return np.where(q > n - 1, period - q, q)


def _pad101(img, ry, rx):
    h, w = img.shape[:2]
    yi = reflect101_index(np.arange(-ry, h + ry), h)
    xi = reflect101_index(np.arange(-rx, w + rx), w)
    return img[yi][:, xi]


# ---------------------------------------------------------------------------------------------------------------
# point operations
# ---------------------------------------------------------------------------------------------------------------


def convert_scale_abs(img, alpha, beta):
    """cv2.convertScaleAbs: |alpha * x + beta|, before rounding and saturation to u8."""
    return np.abs(np.asarray(img, np.float64) * alpha + beta)


def bgr2hsv(img):
    """cv2.COLOR_BGR2HSV, 8-bit: V = max(R,G,B); S = 255 (V - min) / V (0 when V = 0); H in degrees is
    60 (G-B)/diff if V == R, else 120 + 60 (B-R)/diff if V == G, else 240 + 60 (R-G)/diff (0 when diff = 0),
    +360 when negative, and is stored halved so it lies in [0, 180).  Unrounded; H is circular (180 == 0)."""
    f = np.asarray(img, np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    v = f.max(axis=-1)
    diff = v - f.min(axis=-1)
    s = np.where(v > 0, 255.0 * diff / np.where(v > 0, v, 1), 0.0)
    dd = np.where(diff > 0, diff, 1)
    h = np.where(v == r, 60.0 * (g - b) / dd, np.where(v == g, 120.0 + 60.0 * (b - r) / dd, 240.0 + 60.0 * (r - g) / dd))
    h = np.where(diff > 0, h, 0.0)
    h = np.where(h < 0, h + 360.0, h)
    return np.stack([h / 2.0, s, v], axis=-1)


def hsv2bgr(hsv):
    """cv2.COLOR_HSV2BGR, 8-bit: H is in half degrees (H * 2 taken modulo 360), S and V scaled by 1/255; the six-sector
    formula p = V(1-S), q = V(1-S f), t = V(1-S(1-f)).  Returns B, G, R times 255, unrounded."""
    a = np.asarray(hsv, np.float64)
    hh = np.mod(a[..., 0] * 2.0, 360.0) / 60.0
    s, v = a[..., 1] / 255.0, a[..., 2] / 255.0
    sec = np.floor(hh)
    f = hh - sec
    sec = sec.astype(np.int64) % 6
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    r = np.choose(sec, [v, q, p, p, t, v])
    g = np.choose(sec, [t, v, v, q, p, p])
    b = np.choose(sec, [p, p, t, v, v, q])
    return np.stack([b, g, r], axis=-1) * 255.0


def bgr2hsv_u8(img):
    """The 8-bit integer form of COLOR_BGR2HSV: 12-bit reciprocal tables sdiv[v] = rint((255 << 12) / v) and
    hdiv[d] = rint((180 << 12) / (6 d)) (0 at index 0); V = max; S = (diff sdiv[V] + 2048) >> 12; H from G - B if V == R,
    else B - R + 2 diff if V == G, else R - G + 4 diff, then (H hdiv[diff] + 2048) >> 12, + 180 when negative.  Returns
    uint8 H, S, V (H may be 180: the form does not fold it to 0)."""
    i = np.asarray(img, np.int64)
    b, g, r = i[..., 0], i[..., 1], i[..., 2]
    n = np.arange(1, 256, dtype=np.float64)
    sdiv = np.zeros(256, np.int64)
    hdiv = np.zeros(256, np.int64)
    sdiv[1:] = np.rint((255 << 12) / n)
    hdiv[1:] = np.rint((180 << 12) / (6.0 * n))
    v = i.max(axis=-1)
    diff = v - i.min(axis=-1)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


PROFILE_DEFAULTS = {"hue_shift": 0, "sat_scale": 1.0, "val_scale": 1.0, "contrast": 1.0, "brightness": 0, "radical_mode": 0,
                    "target_hue": 0, "hue_window": 20}


def _profile_adjust(hsv_u8, profile, dtype=np.float32, mod=np.mod, less=np.less, wrap=True, to_u8=lambda a: a.astype(np.uint8)):
    """color_profile_adjust with each convention as a parameter, so that a test can state one misreading at a time and show
    that its cases tell it from the definition.  The defaults are the definition."""
    p = dict(PROFILE_DEFAULTS, **profile)
    k = dtype                                              # a Python scalar next to a float32 array enters as float32
    hsv = np.asarray(hsv_u8).astype(dtype)
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    if p["radical_mode"]:
        h_dist = np.abs(h - k(p["target_hue"]))
        if wrap:
            h_dist = np.minimum(h_dist, k(180) - h_dist)
        mask = less(h_dist, k(p["hue_window"]))
        s = np.where(mask, s * k(2.0), s * k(0.5))
    h = mod(h + k(p["hue_shift"]), k(180))
    s = s * k(p["sat_scale"])
    v = v * k(p["val_scale"])
    h = np.clip(h, 0, 179)
    s = np.clip(s, 0, 255)
    v = np.clip(v, 0, 255)
    out = np.stack([h, s, v], axis=-1)
    assert out.dtype == dtype
    return to_u8(out)


def color_profile_adjust(hsv_u8, profile):
    """The numpy middle of the reference's apply_color_profile, between its BGR2HSV and its HSV2BGR, as numpy evaluates it:
    the 8-bit H, S, V as float32 arrays, every profile value a float32; in radical mode the hue distance
    min(|h - target|, 180 - |h - target|), strictly below hue_window, selects s * 2.0, the rest s * 0.5;
    h = np.mod(h + hue_shift, 180) (floored: the sign of 180); s *= sat_scale; v *= val_scale; clips to [0, 179], [0, 255],
    [0, 255]; astype(uint8), which truncates.  `profile`: a dict with the keys of color_profile.json, missing keys at the
    reference's defaults (hue_window 20).  Returns uint8 H, S, V."""
    return _profile_adjust(hsv_u8, profile)


# OpenCV's documented RGB -> XYZ matrix (Rec. 709 primaries) and D65 white point (cvtColor docs, "RGB <-> CIE L*a*b*")
RGB2XYZ = np.array([[0.412453, 0.357580, 0.180423],
                    [0.212671, 0.715160, 0.072169],
                    [0.019334, 0.119193, 0.950227]])
D65 = np.array([0.950456, 1.0, 1.088754])
_LAB_T = 0.008856


def _srgb_to_linear(c):
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def _linear_to_srgb(c):
    return np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 0.0), 1 / 2.4) - 0.055)


def bgr2lab(img):
    """cv2.COLOR_BGR2LAB, 8-bit (sRGB input): sRGB piecewise gamma (c/12.92 up to 0.04045, ((c+0.055)/1.055)^2.4
    above); XYZ = RGB2XYZ . rgb; X /= Xn, Z /= Zn with the D65 white; f(t) = t^(1/3) above 0.008856 and
    7.787 t + 16/116 below; L = 116 Y^(1/3) - 16 (903.3 Y at or below 0.008856), a = 500 (f(X) - f(Y)),
    b = 200 (f(Y) - f(Z)); stored as L * 255/100, a + 128, b + 128.  Unrounded."""
    f = np.asarray(img, np.float64) / 255.0
    lin = _srgb_to_linear(f[..., ::-1])                   # BGR -> RGB
    xyz = lin @ RGB2XYZ.T / D65
    ft = np.where(xyz > _LAB_T, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    y = xyz[..., 1]
    L = np.where(y > _LAB_T, 116.0 * np.cbrt(y) - 16.0, 903.3 * y)
    a = 500.0 * (ft[..., 0] - ft[..., 1])
    b = 200.0 * (ft[..., 1] - ft[..., 2])
    return np.stack([L * 255.0 / 100.0, a + 128.0, b + 128.0], axis=-1)


def lab2bgr(lab):
    """cv2.COLOR_LAB2BGR, 8-bit: the inverse of bgr2lab.  L = L8 * 100/255, a = a8 - 128, b = b8 - 128;
    Y = ((L+16)/116)^3 above L = 903.3 * 0.008856 and L/903.3 below; f(X) = f(Y) + a/500, f(Z) = f(Y) - b/200,
    each inverted through the same cube / linear pieces; times the D65 white; rgb = RGB2XYZ^-1 . XYZ clipped to
    [0, 1]; inverse sRGB gamma; times 255.  Returns B, G, R unrounded."""
    a = np.asarray(lab, np.float64)
    L, A, B = a[..., 0] * 100.0 / 255.0, a[..., 1] - 128.0, a[..., 2] - 128.0
    lin_part = L <= 903.3 * _LAB_T
    y = np.where(lin_part, L / 903.3, ((L + 16.0) / 116.0) ** 3)
    fy = np.where(lin_part, 7.787 * y + 16.0 / 116.0, (L + 16.0) / 116.0)
    fx, fz = fy + A / 500.0, fy - B / 200.0
    ft_t = np.cbrt(_LAB_T)

    def finv(ft):
        return np.where(ft > ft_t, ft ** 3, (ft - 16.0 / 116.0) / 7.787)

    xyz = np.stack([finv(fx), y, finv(fz)], axis=-1) * D65
    rgb = np.clip(xyz @ np.linalg.inv(RGB2XYZ).T, 0.0, 1.0)
    return _linear_to_srgb(rgb)[..., ::-1] * 255.0


def bgr2gray(img):
    """cv2.COLOR_BGR2GRAY: Y = 0.299 R + 0.587 G + 0.114 B (BT.601), unrounded."""
    f = np.asarray(img, np.float64)
    return 0.299 * f[..., 2] + 0.587 * f[..., 1] + 0.114 * f[..., 0]


def gray_q15_coefficients():
    """The integer form of BGR2GRAY on 8-bit images: each BT.601 weight rounded to 15 fractional bits, the blue one
    then adjusted so the three sum to exactly 2^15 (white stays 255).  Returned as (cb, cg, cr)."""
    cr, cg, cb = (int(round(c * (1 << 15))) for c in (0.299, 0.587, 0.114))
    cb += (1 << 15) - (cr + cg + cb)
    return cb, cg, cr


def bgr2gray_q15(img):
    """Integer BGR2GRAY: (cb B + cg G + cr R + 2^14) >> 15 with gray_q15_coefficients()."""
    cb, cg, cr = gray_q15_coefficients()
    i = np.asarray(img, np.int64)
    return ((cb * i[..., 0] + cg * i[..., 1] + cr * i[..., 2] + (1 << 14)) >> 15).astype(np.uint8)


def normalize_minmax(img):
    """cv2.normalize(src, None, 0, 255, NORM_MINMAX): one min and one max over the whole array, every channel
    together; out = (x - min) * 255 / (max - min).  A flat image (max == min) gives all 0.  Unrounded."""
    f = np.asarray(img, np.float64)
    lo, hi = f.min(), f.max()
    if hi - lo <= 0:
        return np.zeros_like(f)
    return (f - lo) * (255.0 / (hi - lo))


# ---------------------------------------------------------------------------------------------------------------
# neighbourhood operations
# ---------------------------------------------------------------------------------------------------------------


def filter2d_3x3(img, kernel):
    """cv2.filter2D(src, -1, kernel) with a 3x3 kernel: correlation (no flip), anchor at the centre, BORDER_REFLECT_101,
    per channel: out(y, x) = sum_ij k[i, j] * src(y + i - 1, x + j - 1).  Unrounded and unsaturated."""
    f = np.asarray(img, np.float64)
    k = np.asarray(kernel, np.float64).reshape(3, 3)
    h, w = f.shape[:2]
    p = _pad101(f, 1, 1)
    out = np.zeros_like(f)
    for i in range(3):
        for j in range(3):
            if k[i, j] != 0:
                out += k[i, j] * p[i:i + h, j:j + w]
    return out


def gaussian_kernel(k, sigma=0.0):
    """cv2.getGaussianKernel(k, sigma) for odd k.  sigma <= 0: the fixed tables [1], [1 2 1]/4, [1 4 6 4 1]/16 and
    [1 3.5 7 9 7 3.5 1]/32 for k = 1, 3, 5, 7; otherwise exp(-x^2 / (2 s^2)) at x = i - (k-1)/2 with
    s = 0.3 ((k-1)/2 - 1) + 0.8, normalised to sum 1.  sigma > 0: exp(-x^2 / (2 sigma^2)) normalised, for every k (the
    fixed tables do not apply, k = 7 included)."""
    assert k % 2 == 1 and k >= 1, k
    if sigma <= 0:
        small = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
                 7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
        if k in small:
            return np.array(small[k], np.float64)
        sigma = 0.3 * ((k - 1) / 2.0 - 1.0) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    c = np.exp(-x * x / (2.0 * sigma * sigma))
    return c / c.sum()


def gaussian_q8(k, sigma=0.0):
    """The 8-bit GaussianBlur's kernel in 8 fractional bits: from the edge towards the centre
    q_i = floor(256 c_i + err + 0.5), err carrying the remainder on to the next coefficient (error diffusion); the
    other half mirrors it and the centre is 256 - 2 * sum, so the kernel sums to exactly 256."""
    c = gaussian_kernel(k, sigma)
    q = np.zeros(k, np.int64)
    err = 0.0
    for i in range(k // 2):
        adj = 256.0 * c[i] + err
        q[i] = q[k - 1 - i] = int(np.floor(adj + 0.5))
        err = adj - q[i]
    q[k // 2] = 256 - q.sum()
    return q


def _separable101(a, kern):
    """sum_y sum_x kern[y] kern[x] a(.), BORDER_REFLECT_101 on the array alone, in a's dtype: rows first, no rounding
    in between."""
    h, w = a.shape
    r = len(kern) // 2
    p = _pad101(a, r, r)
    tmp = sum(kern[j] * p[:, j:j + w] for j in range(len(kern)))
    return sum(kern[i] * tmp[i:i + h] for i in range(len(kern)))


def gaussian_blur(gray, k, sigma=0.0):
    """cv2.GaussianBlur(src, (k, k), sigma): gaussian_kernel(k, sigma) applied separably with BORDER_REFLECT_101
    (reflection is repeated where the radius exceeds the array).  Unrounded float64."""
    return _separable101(np.asarray(gray, np.float64), gaussian_kernel(k, sigma))


def gaussian_blur_u8(gray, k, sigma=0.0):
    """The 8-bit GaussianBlur result in integers: min((sum_y sum_x q_y q_x g + 2^15) >> 16, 255) with
    q = gaussian_q8(k, sigma); one rounding (halves upward), none between the two passes."""
    acc = _separable101(np.asarray(gray, np.int64), gaussian_q8(k, sigma))
    return np.minimum((acc + (1 << 15)) >> 16, 255).astype(np.uint8)


def gaussian_q8_envelope(k, sigma=0.0, value_range=255.0):
    """Bound on |gaussian_blur_u8 - gaussian_blur|: 0.5 for the one rounding, plus ||E||_1 * range / 2 with
    E = q (x) q / 65536 - c (x) c (E sums to 0, so only the spread of the window's values around their mid-range counts)."""
    q = gaussian_q8(k, sigma).astype(np.float64)
    c = gaussian_kernel(k, sigma)
    return 0.5 + np.abs(np.outer(q, q) / 65536.0 - np.outer(c, c)).sum() * value_range / 2.0


def dilate_rect(a, r):
    """cv2.dilate(a, ones((2r+1, 2r+1))): the maximum over the (2r+1)^2 window centred on each pixel; pixels outside the
    image do not take part (the default border value never wins a maximum)."""
    a = np.asarray(a)
    h, w = a.shape
    p = np.full((h + 2 * r, w + 2 * r), -1, np.int64)     # -1 outside: below every pixel, and the centre always takes part
    p[r:r + h, r:r + w] = a
    out = p[r:r + h, r:r + w].copy()
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            np.maximum(out, p[i:i + h, j:j + w], out=out)
    return out.astype(a.dtype)


def dilate_5x5_iter3(a):
    """cv2.dilate(a, ones((5, 5)), iterations=3), literally: three passes of the 5 x 5 form."""
    for _ in range(3):
        a = dilate_rect(a, 2)
    return a


def gaussian_blur_5x5(gray):
    """cv2.GaussianBlur(src, (5, 5), 0): sigma 0 with ksize 5 selects the fixed binomial kernel [1 4 6 4 1] / 16,
    applied separably with BORDER_REFLECT_101.  Unrounded (a multiple of 1/256)."""
    return gaussian_blur(gray, 5)


def gaussian_blur_5x5_u8(gray):
    """The 8-bit GaussianBlur result: the kernel is exact in 8 fractional bits, so the 8-bit path rounds the exact
    sum once, halves upward (fixed-point +0.5 then shift)."""
    return gaussian_blur_u8(gray, 5)


def otsu_threshold(hist):
    """cv2.threshold(THRESH_OTSU) on a 256-bin histogram: the t maximising the between-class variance
    w0 w1 (mu0 - mu1)^2 of the classes [0, t] and [t+1, 255] (0 where a class is empty); the first t on a tie.
    Returns (t, variance per t)."""
    hst = np.asarray(hist, np.float64)
    n = hst.sum()
    p = hst / n
    i = np.arange(256, dtype=np.float64)
    w0 = np.cumsum(p)
    m0 = np.cumsum(i * p)
    mt = m0[-1]
    w1 = 1.0 - w0
    ok = (w0 > 0) & (w1 > 1e-15)
    var = np.zeros(256)
    var[ok] = (mt * w0[ok] - m0[ok]) ** 2 / (w0[ok] * w1[ok])
    return int(np.argmax(var)), var


def bilateral_radius(d, sigma_space):
    """Neighbourhood radius of cv2.bilateralFilter: d/2 for d > 0, else round(1.5 sigma_space); at least 1."""
    if sigma_space <= 0:
        sigma_space = 1.0
    r = d // 2 if d > 0 else int(np.floor(sigma_space * 1.5 + 0.5))
    return max(r, 1)


def bilateral_taps(d, sigma_space):
    """Offsets (dy, dx) of the disc i^2 + j^2 <= r^2 that cv2.bilateralFilter sums over."""
    r = bilateral_radius(d, sigma_space)
    return [(i, j) for i in range(-r, r + 1) for j in range(-r, r + 1) if i * i + j * j <= r * r]


def bilateral(img, d=9, sigma_color=75.0, sigma_space=75.0):
    """cv2.bilateralFilter on 8UC3: taps on the disc of bilateral_radius(d, sigma_space) (non-positive sigmas become
    1); weight exp(-(i^2+j^2) / 2 sigma_space^2) * exp(-(|dB|+|dG|+|dR|)^2 / 2 sigma_color^2) with the L1 colour
    distance to the centre pixel; BORDER_REFLECT_101; out = sum(w I) / sum(w) per channel.  Unrounded."""
    sc = sigma_color if sigma_color > 0 else 1.0
    ss = sigma_space if sigma_space > 0 else 1.0
    r = bilateral_radius(d, sigma_space)
    f = np.asarray(img, np.float64)
    h, w = f.shape[:2]
    p = _pad101(f, r, r)
    num = np.zeros_like(f)
    den = np.zeros((h, w))
    for i, j in bilateral_taps(d, sigma_space):
        q = p[r + i:r + i + h, r + j:r + j + w]
        dist = np.abs(q - f).sum(axis=-1)
        wt = np.exp(-(i * i + j * j) / (2 * ss * ss)) * np.exp(-dist * dist / (2 * sc * sc))
        num += wt[..., None] * q
        den += wt
    return num / den[..., None]


def clahe_tiling(h, w, tiles):
    """(tile_h, tile_w, padded_h, padded_w) of cv2.CLAHE with tileGridSize = tiles = (tiles_x, tiles_y): when the
    image does not divide into the grid in *both* directions it is padded (BORDER_REFLECT_101, bottom and right) by
    tiles - (size % tiles) in each direction (a whole extra tile row/column where that axis did divide)."""
    tx, ty = tiles
    if w % tx == 0 and h % ty == 0:
        return h // ty, w // tx, h, w
    eh, ew = h + ty - h % ty, w + tx - w % tx
    return eh // ty, ew // tx, eh, ew


def clahe_clip(clip_limit, area):
    """Per-bin clip count: max(int(clip_limit * area / 256), 1) when clip_limit > 0; 0 (no clipping) otherwise."""
    return max(int(clip_limit * area / 256), 1) if clip_limit > 0 else 0


def clahe_luts(gray, clip_limit=3.0, tiles=(8, 8)):
    """The per-tile lookup tables of cv2.CLAHE: 256-bin histogram of each tile of the REFLECT_101-padded image; bins
    above the clip count are cut and the excess redistributed, batch = excess // 256 to every bin, then the residual
    one count each to bins 0, step, 2 step, ... with step = max(256 // residual, 1); LUT = sat(round(cumsum * scale))
    with scale = 255 / area held as a float32 and the product taken in float32 (which decides exact .5 ties),
    rounded half to even.  Returns (tiles_y * tiles_x, 256) uint8 in row-major tile order."""
    g = np.asarray(gray)
    h, w = g.shape
    tx, ty = tiles
    th, tw, eh, ew = clahe_tiling(h, w, tiles)
    yi = reflect101_index(np.arange(eh), h)
    xi = reflect101_index(np.arange(ew), w)
    ext = g[yi][:, xi]
    area = th * tw
    clip = clahe_clip(clip_limit, area)
    scale = np.float32(255.0 / area)
    luts = np.empty((ty * tx, 256), np.uint8)
    for y in range(ty):
        for x in range(tx):
            hist = np.bincount(ext[y * th:(y + 1) * th, x * tw:(x + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip > 0:
                excess = int(np.maximum(hist - clip, 0).sum())
                hist = np.minimum(hist, clip)
                batch, residual = divmod(excess, 256)
                hist += batch
                if residual:
                    step = max(256 // residual, 1)
                    idx = np.arange(0, 256, step)[:residual]
                    hist[idx] += 1
            cs = np.cumsum(hist)
            luts[y * tx + x] = np.clip(np.rint(cs.astype(np.float32) * scale), 0, 255).astype(np.uint8)
    return luts


def clahe(gray, clip_limit=3.0, tiles=(8, 8), luts=None):
    """cv2.CLAHE.apply on 8-bit gray: each pixel's value v is looked up in the four nearest tile LUTs and blended
    bilinearly at tile coordinates (x / tile_w - 0.5, y / tile_h - 0.5), the neighbour indices clamped to the grid.
    Unrounded."""
    g = np.asarray(gray)
    h, w = g.shape
    tx, ty = tiles
    th, tw, _, _ = clahe_tiling(h, w, tiles)
    if luts is None:
        luts = clahe_luts(g, clip_limit, tiles)
    L = luts.astype(np.float64).reshape(ty, tx, 256)

    def axis(n, t, nt):
        c = np.arange(n) / t - 0.5
        i1 = np.floor(c).astype(np.int64)
        frac = c - i1
        return np.clip(i1, 0, nt - 1), np.clip(i1 + 1, 0, nt - 1), frac

    y1, y2, fy = axis(h, th, ty)
    x1, x2, fx = axis(w, tw, tx)
    v = g.astype(np.int64)
    Y1, Y2, X1, X2 = y1[:, None], y2[:, None], x1[None, :], x2[None, :]
    FX, FY = fx[None, :], fy[:, None]
    top = L[Y1, X1, v] * (1 - FX) + L[Y1, X2, v] * FX
    bot = L[Y2, X1, v] * (1 - FX) + L[Y2, X2, v] * FX
    return top * (1 - FY) + bot * FY


def perspective_source_coords(M, dsize):
    """Source coordinates of every destination pixel of cv2.warpPerspective(src, M, dsize): (X, Y) = the projective
    map of (x, y) through M^-1 (M maps source to destination), in float64.  W == 0 maps to (0, 0)."""
    dw, dh = dsize
    Mi = np.linalg.inv(np.asarray(M, np.float64))
    yy, xx = np.mgrid[:dh, :dw].astype(np.float64)
    W = Mi[2, 0] * xx + Mi[2, 1] * yy + Mi[2, 2]
    Wi = np.where(W != 0, 1.0 / np.where(W != 0, W, 1.0), 0.0)
    X = (Mi[0, 0] * xx + Mi[0, 1] * yy + Mi[0, 2]) * Wi
    Y = (Mi[1, 0] * xx + Mi[1, 1] * yy + Mi[1, 2]) * Wi
    return X, Y


def warp_perspective(img, M, dsize):
    """cv2.warpPerspective(src, M, dsize) with INTER_LINEAR and BORDER_CONSTANT 0: bilinear interpolation at the exact
    float64 source point, samples outside the image counting as 0.  Returns (out unrounded, X, Y)."""
    f = np.asarray(img, np.float64)
    h, w = f.shape[:2]
    X, Y = perspective_source_coords(M, dsize)
    Xc = np.clip(X, -2.0, w + 1.0)          # beyond one pixel outside every tap is 0 anyway
    Yc = np.clip(Y, -2.0, h + 1.0)
    x0, y0 = np.floor(Xc).astype(np.int64), np.floor(Yc).astype(np.int64)
    ax, ay = (Xc - x0)[..., None], (Yc - y0)[..., None]

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        v = f[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(inside[..., None], v, 0.0)

    out = (tap(y0, x0) * (1 - ax) * (1 - ay) + tap(y0, x0 + 1) * ax * (1 - ay)
           + tap(y0 + 1, x0) * (1 - ax) * ay + tap(y0 + 1, x0 + 1) * ax * ay)
    return out, X, Y


# ---------------------------------------------------------------------------------------------------------------
# Canny
# ---------------------------------------------------------------------------------------------------------------


def sobel3(gray):
    """cv2.Sobel(gray, CV_16S, 1, 0 / 0, 1, ksize=3) with BORDER_REPLICATE, as cv2.Canny takes its gradients:
    dx = [1 2 1]^T (x) [-1 0 1], dy = [-1 0 1]^T (x) [1 2 1].  Returns integer (dx, dy)."""
    g = np.asarray(gray, np.int64)
    h, w = g.shape
    p = g[np.clip(np.arange(-1, h + 1), 0, h - 1)][:, np.clip(np.arange(-1, w + 1), 0, w - 1)]
    dx = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    dy = (p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    return dx, dy


def canny_sector(dx, dy):
    """0 horizontal, 1 vertical, 2 diagonal: the sector of the real gradient angle atan2(|dy|, |dx|), below 22.5 degrees,
    above 67.5 degrees, or between.  (No integer pair lies on a boundary: tan 22.5 degrees is irrational, and the nearest
    ratio of Sobel outputs is 3.6e-7 away.)"""
    ang = np.degrees(np.arctan2(np.abs(dy).astype(np.float64), np.abs(dx).astype(np.float64)))
    return np.where(ang < 22.5, 0, np.where(ang > 67.5, 1, 2))


def hysteresis(cand, strong):
    """The pixels of `cand` 8-connected, through cand, to a pixel of cand & strong: 3x3 growth restricted to cand,
    iterated until nothing changes."""
    h, w = cand.shape
    cur = cand & strong
    while True:
        p = np.zeros((h + 2, w + 2), bool)
        p[1:-1, 1:-1] = cur
        grown = cur.copy()
        for i in range(3):
            for j in range(3):
                grown |= p[i:i + h, j:j + w]
        grown &= cand
        if np.array_equal(grown, cur):
            return cur
        cur = grown


def canny_candidates(gray, t1, t2):
    """(M, low, high, strict, loose, conv) of cv2.Canny(gray, t1, t2) (aperture 3, L1 gradient): low, high =
    sorted((floor(t1), floor(t2))); M = |dx| + |dy|; the two neighbours of a pixel lie along its gradient's sector
    (left / right, up / down, or the diagonal chosen by the sign of dx * dy: along (+1, +1) when positive, (+1, -1) when
    negative), neighbours outside the image counting as 0.  A candidate has M > low and M above both neighbours:
    strictly (`strict`), or at least equal (`loose`), or by OpenCV's tie rule (`conv`): > towards left / up,
    >= towards right / down, > on both diagonal neighbours."""
    low, high = sorted((int(np.floor(t1)), int(np.floor(t2))))
    dx, dy = sobel3(gray)
    M = np.abs(dx) + np.abs(dy)
    h, w = M.shape
    p = np.zeros((h + 2, w + 2), np.int64)
    p[1:-1, 1:-1] = M

    def nb(oy, ox):
        return p[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]

    sec = canny_sector(dx, dy)
    pos = dx * dy > 0
    a = np.where(sec == 0, nb(0, -1), np.where(sec == 1, nb(-1, 0), np.where(pos, nb(-1, -1), nb(-1, 1))))
    b = np.where(sec == 0, nb(0, 1), np.where(sec == 1, nb(1, 0), np.where(pos, nb(1, 1), nb(1, -1))))
    over = M > low
    strict = over & (M > a) & (M > b)
    loose = over & (M >= a) & (M >= b)
    conv = over & (M > a) & np.where(sec == 2, M > b, M >= b)
    return M, low, high, strict, loose, conv


def canny_sets(gray, t1, t2):
    """(hyst(strict), hyst(loose), hyst(conv)) as boolean maps, hyst(S) = the pixels of S 8-connected through S to a pixel
    of S with M > high.  Whatever tie rule an implementation of Canny uses, its edges lie between the first two;
    cv2.Canny's are the third."""
    M, _, high, strict, loose, conv = canny_candidates(gray, t1, t2)
    strong = M > high
    return hysteresis(strict, strong), hysteresis(loose, strong), hysteresis(conv, strong)
