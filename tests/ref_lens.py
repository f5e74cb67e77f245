"""The warp through a lens, restated in plain numpy float64 from the definition in include/cbv.h (cbv_lens): the
coordinates, the split, the 15-bit fixed-point blend, border 0 and the rotation by 180 degrees.  Elementwise numpy
arithmetic rounds every operation once and fuses nothing, which is what the definition asks for.  A reference for tests;
it shares no code with the library."""
import numpy as np

# the lenses of the tests: (fx, fy, cx, cy, k1, k2, p1, p2, k3)
BARREL = (200.0, 200.0, 128.0, 96.0, -0.28, 0.09, 0.001, -0.0005, -0.012)
PINCUSHION = (200.0, 200.0, 128.0, 96.0, 0.15, 0.02, -0.001, 0.0007, 0.0)
BARREL_1080P = (1400.0, 1400.0, 960.0, 540.0, -0.28, 0.09, 0.001, -0.0005, -0.012)

I32_MIN, I32_MAX = -2147483648.0, 2147483647.0


def block_width(dw, dh):
    """bw0 of WarpPerspectiveInvoker's blocks (BLOCK_SZ = 32) for a dw x dh destination"""
    bh0 = min(16, dh)
    return min(32 * 32 // bh0, dw)


def invert3x3(M):
    """cv::invert of a 3 x 3 matrix (cofactors times the reciprocal determinant), in Python floats: one rounding per
    operation.  A singular matrix gives zeros."""
    s = [[float(v) for v in row] for row in np.asarray(M, dtype=np.float64).reshape(3, 3)]
    d = (s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0])
         + s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]))
    if d == 0.0:
        return np.zeros((3, 3))
    d = 1.0 / d
    t = [(s[1][1] * s[2][2] - s[1][2] * s[2][1]) * d, (s[0][2] * s[2][1] - s[0][1] * s[2][2]) * d,
         (s[0][1] * s[1][2] - s[0][2] * s[1][1]) * d, (s[1][2] * s[2][0] - s[1][0] * s[2][2]) * d,
         (s[0][0] * s[2][2] - s[0][2] * s[2][0]) * d, (s[0][2] * s[1][0] - s[0][0] * s[1][2]) * d,
         (s[1][0] * s[2][1] - s[1][1] * s[2][0]) * d, (s[0][1] * s[2][0] - s[0][0] * s[2][1]) * d,
         (s[0][0] * s[1][1] - s[0][1] * s[1][0]) * d]
    return np.array(t).reshape(3, 3)


def distort(lens, u, v):
    """the forward model on ideal pixel positions (arrays or scalars)"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = lens
    x = (u - cx) / fx
    y = (v - cy) / fy
    r2 = x * x + y * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xy2 = 2.0 * x * y
    xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x * x)
    yd = y * kr + p1 * (r2 + 2.0 * y * y) + p2 * xy2
    return xd * fx + cx, yd * fy + cy


def undistort(lens, ud, vd, rounds=40):
    """the fixed-point iteration of cv2.undistortPoints with a fixed number of rounds"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = lens
    xd = (np.asarray(ud, dtype=np.float64) - cx) / fx
    yd = (np.asarray(vd, dtype=np.float64) - cy) / fy
    x, y = xd, yd
    for _ in range(rounds):
        r2 = x * x + y * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xy2 = 2.0 * x * y
        tx = p1 * xy2 + p2 * (r2 + 2.0 * x * x)
        ty = p1 * (r2 + 2.0 * y * y) + p2 * xy2
        x, y = (xd - tx) / kr, (yd - ty) / kr
    return x * fx + cx, y * fy + cy


def coords(lens, Minv, dw, dh):
    """X, Y [dh, dw] int64: the rounded 1/32-px source position of every destination pixel.  lens None: the lens-free warp."""
    M = np.asarray(Minv, dtype=np.float64).reshape(9)
    bw0 = block_width(dw, dh)
    dx = np.arange(dw, dtype=np.int64)[None, :]
    dy = np.arange(dh, dtype=np.int64)[:, None].astype(np.float64)
    bx = ((dx // bw0) * bw0).astype(np.float64)
    x1 = dx.astype(np.float64) - bx
    with np.errstate(all="ignore"):
        X0 = M[0] * bx + M[1] * dy + M[2]
        Y0 = M[3] * bx + M[4] * dy + M[5]
        W0 = M[6] * bx + M[7] * dy + M[8]
        W = W0 + M[6] * x1
        if lens is None:
            Wi = np.where(W != 0.0, 32.0 / W, 0.0)
            fX = (X0 + M[0] * x1) * Wi
            fY = (Y0 + M[3] * x1) * Wi
        else:
            Wi = np.where(W != 0.0, 1.0 / W, 0.0)
            u = (X0 + M[0] * x1) * Wi
            v = (Y0 + M[3] * x1) * Wi
            ud, vd = distort(lens, u, v)
            fX = ud * 32.0
            fY = vd * 32.0
            nan = np.isnan(fX) | np.isnan(fY)  # not a number: the lowest int32, far outside
            fX = np.where(nan, I32_MIN, fX)
            fY = np.where(nan, I32_MIN, fY)
        fX = np.clip(fX, I32_MIN, I32_MAX)
        fY = np.clip(fY, I32_MIN, I32_MAX)
    return np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)  # rint: half to even


def blend(frame, X, Y, rot180=False):
    """the taps and the fixed-point blend of a BGR frame [h, w, 3] at the 1/32-px positions X, Y"""
    f = np.asarray(frame)
    h, w = f.shape[:2]
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    wts = [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
    acc = np.zeros(X.shape + (3,), np.int64)
    for (ox, oy), wt in zip(((0, 0), (1, 0), (0, 1), (1, 1)), wts):
        x, y = sx + ox, sy + oy
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        tap = f[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        acc += np.where(inside[..., None], tap, 0) * wt[..., None]  # a tap outside the frame is BGR 0
    out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    return out[::-1, ::-1].copy() if rot180 else out


def warp(frame, lens, M, dw, dh, rot180=False):
    """the bytes of the warp of a BGR frame with matrix M (board <- ideal frame), as cbv_warp_lens takes it"""
    X, Y = coords(lens, invert3x3(M), dw, dh)
    return blend(frame, X, Y, rot180)


def homography(src, dst):
    """getPerspectiveTransform in float64: the 3 x 3 matrix that takes the four src points to the four dst points"""
    A, b = [], []
    for (x, y), (u, v) in zip(np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y])
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y])
        b += [u, v]
    hvec = np.linalg.solve(np.array(A), np.array(b))
    return np.append(hvec, 1.0).reshape(3, 3)
