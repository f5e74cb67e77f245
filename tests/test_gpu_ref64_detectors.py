"""The detector-side HIP kernels against tests/ref64.py directly: the k = 1..31 GaussianBlur of the squares and of the
pipeline's ChangeDetector stage, cbv_canny, the Canny inside k_hough, and the change statistics of a square.  Every expected
value is computed on the host from the definitions in ref64.py (checkers in ref64_checks.py), never from the oracle;
test_ref64_detectors_host.py runs the same checkers and inputs on the CPU oracle."""
import numpy as np
import pytest

import ref64 as R
import ref64_checks as K

pytestmark = pytest.mark.gpu


def _gray_of(img):
    return R.bgr2gray_q15(img) if img.ndim == 3 else img


# ------------------------------------------------------------------ GaussianBlur k = 1..31 on squares


@pytest.mark.parametrize("k", K.BLUR_KS)
def test_square_blur(gpu_ctx, k):
    """SquareSet.load(squares, k): k_squares_preprocess5 for k = 5, the generic k_squares_preprocess otherwise."""
    from chessboard_vision_amd._squares import GRAY, SquareSet
    sq = K.blur_squares()
    ss = SquareSet(gpu_ctx)
    ss.load(sq, k)
    worst, over1 = 0.0, 0.0
    for key, img in sq.items():
        if img.ndim == 3:
            K.check_gray(_gray_of(img), img)          # the integer gray fed to the blur reference is BT.601 within its bound
        s = K.check_gaussian(ss.get(GRAY, key), _gray_of(img), k)
        worst, over1 = max(worst, s["max"]), max(over1, s["over1"])
    ss.close()
    print("GaussianBlur k=%d: max |out - float64| %.3f, at most %.2f %% of a square over 1 LSB, ||E||_1 %.4f"
          % (k, worst, 100 * over1, K.gaussian_e1(k)))


# ------------------------------------------------------------------ the same blur inside the pipeline


@pytest.mark.parametrize("k", [1, 7, 9, 13, 31])
def test_pipeline_blur_planes_and_histogram(gpu_ctx, k):
    """k_change_blur_stats (calibration mean planes) and k_change_hist on the 640x480 stream with the irregular grid."""
    from chessboard_vision_amd import synth as S
    from chessboard_vision_amd.grid_extractor import SmartGridExtractor
    import change_blur_ref as B
    from test_gpu_change_blur import _pipeline, _positions
    grid = (tuple(S.CALIB_GRID_X), tuple(S.CALIB_GRID_Y))
    p = _pipeline(B.PARAMS_B, k, grid_lines=grid)
    assert p.change_blur == k
    p.run(9, 1)
    ge = SmartGridExtractor()
    ge.grid_lines_x, ge.grid_lines_y = list(grid[0]), list(grid[1])
    sq0, sq9 = ge.split_board(p.download(2, 0)), ge.split_board(p.download(2, 9))
    hist = p.change_hist(0, 9, k)
    positions = _positions(p)
    assert len(positions) == 64 == len(sq0) and len({sq0[pos].shape for pos in positions}) > 1
    moved = 0
    for i, pos in enumerate(positions):
        base, cur = R.gaussian_blur_u8(_gray_of(sq0[pos]), k), R.gaussian_blur_u8(_gray_of(sq9[pos]), k)
        mean, var = p.model(pos)
        assert mean.dtype == np.float32 and np.all(var == np.float32(B.PARAMS_B[1])), (k, pos)
        K.check_gaussian(mean, _gray_of(sq0[pos]), k)
        want = np.bincount(np.abs(cur.astype(np.int64) - base.astype(np.int64)).ravel(), minlength=256)
        assert np.array_equal(hist[i], want), (k, pos)
        moved += int(want[1:].sum())
    assert moved > 0
    p.close()


# ------------------------------------------------------------------ Canny


@pytest.mark.parametrize("h,w,content,t", K.canny_cases(), ids=str)
def test_canny(gpu_ctx, h, w, content, t):
    from chessboard_vision_amd.grid_extractor import canny
    gray = K.canny_input(content, h, w)
    s = K.check_canny(canny(gray, *t), gray, *t, tie_cap=K.canny_tie_cap(content, h, w))
    print("Canny %s %dx%d %s: %d edges, gap %.2f %%" % (content, h, w, t, s["edges"], 100 * s["gap"]))


@pytest.mark.parametrize("end", ["left", "right"])
def test_canny_weak_curve_across_the_tiles(gpu_ctx, end):
    """Tiled hysteresis: a 130 x 197 image, one weak curve through all six 64 x 64 tiles, strong at one end only."""
    from chessboard_vision_amd.grid_extractor import canny
    K.check_hysteresis_curve(canny(K.hysteresis_curve(end), *K.CURVE_THRESHOLDS), end)


def test_canny_magnitude_equal_to_a_threshold(gpu_ctx):
    """M > low and M > high are strict: a step whose magnitude equals the threshold (ref64_checks.threshold_step)."""
    from chessboard_vision_amd.grid_extractor import canny
    K.check_threshold_step(canny)


@pytest.fixture(scope="module")
def hough_squares(oracle):
    from test_gpu_stages import _hough_squares
    return _hough_squares(oracle)       # the oracle only prepares these inputs


@pytest.mark.parametrize("param1", [100, 60])
def test_hough_internal_canny_edge_count(gpu_ctx, hough_squares, param1):
    """cbv_hough_result.n_edges = |hyst(conv)| at (param1 / 2, param1); the edge map itself is not exported."""
    from chessboard_vision_amd._squares import GRAY, SquareSet
    total = 0
    for g0 in range(0, len(hough_squares), 64):
        part = hough_squares[g0:g0 + 64]
        ss = SquareSet(gpu_ctx)
        ss.load({i: g for i, g in enumerate(part)}, 5)
        for i, g in enumerate(part):
            ss.set(GRAY, i, g)
        res = ss.hough(param1=param1)
        for i, g in enumerate(part):
            want = int(R.canny_sets(g, param1 / 2, param1)[2].sum())
            assert res[i].n_edges == want, (g0 + i, g.shape, res[i].n_edges, want)
            total += want
        ss.close()
    print("Hough-internal Canny param1=%d: %d edges over %d squares" % (param1, total, len(hough_squares)))
    assert total > 1000


def test_hough_internal_canny_magnitude_equal_to_low(gpu_ctx):
    """param1 = 80: low = 40 is the magnitude of the weak stretch of threshold_step(), which must stay out of the count."""
    from chessboard_vision_amd._squares import GRAY, SquareSet
    g = K.threshold_step()
    want = int(R.canny_sets(g, 40, 80)[2].sum())
    assert 0 < want < int(R.canny_sets(g, 38, 80)[2].sum())
    ss = SquareSet(gpu_ctx)
    ss.load({0: g}, 5)
    ss.set(GRAY, 0, g)
    assert ss.hough(param1=80)[0].n_edges == want
    ss.close()


# ------------------------------------------------------------------ change statistics of a square


def test_square_change_statistics(gpu_ctx):
    """sad_ref, z_count and z_max of the edge shapes of test_gpu_stages.test_squares_edge_shapes against numpy float32,
    with set reference, mean and variance planes; one square has variance 0 (z = inf where the pixel differs from the mean,
    NaN where it equals it) and one has variance 0 only where the pixel differs (inf, no NaN)."""
    from chessboard_vision_amd._squares import GRAY, MEAN, REF, VAR, SquareSet
    rng = np.random.default_rng(4)
    shapes = [(128, 128, 3), (1, 1), (5, 7, 3), (77, 80), (3, 128, 3), (128, 2)]
    sq = {i: rng.integers(0, 256, size=s, dtype=np.uint8) for i, s in enumerate(shapes)}
    for k, z_thr in ((5, 2.5), (9, 1.45)):
        ss = SquareSet(gpu_ctx)
        ss.load(sq, k)
        ss.calibrate(400.0)
        planes = {}
        for i, img in sq.items():
            g = R.gaussian_blur_u8(_gray_of(img), k)
            assert np.array_equal(ss.get(GRAY, i), g)
            ref = rng.integers(0, 256, g.shape, dtype=np.uint8)
            mean = (g.astype(np.float32) + rng.normal(0, 20, g.shape).astype(np.float32)).astype(np.float32)
            var = rng.uniform(1, 900, g.shape).astype(np.float32)
            if i == 3:                                   # variance 0 everywhere; mean equal to the pixel on half of them
                var[:] = 0
                mean = np.where(rng.random(g.shape) < 0.5, g.astype(np.float32), mean).astype(np.float32)
            if i == 4:                                   # variance 0 only where the pixel differs from the mean
                mean = np.floor(mean)
                var[g.astype(np.float32) != mean] = 0
                var[g.astype(np.float32) == mean] = 25
            planes[i] = (g, ref, mean, var)
            ss.set(REF, i, ref)
            ss.set(MEAN, i, mean)
            ss.set(VAR, i, var)
        st = ss.stats(use_ref=True, use_model=True, z_threshold=z_thr)
        for i, (g, ref, mean, var) in planes.items():
            sad, z_count, z_max = K.change_stats_ref(g, ref, mean, var, z_thr)
            assert st[i].n == g.size and st[i].sad_ref == sad, (k, i)
            assert st[i].z_count == z_count, (k, i, st[i].z_count, z_count)
            got = np.float32(st[i].z_max)
            assert (np.isnan(got) and np.isnan(z_max)) or got == z_max, (k, i, got, z_max)
        assert np.isnan(np.float32(st[3].z_max)) and np.isinf(np.float32(st[4].z_max)) and st[4].z_count > 0
        ss.close()
