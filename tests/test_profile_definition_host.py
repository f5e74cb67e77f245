"""apply_color_profile beyond the neutral setting, on the CPU oracle, against its definition (tests/ref64.py: the float64
convertScaleAbs, the integer BGR2HSV, the numpy middle of the reference's function as numpy evaluates it, the float64
HSV2BGR).  The kernel, the oracle and the recorded fixtures all come from one restatement of that function; here the
oracle has to land on the one candidate per pixel that the definition leaves (ref64_checks.check_profile), for every profile
of PROFILE_CASES.  test_gpu_ref64.py runs the same checks on the HIP kernels.  The last test uses the reference alone: it
states each convention that a restatement could have misread and shows that the cases tell it from the definition."""
import functools

import numpy as np
import pytest

import ref64 as R
import ref64_checks as K


def test_bgr2hsv_integer_form_whole_cube(oracle):
    """ref64.bgr2hsv_u8 inside check_bgr2hsv's envelope around the float64 definition on all 2^24 colours (reference against
    reference), and the oracle's BGR2HSV equal to it."""
    cube = np.arange(1 << 24, dtype=np.uint32)
    for part in np.array_split(cube, 8):
        img = np.stack([part & 255, (part >> 8) & 255, part >> 16], axis=-1).astype(np.uint8).reshape(-1, 4096, 3)
        hsv = R.bgr2hsv_u8(img)
        K.check_bgr2hsv(hsv, img)
        K.check_exact(oracle.bgr2hsv(img), hsv, "oracle BGR2HSV against the integer form")


@pytest.mark.parametrize("name,offset", K.profile_cube_cases())
def test_oracle_profile_on_cube(oracle, name, offset):
    s = K.check_profile_cube(oracle.apply_color_profile, name, offset)
    print("profile %s cube %d: max %.4f, over 1 LSB %.4f, ties %d" % (name, offset, s["max"], s["over1"], s["ties"]))


@pytest.mark.parametrize("name", list(K.PROFILE_CASES))
def test_oracle_profile_on_small_frames(oracle, name):
    K.check_profile_frames(oracle.apply_color_profile, name)


def test_neg_contrast_byte_map_takes_the_observed_neighbour_at_ties():
    """contrast -0.71, brightness 12.9: levels 40, 140 and 240 are the .5 ties of convertScaleAbs.  profile_byte_map accepts
    either neighbour there and hands it on; one level off a tie by a whole LSB is refused."""
    p = K.PROFILE_CASES["neg_contrast"]
    x = R.convert_scale_abs(np.arange(256), p["contrast"], p["brightness"])
    ties = np.nonzero(np.abs(x - np.floor(x) - 0.5) <= K.csa_eps(p["contrast"], p["brightness"]))[0]
    assert list(ties) == [40, 140, 240]
    for side in (np.floor, np.ceil):
        ramp = K.byte_map_definition(p).copy()
        ramp[ties] = side(x[ties])
        got = K.profile_byte_map(np.repeat(ramp[None, :, None], 3, axis=2), p)
        assert np.array_equal(got, ramp)
    ramp = K.byte_map_definition(p).copy()
    ramp[100] += 1
    with pytest.raises(AssertionError):
        K.profile_byte_map(np.repeat(ramp[None, :, None], 3, axis=2), p)


# ------------------------------------------------------------------ the cases are worth something

# misreading -> (what changes in ref64._profile_adjust, or "noabs" for the byte map; the profiles that carry the line)
MISREADINGS = {
    "rounding instead of truncation": (dict(to_u8=lambda a: np.rint(a).astype(np.uint8)), ("shipped", "radical", "clipping", "val06")),
    "fmod instead of floored mod": (dict(mod=np.fmod), ("shipped", "partial_negative", "stages_fractional")),
    "<= instead of < on the radical window": (dict(less=np.less_equal), ("radical", "radical_wrap", "radical_lilac")),
    "hue distance without the wrap at 180": (dict(wrap=False), ("radical_wrap",)),
    "float64 instead of float32 products": (dict(dtype=np.float64), ("radical",)),
    "no abs in the byte map": ("noabs", ("shipped", "clipping", "stages_fractional")),
}
LEDGER_MIN_PIXELS = 1000


@functools.lru_cache(maxsize=None)
def _cube_hsv_in(name, offset, noabs=False):
    p = K.PROFILE_CASES[name]
    bm = K.byte_map_definition(p)
    if noabs:
        x = np.arange(256, dtype=np.float64) * p.get("contrast", 1.0) + p.get("brightness", 0)
        bm = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    return R.bgr2hsv_u8(bm[K.color_cube(offset)])


def _pixels_put_outside(name, offset, change):
    """Pixels of the cube that an implementation with the one `change` would put outside 0.5 + HSV2BGR_EPS of the definition."""
    p = K.PROFILE_CASES[name]
    base = R.color_profile_adjust(_cube_hsv_in(name, offset), p)
    if change == "noabs":
        other = R.color_profile_adjust(_cube_hsv_in(name, offset, True), p)
    else:
        other = R._profile_adjust(_cube_hsv_in(name, offset), p, **change)
    moved = (base != other).any(axis=-1)                      # HSV2BGR is a function of the triple: only these can differ
    ref = np.clip(R.hsv2bgr(base[moved]), 0, 255)
    out = np.rint(np.clip(R.hsv2bgr(other[moved]), 0, 255))
    return int((np.abs(out - ref) > 0.5 + K.HSV2BGR_EPS).any(axis=-1).sum())


@pytest.mark.parametrize("misreading", list(MISREADINGS))
def test_cases_tell_a_misreading_from_the_definition(misreading):
    change, carriers = MISREADINGS[misreading]
    counts = {(n, o): _pixels_put_outside(n, o, change) for n in carriers for o in K.profile_cube_offsets(n)}
    print(misreading, counts)
    assert set(carriers) <= set(K.PROFILE_CASES)
    assert min(counts.values()) >= LEDGER_MIN_PIXELS, (misreading, counts)      # every carrier on every cube it meets
