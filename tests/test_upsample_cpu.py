"""tests/upsample_ref.py, the float64 restatement of tpt_upsample's definition (DESIGN.md section 5
"Guided upsampling"): that it has teeth, and that the synthetic inputs of tests/test_gpu_upsample.py
(tests/upsample_cases.py) meet the premises that file's tolerance rests on.  No GPU."""
import numpy as np
import pytest

from tests import upsample_cases as K
from tests import upsample_ref as R


@pytest.fixture(scope="module")
def refs():
    """Every case's inputs and reference output, without and with demodulation, computed once."""
    out = {}
    for (full, low), cid in zip(K.CASES, K.CASE_IDS):
        rad, gl, g = K.case_inputs(full, low)
        for demod in (False, True):
            det = {}
            frame, fb = R.upsample_ref(rad, gl, g, demodulate=demod, details=det, **K.SIGMA)
            out[cid, demod] = (frame, fb, det["emin"])
    return out


# ---- the footprint ----

def test_footprint_is_the_pixel_centre_map():
    """The integer footprint is floor((x + 0.5) lo / full - 0.5) and its fraction, for every ratio
    of the cases; equal sizes and coinciding centres give a single tap."""
    for (W, _), (wl, _) in K.CASES:
        q, f, two = R.axis_footprint(wl, W)
        for x in range(W):
            s = (x + 0.5) * wl / W - 0.5
            x0 = int(np.floor(s + 1e-12))
            assert q[0, x] == min(max(x0, 0), wl - 1) and q[1, x] == min(max(x0 + 1, 0), wl - 1)
            assert abs(f[x] - (s - x0)) < 1e-9
            assert two[x] == (abs(s - round(s)) > 1e-9)
    q, f, two = R.axis_footprint(37, 37)
    assert (q[0] == np.arange(37)).all() and not two.any() and (f == 0.0).all()
    q, f, two = R.axis_footprint(13, 37 + 2)              # 39 = 3 * 13: the middle pixel of three coincides
    assert [bool(t) for t in two[:3]] == [True, False, True]


# ---- teeth ----

def test_constant_image_is_a_fixed_point(refs):
    for (full, low) in K.CASES:
        _, gl, g = K.case_inputs(full, low)
        const = np.full(low[::-1] + (3,), np.float32(0.7371))
        out, _ = R.upsample_ref(const, gl, g, demodulate=False, **K.SIGMA)
        assert (out == np.float64(np.float32(0.7371))).all()


def test_equal_sizes_give_the_identity():
    rad, gl, g = K.case_inputs((37, 29), (37, 29))
    out, fb = R.upsample_ref(rad, gl, g, demodulate=False, **K.SIGMA)
    assert not fb.any()
    assert np.array_equal(out, rad.astype(np.float64))


def test_material_coded_frame_keeps_the_full_size_edges():
    """A low frame coloured by material id comes out piecewise constant along the full-size
    material edges, wherever a pixel is no fallback pixel."""
    seen = 0
    for (full, low) in K.CASES:
        _, gl, g = K.case_inputs(full, low)
        out, fb = R.upsample_ref(K.material_coded(gl), gl, g, demodulate=False, **K.SIGMA)
        want = K.material_coded(g).astype(np.float64)
        assert np.array_equal(out[~fb], want[~fb]), (full, low)
        seen += int((~fb).sum())
        if fb.any():                                      # a fallback pixel mixes other materials' codes
            assert not np.array_equal(out[fb], want[fb])
    assert seen > 1000


def test_material_rule_has_teeth():
    """Without the material test the same frame bleeds across the material edges."""
    _, gl, g = K.case_inputs((37, 29), (19, 15))
    out, fb = R.upsample_ref(K.material_coded(gl), gl, g, demodulate=False, use_material=False, **K.SIGMA)
    good, fb_good = R.upsample_ref(K.material_coded(gl), gl, g, demodulate=False, **K.SIGMA)
    want = K.material_coded(g).astype(np.float64)
    piecewise_constant = np.array_equal(out[~fb_good], want[~fb_good])
    assert not piecewise_constant                          # the named assertion of the test above fails
    assert not fb.any()                                    # and nothing falls back any more
    assert np.array_equal(good[~fb_good], want[~fb_good])


def _dissimilar():
    """One material everywhere, but the low frame's depth is three times the full frame's: every
    tap has e = 4 / 0.05^2 = 1,600, whose exp is 0 even in float64."""
    gl = {"normal": np.tile(np.float32([0, 0, 1]), (2, 2, 1)), "depth": np.full((2, 2), 3.0, np.float32),
          "material": np.zeros((2, 2), np.int32)}
    g = {"normal": np.tile(np.float32([0, 0, 1]), (4, 4, 1)), "depth": np.full((4, 4), 1.0, np.float32),
         "material": np.zeros((4, 4), np.int32)}
    rad = np.arange(12, dtype=np.float32).reshape(2, 2, 3)
    return rad, gl, g


def test_emin_rule_has_teeth():
    """When every tap is dissimilar the most similar wins; without the subtraction the sum of the
    weights underflows to 0."""
    rad, gl, g = _dissimilar()
    det = {}
    out, fb = R.upsample_ref(rad, gl, g, demodulate=False, details=det, **K.SIGMA)
    all_finite = np.isfinite(out).all()
    assert all_finite and not fb.any()
    assert det["emin"].min() > 1500.0
    assert np.allclose(out, R.bilinear_ref(rad, 4, 4))     # equal e: the weights are the bilinear ones
    bad, _ = R.upsample_ref(rad, gl, g, demodulate=False, use_emin=False, **K.SIGMA)
    all_finite = np.isfinite(bad).all()
    assert not all_finite                                  # the named assertion above fails


def test_black_albedo_does_not_blow_up_in_the_fallback():
    """A black-albedo low pixel next to a bright material: a full-size pixel of a material the low
    frame does not hold falls back to the raw radiance -- demodulating it would divide by 1e-3 and
    multiply by the bright albedo."""
    gl = {"albedo": np.float32([[[0, 0, 0], [0.9, 0.9, 0.9]]]), "normal": np.tile(np.float32([0, 0, 1]), (1, 2, 1)),
          "depth": np.full((1, 2), 2.0, np.float32), "material": np.int32([[0, 1]])}
    g = {"albedo": np.full((1, 4, 3), 0.9, np.float32), "normal": np.tile(np.float32([0, 0, 1]), (1, 4, 1)),
         "depth": np.full((1, 4), 2.0, np.float32), "material": np.int32([[0, 2, 2, 1]])}
    rad = np.float32([[[0.5, 0.5, 0.5], [1.0, 1.0, 1.0]]])
    out, fb = R.upsample_ref(rad, gl, g, demodulate=True, **K.SIGMA)
    assert fb.tolist() == [[False, True, True, False]]
    assert out[fb].max() <= 1.0 and out[fb].min() >= 0.5   # within the raw radiance's range
    assert np.allclose(out[0, 1], 0.5 + 0.25 * 0.5) and np.allclose(out[0, 2], 0.5 + 0.75 * 0.5)
    assert np.allclose(out[0, 0], 0.5 / 1e-3 * 0.9)        # an accepted black tap is demodulated, as defined
    plain, _ = R.upsample_ref(rad, gl, g, demodulate=False, **K.SIGMA)
    assert np.array_equal(plain[fb], out[fb])              # the fallback ignores the flag


# ---- the premises of the GPU inputs ----

def test_every_case_is_finite(refs):
    for key, (frame, fb, emin) in refs.items():
        assert np.isfinite(frame).all(), key
        assert np.abs(frame).max() > 0.0


def test_fallback_premises(refs):
    with_fallback = 0
    for (cid, demod), (frame, fb, emin) in refs.items():
        if demod:
            continue
        print(f"{cid}: fallback {int(fb.sum())} of {fb.size}, largest e_min {emin.max():.1f}")
        assert 2 * int(fb.sum()) <= fb.size, cid           # no case more than half in fallback
        with_fallback += bool(fb.any())
    assert with_fallback >= 3


def test_largest_emin_is_at_most_1000(refs):
    """The allowance of tests/test_gpu_upsample.py, 1e-3, is a few float32 ulp of e times 1,000."""
    worst = max(float(emin.max()) for _, _, emin in refs.values())
    print(f"largest e_min over all cases: {worst:.1f}")
    assert 0.0 < worst <= 1000.0
