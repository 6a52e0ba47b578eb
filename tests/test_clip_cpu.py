"""History clipping without a GPU: the reference (tests/clip_ref.py) against wrong copies of
itself, the premises of tests/test_gpu_clip.py's cases, and what the clip is for.

Teeth, in the style of test_temporal_ref_teeth.py: each of the similarity rule, the n < 4 rule,
the history cap and the moment shift is knocked out of the reference in turn, and the frame in
which the rule first acts moves by at least 100 times the bound the GPU test asserts -- a kernel
without the rule cannot pass the GPU comparison of that case.  The similarity rule, the n < 4 rule
and the moment shift act in frame 2 of a two-frame case.  The cap cannot: frame 2 gathers history
lengths of 1, and the smallest cap is 1.  It is judged on frame 3 of the chain, whose cap is 1 and
whose reprojected pixels gather lengths of 2.

Premises: every clipped case of the GPU test shows reprojected pixels on either side of the clip
(20 each; the 15-pixel frame one each), a pixel with fewer than four similar neighbours, and at
most 1 % of undecidable pixels, with the reference alone.

The lag scenario: a static camera over the synthetic guides, ten noisy frames, a rectangle whose
radiance drops to 0.3 of itself from frame 6 on."""
import numpy as np
import pytest

from tests import clip_cases as K
from tests import clip_ref as CR
from tests import temporal_ref as TR
from tests import test_gpu_clip as GC
from tests import test_gpu_temporal as G

# knock-out -> (the case, the frame judged, 0-based)
TEETH = {"similarity": ("pitch_roll_r3", 1), "n4": ("static_r3", 1), "shift": ("translate_r1", 1), "cap": ("chain", 2)}


def _sequence(case):
    return K.chain() if case == "chain" else K.two_frames(case)


@pytest.mark.parametrize("rule", list(TEETH))
def test_case_exposes_rule(rule):
    case, k = TEETH[rule]
    cams, frames, params, clip, _ = _sequence(case)
    ref = K.reference(cams, frames, params, clip)[k]
    state = K.reference(cams[:k], frames[:k], params, clip)[-1]["state"]
    wrong = TR.temporal_ref(state, cams[k], *frames[k], clip=clip, _without=rule, **params)
    dec = ref["decidable"] & wrong["decidable"]
    delta = max(float(np.abs(ref[f] - wrong[f])[dec].max() / np.abs(ref[f]).max())
                for f in ("out", "variance", "history_len"))
    print(f"{case} frame {k + 1} without {rule}: max|d| / max = {delta:.3g} over colour, variance and history length")
    assert delta >= 100 * GC.BOUND


def test_every_rule_has_a_case():
    assert set(TEETH) == set(CR.KNOCKS)


@pytest.mark.parametrize("name", list(K.TWO_FRAME))
def test_two_frame_premises(name):
    cams, frames, params, clip, _ = K.two_frames(name)
    refs = K.reference(cams, frames, params, clip)
    w, h = K.TWO_FRAME[name][:2]
    assert not refs[0]["reprojected"].any() and not refs[0]["clipped"].any()
    K.premises(name, refs[1], w, h)


def test_chain_premises():
    cams, frames, params, clip, _ = K.chain()
    refs = K.reference(cams, frames, params, clip)
    for k in (1, 2, 3):
        K.premises(f"chain frame {k + 1}", refs[k], G.W, G.H)
    # the cap acts: an unclipped pixel's length goes on growing, a clipped one's is 2
    n = refs[3]["history_len"]
    assert (n[refs[3]["clipped"]] == 2.0).all() and (n == 4.0).any()


def test_motion_case_premises():
    """test_gpu_motion's both_move, as test_gpu_clip.motion_frames builds it."""
    M, cams, vts, frames = GC.motion_frames(True)
    params = dict(K.PARAMS, demodulate=True)
    first = M.MR.temporal_motion_ref(None, cams[0], *frames[0], M.CARRIER, vts[0], clip=K.CLIP, **params)
    second = M.MR.temporal_motion_ref(first["state"], cams[1], *frames[1], M.CARRIER, vts[1], clip=K.CLIP, **params)
    K.premises("both_move", second, G.W, G.H)


def test_deform_case_premises():
    """deform_cases' camera_bulge on feature buffers computed in numpy (the GPU test feeds the GPU's own)."""
    from tests import deform_cases as DC
    from tests import deform_ref as DR
    from tests import deform_scenes as DS
    spec, extra, _ = DC.CASES["camera_bulge"]
    params = dict(DC.PARAMS, **extra, demodulate=True)
    state = None
    for cam, wv, wn, rad, aov, deform in DC.sequence(spec):
        ref = DR.temporal_deform_ref(state, cam, rad, CR.speck(aov), DS.rest()[0], wv, wn, clip=K.CLIP, **params)
        state = ref["state"]
    K.premises("camera_bulge", ref, DC.W, DC.H)


def test_path_case_premises():
    """temporal_path_cases' hall_two on the CPU walk's mirror-path buffers (the GPU test feeds the GPU's own)."""
    from tests import temporal_path_cases as PK
    from tests import temporal_path_ref as TP
    name, w, h, cap, _ = PK.GPU_CASES["hall_two"]
    state = None
    for i, cam in enumerate(PK.case_cameras("hall_two")):
        aov = CR.speck(PK.walk(name, w, h, cap, cam))
        ref = TP.temporal_path_ref(state, cam, PK.radiance(101 + 101 * i, aov), aov, clip=K.CLIP,
                                   point_tol=PK.POINT_TOL, **dict(PK.PARAMS, demodulate=True))
        state = ref["state"]
    assert (aov["bounces"] > 0).sum() >= 100
    K.premises("hall_two", ref, w, h)


def test_loose_box_and_off_are_the_reference():
    """clip None is the entry point's reference itself; a box of 1e30 standard deviations clips nothing."""
    cams, frames, params, clip, _ = K.two_frames("pitch_roll_r3")
    off = K.reference(cams, frames, params, None)[1]
    plain = TR.temporal_ref(TR.temporal_ref(None, cams[0], *frames[0], **params)["state"], cams[1], *frames[1], **params)
    loose = K.reference(cams, frames, params, dict(clip, gamma=1e30))[1]
    for f in ("out", "variance", "history_len"):
        assert np.array_equal(off[f], plain[f])
        assert np.abs(loose[f] - plain[f]).max() <= 1e-12 * np.abs(plain[f]).max()
    assert not loose["clipped"].any() and loose["boxed"].sum() > 900


def test_box_is_exact_on_a_constant_window():
    """Moments about the centre's colour: a constant neighbourhood has sigma exactly 0, lo = hi = c."""
    cam = TR.camera(aspect=G.ASPECT)
    rad, aov = K.frame(cam, 101, G.W, G.H)
    flat = np.full_like(rad, np.float32(0.1) * np.float32(3.0))
    lo, hi, n = CR.box_ref(flat, aov, 3, 1.0, 0.1, 0.9, False)
    boxed = n >= 4
    assert boxed.sum() > 900 and (~boxed).sum() >= 2
    assert np.array_equal(lo[boxed], flat[boxed].astype(np.float64)) and np.array_equal(hi[boxed], lo[boxed])
    assert np.isneginf(lo[~boxed]).all() and np.isposinf(hi[~boxed]).all()


def test_clip_shortens_the_lag():
    """Ten frames from a static camera; the rectangle of rows [8, 16) and columns [10, 22) drops to 0.3 of
    its radiance from frame 6 on.  Two frames later the rectangle's mean absolute error against the
    new level is lower with the clip on than with it off, and outside it the error is no more than
    twice the unclipped one."""
    w, h = G.W, G.H
    cam = TR.camera(aspect=G.ASPECT)
    aov = TR.synthetic_guides(cam, w, h)
    region = np.zeros((h, w), bool)
    region[8:16, 10:22] = True
    assert len(np.unique(aov["material"][region])) == 2     # (it lies across the near strip's edge)
    level = np.where(aov["material"][..., None] >= 0, 1.0, 0.5) * np.ones((h, w, 3))
    rng = np.random.default_rng(7)
    params = dict(K.PARAMS, demodulate=False)
    states, outs = {False: None, True: None}, {}
    for k in range(1, 11):
        now = level * np.where(region[..., None] & (k >= 6), 0.3, 1.0)
        rad = (now * rng.gamma(4.0, 0.25, (h, w, 3))).astype(np.float32)       # relative standard deviation 0.5
        for on in (False, True):
            r = TR.temporal_ref(states[on], cam, rad, aov, clip=K.CLIP if on else None, **params)
            states[on] = r["state"]
            if k == 8:
                truth, outs[on] = now, r["out"]
    err = {on: np.abs(outs[on] - truth) for on in outs}
    inside = {on: float(err[on][region].mean()) for on in err}
    outside = {on: float(err[on][~region].mean()) for on in err}
    print(f"frame 8, mean |out - truth|: rectangle {inside[False]:.4f} off, {inside[True]:.4f} on; "
          f"elsewhere {outside[False]:.4f} off, {outside[True]:.4f} on")
    assert inside[True] < inside[False]
    assert outside[True] <= 2.0 * outside[False]
