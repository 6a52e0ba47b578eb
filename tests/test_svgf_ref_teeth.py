"""The inputs of tests/test_gpu_svgf.py have teeth: for each rule of tpt_denoise_svgf's
definition (DESIGN.md section 5 "Post-pass") the 37 x 29 frame's colour moves by at
least 100 times the GPU test's bound when that rule is knocked out of the float64
reference.  A kernel without the rule then cannot pass the GPU comparison.  CPU only:
the reference against a wrong copy of itself.

Also here: the frame test_gpu_svgf.synthetic restates is test_gpu_denoise.synthetic's,
bit for bit, and its two new planes are what the GPU tests take them to be."""
import numpy as np
import pytest

from tests import svgf_ref as SR
from tests import test_gpu_denoise as D
from tests import test_gpu_svgf as G

ITERATIONS = 3


def knocked_out(rule, demodulate):
    rad, aov, var, hist = G.synthetic()
    kw = dict(G.SIG, iterations=ITERATIONS, demodulate=demodulate)
    wrong = SR.svgf_ref(rad, aov["albedo"], aov["normal"], aov["depth"], var, hist, _without=rule, **kw)
    return G.reference((G.W, G.H), ITERATIONS, demodulate), wrong


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("rule", SR.RULES)
def test_frame_exposes_rule(rule, demodulate):
    ref, wrong = knocked_out(rule, demodulate)
    delta = np.abs(ref["out"] - wrong["out"]).max() / np.abs(ref["out"]).max()
    dvar = np.abs(ref["variance"] - wrong["variance"]).max() / ref["variance"].max()
    print(f"without {rule}, demodulate {demodulate}: max|d colour| / max|c| = {delta:.3g}, "
          f"max|d variance| / max v = {dvar:.3g}")
    assert delta >= 100 * G.BOUND["colour"]
    if rule == "squared":                                  # the rule that is about the variance output
        assert dvar >= 100 * G.BOUND["variance"]


def test_every_rule_is_knocked_out():
    assert set(SR.RULES) == {"per_pixel_variance", "prefilter", "estimate", "boost", "squared"}
    with pytest.raises(AssertionError):
        rad, aov, var, hist = G.synthetic()
        SR.svgf_ref(rad, aov["albedo"], aov["normal"], aov["depth"], var, hist, _without="no such rule")


@pytest.mark.parametrize("size", [(G.W, G.H)] + [s for s, _ in G.NEW_CASES])
def test_synthetic_restates_the_denoiser_frame(size):
    w, h = size
    rad, aov, var, hist = G.synthetic(w, h)
    rad0, aov0 = D.synthetic(w, h, 11)
    assert np.array_equal(rad.view(np.uint32), rad0.view(np.uint32))
    for k in ("albedo", "normal", "depth"):
        assert aov[k].dtype == np.float32 and np.array_equal(aov[k].view(np.uint32), aov0[k].view(np.uint32))
    assert var.dtype == np.float32 and var.shape == (h, w) and hist.dtype == np.float32 and hist.shape == (h, w)
    assert var.min() >= 0.0 and var.max() <= 0.5
    assert set(np.unique(hist)) <= set(range(1, 9))


def test_new_planes_at_37x29():
    _, _, var, hist = G.synthetic()
    assert (var[10:14, 3:9] == 0.0).all() and (var == 0.0).sum() == 24     # the block of zeros, nothing else
    short = (hist < G.SIG["min_history"]).mean()
    assert 0.33 <= short <= 0.40
    assert set(np.unique(hist)) == set(range(1, 9))
