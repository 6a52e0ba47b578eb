"""The inputs of tests/test_gpu_deform.py have teeth: for each rule that tpt_temporal_deform adds
to tpt_temporal's definition (DESIGN.md section 5 "Deforming meshes") a case exists whose last
frame moves by at least 100 times the GPU test's bound when that rule is knocked out of the
float64 reference (tests/deform_ref.py).  A kernel without the rule then cannot pass the GPU
comparison of that case.  CPU only, on feature buffers computed in numpy
(deform_scenes.numpy_guides): the reference against a wrong copy of itself."""
import numpy as np
import pytest

from tests import deform_cases as DC
from tests import test_gpu_deform as D

PAIRS = [(name, rule) for name, spec in DC.CASES.items() for rule in spec[2]]
RULES = {"X", "ne", "current", "snapshot"}


def moved_by(ref, wrong):
    dec = ref["decidable"]
    delta = np.abs(ref["out"] - wrong["out"])[dec].max() / np.abs(ref["out"]).max()
    flipped = int((ref["reprojected"] != wrong["reprojected"])[dec].sum())
    return delta, flipped, int((~dec).sum())


@pytest.mark.parametrize("name,rule", PAIRS)
def test_case_exposes_rule(name, rule):
    seq, params, refs = DC.case(name)
    wrong = DC.reference(seq, params, _without=rule)[1]
    delta, flipped, undecidable = moved_by(refs[1], wrong)
    print(f"{name} without {rule}: max|d out| / max|out| = {delta:.3g}, {flipped} pixels change side, "
          f"{undecidable} undecidable")
    assert delta >= 100 * D.BOUND


def test_alternation_exposes_the_snapshot_rule():
    """"The snapshot is always valid": after a tpt_temporal call in between, the hit pixels are
    reprojected through a snapshot two calls old instead of being disoccluded."""
    seq = DC.sequence(DC.ALTERNATION)
    params = dict(DC.PARAMS, demodulate=True)
    refs = DC.reference(seq, params)
    wrong = DC.reference(seq, params, _without="snapshot")
    delta, flipped, _ = moved_by(refs[2], wrong[2])
    print(f"alternation without snapshot: max|d out| / max|out| = {delta:.3g}, {flipped} pixels change side")
    assert delta >= 100 * D.BOUND and flipped > 400
    for k in range(2):                                      # and only there
        assert np.array_equal(refs[k]["out"], wrong[k]["out"])


def test_every_rule_has_a_case():
    assert {rule for _, rule in PAIRS} | {"snapshot"} == RULES
    for letter, name in zip("abcde", DC.CASES):             # the five deformations, each with a rule to decide
        assert DC.CASES[name][2], letter


def test_knock_outs_change_nothing_when_nothing_deforms():
    """The rules act on deformed triangles only."""
    seq = DC.sequence([(DC.STATIC, DC.REST, 101), (DC.MOVED, DC.REST, 202)])
    params = dict(DC.PARAMS, demodulate=True)
    ref = DC.reference(seq, params)[1]
    for rule in ("X", "ne", "current", "snapshot"):
        wrong = DC.reference(seq, params, _without=rule)[1]
        assert np.array_equal(ref["out"], wrong["out"]) and np.array_equal(ref["motion"], wrong["motion"])


def test_bound_is_below_its_ceiling():
    assert D.BOUND <= min(D.ceiling(w, h) for w, h in ((DC.W, DC.H),) + DC.SIZES + DC.TINY)
    assert D.BOUND == 10 * D.MEASURED_MAX
