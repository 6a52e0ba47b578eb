"""The inputs of tests/test_gpu_motion.py have teeth: for each rule that tpt_temporal_motion
adds to tpt_temporal's definition (DESIGN.md section 5 "Moving objects") a case exists whose
second frame moves by at least 100 times the GPU test's bound when that rule is knocked out
of the float64 reference (tests/motion_ref.py).  A kernel without the rule then cannot pass
the GPU comparison of that case.  Also the conditions on those inputs that the GPU
comparisons rely on.  CPU only: the reference against a wrong copy of itself."""
import numpy as np
import pytest

from tests import motion_ref as MR
from tests import test_gpu_motion as M

PAIRS = [(name, rule) for name, spec in M.MOTION_CASES.items() for rule in spec[3]]


@pytest.mark.parametrize("name,rule", PAIRS)
def test_case_exposes_rule(name, rule):
    seq, params, refs = M.case(name)
    wrong = M.reference(seq, params, _without=rule)[1]
    ref = refs[1]
    dec = ref["decidable"]
    delta = np.abs(ref["out"] - wrong["out"])[dec].max() / np.abs(ref["out"]).max()
    flipped = int((ref["reprojected"] != wrong["reprojected"])[dec].sum())
    print(f"{name} without {rule}: max|d out| / max|out| = {delta:.3g}, {flipped} pixels change side, "
          f"{int((~dec).sum())} undecidable")
    assert delta >= 100 * M.BOUND


def test_every_rule_has_a_case():
    assert {rule for _, rule in PAIRS} == {"D", "G", "dist"}


def test_knock_outs_change_nothing_when_nothing_moves():
    """The three rules act on moved objects only."""
    seq = M.sequence([(M.STATIC, {}, 101), (M.G.CAMERAS["yaw_translate"], {}, 202)])
    params = dict(M.PARAMS, demodulate=True)
    ref = M.reference(seq, params)[1]
    for rule in ("D", "G", "dist"):
        wrong = M.reference(seq, params, _without=rule)[1]
        assert np.array_equal(ref["out"], wrong["out"]) and np.array_equal(ref["motion"], wrong["motion"])


def _all_sequences():
    for name in M.MOTION_CASES:
        for demodulate in (False, True):
            seq, params, refs = M.case(name, demodulate)
            yield f"{name} demodulate {demodulate}", seq, refs
    for materials in ((0, 1, 2), M.ONE):
        seq = M.sequence(M.CHAIN, materials)
        yield f"chain {materials}", seq, M.reference(seq, dict(M.PARAMS, demodulate=True))
    for w, h in ((131, 9), (70, 70), (1, 1), (3, 2), (16, 16)):
        seq, params, refs = M.sized(w, h)
        yield f"{w} x {h}", seq, refs


def test_every_gpu_case_is_decidable():
    """At most 1 % of any reference frame sits on a threshold, and everything is finite."""
    for tag, seq, refs in _all_sequences():
        for k, r in enumerate(refs):
            assert (~r["decidable"]).mean() <= 0.01, f"{tag} frame {k + 1}: {(~r['decidable']).sum()} undecidable"
            assert np.isfinite(r["out"]).all() and np.isfinite(r["variance"]).all() and np.isfinite(r["motion"]).all()


@pytest.mark.parametrize("name", list(M.MOTION_CASES))
def test_moved_patch_is_reprojected_and_uncovers(name):
    """The moved patch finds its history and its motion disoccludes pixels (but for the turn
    about its own centre, M.NOTHING_UNCOVERED); where the patch enters the frame
    (M.EDGE_CASES) some of them are its own."""
    seq, params, refs = M.case(name)
    r = refs[1]
    on = seq[1][2][1]["face"] == MR.patch_faces(M.CARRIER)[M.MOVED_PATCH[name]]
    dec = r["decidable"]
    assert on.sum() > 100
    assert (r["reprojected"] & on & dec).sum() > 100
    assert (~r["reprojected"] & dec).any() == (name not in M.NOTHING_UNCOVERED)
    if name in M.EDGE_CASES:
        assert (~r["reprojected"] & on & dec).sum() >= 5


def test_chain_has_whole_and_new_histories():
    seq = M.sequence(M.CHAIN)
    r = M.reference(seq, dict(M.PARAMS, demodulate=True))[2]
    n = r["history_len"]
    assert (n == 3.0).any() and (n == 1.0).any() and ((n > 2.0) & (n < 3.0)).any()
    vts = [vt for _, vt, _ in seq]
    flags = [MR.motion_matrices_ref(a, b)[2] for a, b in zip(vts, vts[1:])]
    assert flags[0][M.CUBE] == MR.TRACKED and flags[0][M.CUBE1] == MR.IDENTITY      # a different motion
    assert flags[1][M.CUBE] == MR.TRACKED and flags[1][M.CUBE1] == MR.TRACKED       # in each step
    assert not np.array_equal(*[MR.motion_matrices_ref(a, b)[0][M.CUBE] for a, b in zip(vts, vts[1:])])


def test_synthetic_faces_belong_to_their_objects():
    faces = MR.patch_faces(M.CARRIER)
    assert [int(M.CARRIER.face_object[f]) for f in faces] == list(MR.PATCH_OBJECTS)
    assert len(set(faces)) == 3 and all(0 <= f < M.CARRIER.n_faces for f in faces)
    lo, hi = M.CARRIER.faces_of(M.CUBE)
    assert faces[MR.STRIP] == hi - 1                       # the last face of its interval
