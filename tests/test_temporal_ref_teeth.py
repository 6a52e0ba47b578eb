"""The inputs of tests/test_gpu_temporal.py's rule cases have teeth: for each rule of
tpt_temporal's definition (DESIGN.md section 5 "Post-pass") a case exists whose second
frame moves by at least 100 times the GPU test's bound when that rule is knocked out
of the float64 reference.  A kernel without the rule then cannot pass the GPU
comparison of that case.  CPU only: the reference against a wrong copy of itself.

Also here: the reference helpers that were generalised (TR.camera's pitch and roll,
test_gpu_denoise.synthetic's frame size) still give what they gave before, bit for bit."""
import numpy as np
import pytest

from tests import temporal_ref as TR
from tests import test_gpu_temporal as G
from tests import test_gpu_denoise as D

PAIRS = [(case, rule) for case, spec in G.RULE_CASES.items() for rule in spec[3]]


def knocked_out(rule, case, demodulate=True):
    """(reference, reference without `rule`) for frame 2 of the case."""
    (cam1, cam2), (f1, f2), params, (r1, r2) = G.two_frames(case, demodulate)
    state, kw = r1["state"], dict(params)
    if rule == "depth":
        kw["depth_tol"] = 1e9
    elif rule == "normal":
        kw["normal_min"] = -1.0
    elif rule == "sensor":                                 # the previous camera with the current one's sensor
        state = dict(state, cam=dict(state["cam"], vfov=cam2["vfov"], aspect=cam2["aspect"]))
    else:
        kw["_without"] = rule
    return r2, TR.temporal_ref(state, cam2, *f2, **kw)


@pytest.mark.parametrize("case,rule", PAIRS)
def test_case_exposes_rule(case, rule):
    ref, wrong = knocked_out(rule, case)
    dec = ref["decidable"]
    delta = np.abs(ref["out"] - wrong["out"])[dec].max() / np.abs(ref["out"]).max()
    flipped = int((ref["reprojected"] != wrong["reprojected"])[dec].sum())
    print(f"{case} without {rule}: max|d out| / max|out| = {delta:.3g}, {flipped} pixels change side, "
          f"{int((~dec).sum())} undecidable")
    assert delta >= 100 * G.BOUND_NEW


def test_every_rule_has_a_case():
    assert {rule for _, rule in PAIRS} == {"depth", "normal", "prev_origin", "sensor", "front"}


@pytest.mark.parametrize("case", list(G.RULE_CASES))
@pytest.mark.parametrize("demodulate", [False, True])
def test_case_is_decidable(case, demodulate):
    """A condition on the inputs, which the GPU comparison asserts again."""
    _, _, _, (r1, r2) = G.two_frames(case, demodulate)
    for r in (r1, r2):
        assert (~r["decidable"]).mean() <= 0.01
        assert np.isfinite(r["out"]).all() and np.isfinite(r["variance"]).all()


def test_turn_180_sees_nothing_of_frame_1():
    (_, cam2), (_, f2), _, (_, r2) = G.two_frames("turn_180")
    assert not r2["reprojected"].any() and r2["decidable"].all()
    _, wrong = knocked_out("front", "turn_180")
    sky = f2[1]["material"] < 0
    assert (wrong["reprojected"] & sky).sum() > 100        # a mirrored projection would find history for the sky


def test_present_cases_cannot_see_the_rules():
    """Why the rule cases exist: the three-material cases of test_matches_numpy_reference
    do not move at all when the depth or the normal rule is knocked out."""
    cam1 = G.CAMERAS["static"]
    f1 = G.frame(cam1, 101)
    r1 = TR.temporal_ref(None, cam1, *f1, demodulate=True, **G.PARAMS)
    for name in ("translate", "yaw_translate"):
        f2 = G.frame(G.CAMERAS[name], 202)
        ref = TR.temporal_ref(r1["state"], G.CAMERAS[name], *f2, demodulate=True, **G.PARAMS)
        for kw in ({"depth_tol": 1e9}, {"normal_min": -1.0}):
            wrong = TR.temporal_ref(r1["state"], G.CAMERAS[name], *f2, demodulate=True, **dict(G.PARAMS, **kw))
            assert np.array_equal(ref["out"], wrong["out"])


@pytest.mark.parametrize("yaw,move", [(0.0, (0.0, 0.0, 0.0)), (1.5, G.MOVE), (2.0, (0.0, 0.0, 0.0)),
                                      (3.0, (0.26, 0.10, 0.04)), (180.0, (0.0, 0.0, 0.0))])
def test_camera_without_pitch_and_roll_is_what_it_was(yaw, move):
    t = np.deg2rad(yaw)                                    # TR.camera before it took pitch_deg and roll_deg
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(t), np.sin(t), -np.sin(t), np.cos(t)
    m[:3, 3] = move
    was = m.T.reshape(16).astype(np.float32)
    for cam in (TR.camera(yaw, move, aspect=G.ASPECT), TR.camera(yaw, move, aspect=G.ASPECT, pitch_deg=0.0, roll_deg=0.0)):
        assert np.array_equal(cam["c2w"].view(np.uint32), was.view(np.uint32))
        assert cam["vfov"] == 0.8 and cam["aspect"] == G.ASPECT


def test_camera_pitch_and_roll():
    """R = R_y(yaw) R_x(pitch) R_z(roll): a rotation; roll alone keeps the viewing axis,
    pitch alone keeps +x, and the order is yaw last."""
    c = TR.camera(10.0, (1.0, 2.0, 3.0), pitch_deg=-20.0, roll_deg=30.0)
    m = c["c2w"].astype(np.float64).reshape(4, 4).T
    r = m[:3, :3]
    assert np.abs(r @ r.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(r) - 1.0) < 1e-6
    assert np.array_equal(m[:3, 3], [1.0, 2.0, 3.0]) and np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0])
    roll = TR.camera(roll_deg=30.0)["c2w"].astype(np.float64).reshape(4, 4).T[:3, :3]
    assert np.allclose(roll @ [0, 0, 1], [0, 0, 1]) and np.allclose(roll @ [1, 0, 0], [np.cos(np.pi / 6), 0.5, 0])
    pitch = TR.camera(pitch_deg=-20.0)["c2w"].astype(np.float64).reshape(4, 4).T[:3, :3]
    assert np.allclose(pitch @ [1, 0, 0], [1, 0, 0])
    assert pitch[1, 2] > 0                                 # pitch < 0: the view direction -z tips down (-y)
    yaw = TR.camera(10.0)["c2w"].astype(np.float64).reshape(4, 4).T[:3, :3]
    assert np.allclose(r, yaw @ pitch @ roll, atol=1e-7)


def test_guides_materials_change_nothing_else():
    cam = G.CAMERAS["yaw_translate"]
    a, b = TR.synthetic_guides(cam, G.W, G.H), TR.synthetic_guides(cam, G.W, G.H, G.ONE)
    assert np.array_equal(a["depth"], b["depth"]) and np.array_equal(a["normal"], b["normal"])
    assert np.array_equal(a["material"] < 0, b["material"] < 0)
    assert set(np.unique(a["material"])) == {-1, 0, 1, 2} and set(np.unique(b["material"])) == {-1, 0}


def test_denoise_synthetic_at_37x29_is_what_it_was():
    W, H = 37, 29                                          # test_gpu_denoise.synthetic before it took a size
    rng = np.random.default_rng(11)
    rad = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    alb = rng.uniform(0.2, 1.0, (H, W, 3)).astype(np.float32)
    nrm = np.zeros((H, W, 3), np.float32)
    nrm[:, :20] = (0.0, 0.0, 1.0)
    nrm[:, 20:] = (0.6, 0.0, 0.8)
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    z = (2.0 + 0.01 * x + np.where(y >= 15, 1.5, 0.0)).astype(np.float32)
    nrm[3:9, 25:33] = 0.0
    z[3:9, 25:33] = 0.0
    alb[3:9, 25:33] = 1.0
    alb[20, 5] = 0.0
    rad[20, 5] = 0.0
    for got in (D.synthetic(), D.synthetic(37, 29, 11)):
        for a, b in ((got[0], rad), (got[1]["albedo"], alb), (got[1]["normal"], nrm), (got[1]["depth"], z)):
            assert a.dtype == np.float32 and a.shape == b.shape
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("w,h", D.NEW_SIZES)
def test_denoise_synthetic_features_scale(w, h):
    """Each feature is there wherever the frame can hold it, and the reference is finite."""
    from tests import post_ref as R
    rad, aov = D.synthetic(w, h, 11)
    assert rad.shape == (h, w, 3) and aov["depth"].shape == (h, w)
    miss = aov["depth"] == 0.0
    assert ((aov["normal"] == 0.0).all(-1) == miss).all() and (aov["albedo"][miss] == 1.0).all()
    if w >= 37 and h >= 29:
        assert miss.any()
    if w >= 2:
        assert len(np.unique(aov["normal"][~miss], axis=0)) == 2       # two normal regions
    if h >= 2:
        assert (aov["depth"][~miss].max() - aov["depth"][~miss].min()) >= 1.5   # the depth step
    if w * h > 1:
        assert ((aov["albedo"] == 0.0).all(-1)).sum() == 1            # the black-albedo pixel
    for its in {iterations for (ww, hh), iterations in D.NEW_CASES if (ww, hh) == (w, h)}:
        ref = R.atrous_ref(rad, aov["albedo"], aov["normal"], aov["depth"], its, demodulate=True, **D.SIG)
        assert np.isfinite(ref).all()
