"""tpt_temporal_path on the CPU: the premises of its definition restated with the oracle, the
teeth of tests/temporal_path_ref.py, and that the device cases of
tests/test_gpu_temporal_path.py are decidable.

Premises (DESIGN.md section 5 "Temporal accumulation through mirrors").  The input is a
noise-free signal 0.5 + 0.5 sin(2 pi P / (z_med / 8)) of each pixel's terminal point P, two
frames at alpha 0.1, the second camera translated.  What the second frame blends in is then
known: history = (out - k truth) / (1 - k) with k = 1/2, and its distance from the truth is
the wrong history a rule lets through.  A pixel is bad above 0.1 (mean over the channels)."""
import numpy as np
import pytest

from tests import temporal_path_cases as K
from tests import temporal_path_ref as TP
from tests import temporal_ref as TR

W, H = 96, 54


def signal(points, z_med):
    return (0.5 + 0.5 * np.sin(2.0 * np.pi * points.astype(np.float64) / (z_med / 8.0))).astype(np.float32)


_PREMISE = {}


def premise(name):
    """name -> {rule: (kept, mean error, bad)} over the reprojected pixels of frame 2 whose
    first hit is a mirror, and the number of such pixels.  S0: tpt_temporal on first-hit
    guides; S1: the virtual point and k' = k alone (point_tol 1e9); S4: the definition at one
    and at two footprints."""
    if name in _PREMISE:
        return _PREMISE[name]
    cap = K.cap_of(name)
    cam1 = K.scene_camera(name)
    cam2 = K.moved(cam1, K.translation(name))
    z_med = K.median_depth(name)
    paths = [K.walk(name, W, H, cap, c) for c in (cam1, cam2)]
    firsts = [K.walk(name, W, H, 0, c) for c in (cam1, cam2)]
    rads = [signal(p["points"], z_med) for p in paths]
    mirror = K.mirror_first_hit(name, paths[1])
    res = {"mirror_px": int(mirror.sum())}

    def score(r2):
        hist = 2.0 * r2["out"] - rads[1]                  # N = 2: k = max(alpha, 1 / 2)
        err = np.abs(hist - rads[1]).mean(-1)
        on = mirror & r2["reprojected"]
        return int(on.sum()), float(err[on].mean()) if on.any() else 0.0, int((err[on] > 0.1).sum())

    r1 = TR.temporal_ref(None, cam1, rads[0], firsts[0], demodulate=False, **K.PARAMS)
    res["S0"] = score(TR.temporal_ref(r1["state"], cam2, rads[1], firsts[1], demodulate=False, **K.PARAMS))
    for rule, tol in (("S1", 1e9), ("S4_1", 1.0), ("S4_2", 2.0)):
        chain = K.run_reference(list(zip(rads, paths)), (cam1, cam2), False, point_tol=tol)
        res[rule] = score(chain[1])
    print(name, res)
    _PREMISE[name] = res
    return res


@pytest.mark.parametrize("name,kept_min", [("hall", 300), ("box2", 100), ("tilted", 0), ("box", 1)])
def test_one_footprint_lets_no_wrong_history_through(name, kept_min):
    res = premise(name)
    kept, _, bad = res["S4_1"]
    assert bad == 0
    assert kept >= kept_min


def test_first_hit_reprojection_ghosts_on_a_planar_mirror():
    """What tpt_temporal does today under a translated camera: the mirror's surface point
    passes every test, and another reflection's history is blended in."""
    res = premise("hall")
    assert res["S0"][2] > 100
    assert res["S4_1"][1] < res["S1"][1] < res["S0"][1]    # each rule removes wrong history


# ---- the teeth of temporal_path_ref ----



def frames_of(case, demodulate=False):
    name, w, h, cap, _ = K.GPU_CASES[case]
    cams = K.case_cameras(case)
    paths = [K.walk(name, w, h, cap, c) for c in cams]
    return cams, [(K.radiance(101 + 101 * i, p), p) for i, p in enumerate(paths)]


@pytest.mark.parametrize("rule,case", [("k", "hall_two"), ("point", "hall_two"), ("point", "box2_two"),
                                       ("point", "tilted_two"), ("direction", "box_two"), ("virtual", "hall_two"),
                                       ("virtual", "box2_two")])
def test_reference_has_teeth(rule, case):
    """Each rule knocked out of the reference moves the last frame of a device case by at least
    100 times the device tests' bound (temporal_path_cases.GPU_BOUND): a kernel without the rule
    fails them."""
    cams, frames = frames_of(case)
    good = K.run_reference(frames, cams, False)[-1]
    wrong = K.run_reference(frames, cams, False, without=rule)[-1]
    both = good["decidable"] & wrong["decidable"]
    moved = np.abs(good["out"] - wrong["out"])[both].max() / np.abs(good["out"]).max()
    changed = int((good["reprojected"] != wrong["reprojected"])[both].sum())
    print(f"{rule} on {case}: moves the output by {moved:.3e} of its range, {changed} pixels change sides")
    assert moved >= 100 * K.GPU_BOUND
    assert changed > 0


@pytest.mark.parametrize("case", list(K.GPU_CASES))
@pytest.mark.parametrize("demodulate", [False, True])
def test_device_cases_are_decidable(case, demodulate):
    """With the reference alone: at most 1 % of a case's pixels fall within the margins of a
    threshold, in every frame."""
    cams, frames = frames_of(case)
    for i, r in enumerate(K.run_reference(frames, cams, demodulate)):
        und = (~r["decidable"]).mean()
        print(f"{case} frame {i + 1}: {(~r['decidable']).sum()} undecidable, {int(r['reprojected'].sum())} reprojected")
        assert und <= 0.01


def test_cap_zero_buffers_are_first_hit_accumulation():
    """Rule 5 in the reference: with k = 0 everywhere temporal_path_ref is temporal_ref."""
    name = "box2"
    cams = K.case_cameras("box2_chain")
    paths = [K.walk(name, 80, 45, 0, c) for c in cams]
    frames = [(K.radiance(7 + i, p), p) for i, p in enumerate(paths)]
    got = K.run_reference(frames, cams, True)
    state = None
    for cam, (rad, aov), g in zip(cams, frames, got):
        r = TR.temporal_ref(state, cam, rad, aov, demodulate=True, **K.PARAMS)
        state = r["state"]
        assert np.array_equal(r["out"], g["out"]) and np.array_equal(r["history_len"], g["history_len"])
        assert np.array_equal(r["decidable"], g["decidable"])
    assert (got[-1]["history_len"] > 2).any()


def test_a_first_hit_call_disoccludes_the_mirror_pixels():
    """Rule 6 in the reference: after a tpt_temporal call every stored k' is 0."""
    cams, frames = frames_of("hall_two")
    r1 = TR.temporal_ref(None, cams[0], *frames[0], demodulate=False, **K.PARAMS)
    r2 = TP.temporal_path_ref(r1["state"], cams[1], *frames[1], demodulate=False,
                              point_tol=K.POINT_TOL, **K.PARAMS)
    followed = frames[1][1]["bounces"] > 0
    assert followed.sum() > 300
    assert not r2["reprojected"][followed].any()
    assert r2["reprojected"][~followed].any()
