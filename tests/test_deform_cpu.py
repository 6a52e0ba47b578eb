"""Deforming meshes without a GPU: the numpy restatement of tpt_temporal_deform
(tests/deform_ref.py) where nothing deforms, the test scene and its deformations
(tests/deform_scenes.py), and the cap on undecidable pixels of every case the GPU tests run
(tests/deform_cases.py), on feature buffers computed in numpy."""
import numpy as np
import pytest

from tests import deform_cases as DC
from tests import deform_ref as DR
from tests import deform_scenes as DS
from tests import temporal_ref as TR


@pytest.mark.parametrize("demodulate", [False, True])
def test_reference_with_nothing_deformed_is_temporal_ref(demodulate):
    """The sheet at rest: temporal_ref.temporal_ref on the same inputs, array for array, over three
    frames of a moving camera; the motion is the camera's alone."""
    seq = DC.sequence([(c, DC.REST, seed) for c, seed in zip((DC.STATIC, DC.MOVED, DC.THIRD), (101, 202, 303))])
    params = dict(DC.PARAMS, demodulate=demodulate)
    mine = DC.reference(seq, params)
    state = None
    for k, (cam, wv, wn, rad, aov, _) in enumerate(seq):
        ref = TR.temporal_ref(state, cam, rad, aov, **params)
        state = ref["state"]
        for key in ("out", "variance", "history_len", "reprojected", "decidable"):
            assert np.array_equal(mine[k][key], ref[key]), (k, key)
        for key in ("C", "N", "M1", "M2", "n", "z", "m"):
            assert np.array_equal(mine[k]["state"][key], ref["state"][key]), (k, key)
    assert (mine[0]["motion"] == 0.0).all() and np.abs(mine[1]["motion"]).max() > 0.5
    assert mine[2]["reprojected"].any() and (~mine[2]["reprojected"]).any()
    assert (mine[2]["history_len"] == 3.0).any()


def test_another_entry_point_is_temporal_ref_and_invalidates_the_snapshot():
    seq = DC.sequence(DC.ALTERNATION)
    params = dict(DC.PARAMS, demodulate=True)
    refs = DC.reference(seq, params)
    cam, wv, wn, rad, aov, deform = seq[1]
    theirs = TR.temporal_ref(refs[0]["state"], cam, rad, aov, **params)
    assert not deform and np.array_equal(refs[1]["out"], theirs["out"]) and (refs[1]["motion"] == 0.0).all()
    assert refs[1]["state"]["snap_valid"] is False
    hit = seq[2][4]["material"] >= 0
    r = refs[2]
    assert (r["history_len"][hit] == 1.0).all() and np.allclose(r["out"][hit], seq[2][3][hit], rtol=0, atol=1e-12)
    assert (r["history_len"][~hit] == 3.0).all() and (~hit).sum() > 100      # the sky keeps its history
    assert r["state"]["snap_valid"] is True


def test_scene_is_what_the_cases_assume():
    idx, v, n, lut = DS.rest()
    assert len(idx) == 3 * DS.N_FACES == 3 * 130 and len(v) == 85 and DS.N_SHEET_FACES == 128
    assert lut.tolist() == [[0, 0], [128, 1]] and int(idx.max()) == 84
    aov = DS.numpy_guides(DC.STATIC, DC.W, DC.H, v, n)
    sheet, wall, sky = aov["face"] < 128, aov["face"] >= 128, aov["face"] < 0
    sheet &= ~sky
    assert sheet.sum() > 400 and wall.sum() > 200 and sky.sum() > 300
    assert sheet[DC.H // 2, DC.W // 2] and sky[0].all() and sky[:, 0].all() and sky[-1].all() and sky[:, -1].all()
    # (the depth is the ray parameter, and the library's rays are 0.17 % short of unit length: frsqrt)
    assert 2.5 <= aov["depth"][sheet].min() < 2.51 and (aov["material"][wall] == 1).all()
    assert len(np.unique(aov["face"][sheet])) == 128                       # every triangle of the sheet is seen
    assert np.abs(np.linalg.norm(aov["normal"][~sky], axis=-1) - 1.0).max() < 1e-6


def test_deformations_are_the_sizes_the_cases_name():
    _, v, n, _ = DS.rest()
    s = v[:DS.N_SHEET_VERTS]
    px = DC.H / float(TR.sensor(0.8, DC.ASPECT)[1]) / 2.5                   # pixels per world unit at the sheet
    b, bn = DS.bulge(s)
    assert bn is None and np.isclose((b - s)[:, 2].max(), 0.6, atol=1e-6) and 0.6 <= 2.5 / 4
    assert np.array_equal(b[:, :2], s[:, :2])
    w, wn = DS.swirl(s)
    step = np.linalg.norm(w - s, axis=-1).max() * px
    assert wn is None and 1.3 <= step <= 1.6 and (w[:, 2] == s[:, 2]).all()
    d, dn = DS.bend(s)
    tilt = np.degrees(np.arccos(np.clip(dn[:, 2], -1, 1)))
    assert 5.5 <= tilt.max() <= 6.0 and np.cos(np.radians(tilt.max())) < 0.999
    assert np.abs(d - s).max() / 2.5 < 0.02                                 # far inside depth_tol
    h, hn = DS.half(s)
    moved = (h != s).any(-1)
    assert hn is None and moved.sum() == 36 and np.array_equal(_bits(h[~moved]), _bits(s[~moved]))
    # under `half` a wave of 64 neighbouring pixels holds static and deformed triangles
    wv, wn = DS.deformed(DS.half)
    f = DS.numpy_guides(DC.STATIC, DC.W, DC.H, wv, wn)["face"]
    tri = DS.rest()[0].reshape(-1, 3)
    static_tri = np.array([np.array_equal(_bits(wv[t]), _bits(v[t])) for t in tri])
    row = f[DC.H // 2]
    kinds = {bool(static_tri[x]) for x in row if 0 <= x < 128}
    assert kinds == {True, False}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _all_sequences():
    for name in DC.CASES:
        for demodulate in (False, True):
            seq, params, refs = DC.case(name, demodulate)
            yield f"{name} demodulate {demodulate}", seq, refs, 0.01
    params = dict(DC.PARAMS, demodulate=True)
    for tag, spec in (("chain", DC.CHAIN), ("alternation", DC.ALTERNATION)):
        seq = DC.sequence(spec)
        yield tag, seq, DC.reference(seq, params), 0.01
    for w, h in DC.SIZES:
        seq, _, refs = DC.sized(w, h)
        yield f"{w} x {h}", seq, refs, 0.01
    for w, h in DC.TINY:
        seq, _, refs = DC.sized(w, h)
        yield f"{w} x {h}", seq, refs, 0.0                                  # none at all in the tiny frames


def test_every_gpu_case_is_decidable():
    """At most 1 % of any reference frame sits on a threshold (none of a tiny frame), and
    everything is finite."""
    for tag, seq, refs, cap in _all_sequences():
        for k, r in enumerate(refs):
            und = (~r["decidable"]).mean()
            assert und <= cap, f"{tag} frame {k + 1}: {(~r['decidable']).sum()} undecidable"
            assert np.isfinite(r["out"]).all() and np.isfinite(r["variance"]).all() and np.isfinite(r["motion"]).all()


@pytest.mark.parametrize("name", list(DC.CASES))
def test_deformed_sheet_is_reprojected(name):
    """The sheet finds its history under every deformation: more than nine tenths of its pixels,
    the rest being what the deformation uncovers at its rim."""
    seq, params, refs = DC.case(name)
    f = seq[1][4]["face"]
    sheet = (f >= 0) & (f < DS.N_SHEET_FACES)
    r = refs[1]
    assert sheet.sum() > 400 and (r["reprojected"] & sheet).sum() > 0.9 * sheet.sum()
    assert np.abs(r["motion"][sheet]).max() > 0.1


def test_chain_has_whole_and_blended_histories():
    seq = DC.sequence(DC.CHAIN)
    n = DC.reference(seq, dict(DC.PARAMS, demodulate=True))[2]["history_len"]
    assert (n == 3.0).any() and (n == 1.0).any() and ((n > 2.0) & (n < 3.0)).any()


def test_bad_faces_and_flat_triangles_disocclude():
    """A face id outside [0, n_faces) and a triangle of zero area on hit pixels: N = 1 and the
    output is the input; the other pixels as without them."""
    seq, params, refs = DC.case("swirl")
    idx = DS.rest()[0]
    cam, wv, wn, rad, aov, _ = seq[1]
    sheet = (aov["face"] >= 0) & (aov["face"] < DS.N_SHEET_FACES)
    for bad in (-1, DS.N_FACES):
        g = dict(aov, face=np.where(sheet, bad, aov["face"]).astype(np.int32))
        r = DR.temporal_deform_ref(refs[0]["state"], cam, rad, g, idx, wv, wn, **params)
        assert (r["history_len"][sheet] == 1.0).all() and (r["motion"][sheet] == 0.0).all()
        assert np.array_equal(r["out"][~sheet], refs[1]["out"][~sheet])
    flat = idx.copy().reshape(-1, 3)
    target = int(aov["face"][DC.H // 2, DC.W // 2])
    flat[target, 2] = flat[target, 1]                                       # two corners the same vertex
    r = DR.temporal_deform_ref(refs[0]["state"], cam, rad, aov, flat.reshape(-1), wv, wn, **params)
    on = aov["face"] == target
    assert on.sum() >= 1 and (r["history_len"][on] == 1.0).all()
    assert np.allclose(r["out"][on], rad[on], rtol=0, atol=1e-12)                     # (float64 demodulation: rounding)
    assert np.array_equal(r["out"][~on], refs[1]["out"][~on])
