"""History clipping (tpt_history_set_clip; DESIGN.md section 5 "History clipping") on the GPU: the
four temporal entry points with the clip on against a float64 numpy restatement of the box and the
clamp (tests/clip_ref.py), the clip's identities bit for bit, and its refusals.
tests/test_clip_cpu.py shows on the CPU that the cases' inputs can see each rule of the
definition and that the reference alone meets the premises asserted here.

The clipped / not-clipped split is not an output of its own.  It is checked through the count
(clip_stats.clipped lies between the reference's count over the decidable pixels and that plus
the undecidable ones, and equals it where every pixel is decidable) and through the colours: a
pixel on the wrong side of the clip differs from the reference by its distance to the box edge."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests import clip_cases as K
from tests import clip_ref as CR
from tests import temporal_ref as TR
from tests import test_gpu_temporal as G

pytestmark = pytest.mark.gpu

# The bound.  test_gpu_temporal's a-priori ceiling stands: 4e-3 of the value range for the float32
# reprojected coordinate's 2^-14 px.  The clamp is 1-Lipschitz in the history colour, and the box
# edges are sums of at most 49 float32 terms (6e-6 relative at worst): neither adds to it.
# MEASURED_MAX is the largest max|gpu - ref| / max|ref| over colour, variance and history length
# of every comparison below on MI355X; the asserted bound is ten times that and must stay under
# the ceiling.  Measured (undecidable pixels of the last frame in brackets; every first frame has
# none and differs by rounding, 1e-16):
#   static, radius 3 / radius 1 undemodulated             3.6e-7 / 6.9e-7 (variance) [1 / 2]
#   translate, radius 1 / radius 3 undemodulated, tiles   1.85e-6 / 2.37e-6 [2 / 0]
#   pitch_roll, radius 3 / radius 1 in tiles              3.30e-6 / 3.29e-6 (variance) [2 / 2]
#   131 x 9, radius 3 / radius 1 undemodulated            1.263e-5 colour / 1.220e-5 variance [2 of 1,179]
#   5 x 3, radius 3 / radius 1 in tiles                   1.48e-6 / 3.0e-7 [0]
#   70 x 70 in tiles, radius 3                            5.69e-6 colour [22 of 4,900]
#   four-frame chain, cap 1                               2.05e-6, blended history lengths 1.04e-6 [1]
#   motion both_move / deform camera_bulge / path hall_two  1.91e-6 / 3.33e-6 / 6.38e-6 (variance) [1 / 4 / 6]
# These are the unclipped entry points' own figures on the same kinds of frame (test_gpu_temporal.py:
# 8.61e-6 at 131 x 9, 4.80e-6 at 70 x 70): the clip adds nothing that shows.  The largest is 1.5
# times the figure clip_ref.MARGIN was taken from, which leaves the margin 6.8 times it.
CEILING = G.CEILING
MEASURED_MAX = 1.263e-5             # colour, 131 x 9 radius 3 frame 2
BOUND = 10 * MEASURED_MAX
assert BOUND <= CEILING


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def ctx(gpu_available):
    """box2, built: tpt_temporal needs a device only, tpt_temporal_motion the objects' matrices,
    tpt_temporal_deform the world buffers."""
    from tests import test_gpu_motion as M
    d = M.T.Scene(M.scene_path("box2")).copySceneToDevice(0).build()
    yield d
    d.close()


def call(pt, hist, cam, rad, aov, entry="temporal", **kw):
    """One call of the entry point at the size of `rad`: (out, variance, history length, stats, motion_out),
    stats with the clip's figures too."""
    h, w = rad.shape[:2]
    var, n, st = np.full((h, w), -3.0, np.float32), np.full((h, w), -3.0, np.float32), {}
    kw = dict(kw, variance=var, history_len=n, stats=st)
    mv = None
    if entry in ("motion", "deform"):
        mv = kw["motion_out"] = np.full((h, w, 2), -3.0, np.float32)
        kw[entry] = True
    if entry == "path":
        out = pt.temporalPath(hist, G._cam(cam), rad, aov, **kw)
    else:
        out = pt.temporal(hist, G._cam(cam), rad, aov, **kw)
    st.update(hist.clip_stats())
    return out, var, n, st, mv


def play(d, cams, frames, params, clip, flags=0, entry="temporal", before=None, **kw):
    """A new history, the clip set (None: left off), through the frames.  before(k): called ahead of frame k."""
    h, w = frames[0][0].shape[:2]
    pt = T.PathTracer("", w, h, 0)
    hist = T.History(d, w, h)
    if clip is not None:
        hist.set_clip(**clip)
    got = []
    for k, (cam, (rad, aov)) in enumerate(zip(cams, frames)):
        if before is not None:
            before(k)
        got.append(call(pt, hist, cam, rad, aov, entry, flags=flags, **params, **kw))
    hist.close()
    return got


def compare(tag, got, ref, w, h, exact_n=True, bound=BOUND):
    """test_gpu_temporal.compare, then the clip's counts against the reference's, to within the
    undecidable pixels, and the premises of a clipped frame."""
    errs = G.compare(tag, got[:4], ref, exact_n=exact_n, bound=bound)
    st, dec = got[3], ref["decidable"]
    und = int((~dec).sum())
    clipped = int((ref["clipped"] & dec).sum())
    assert clipped <= st["clipped"] <= clipped + und, (tag, st, clipped, und)
    assert st["boxed"] == int(ref["boxed"].sum()), tag      # float32 decisions restated in float32: exact
    assert st["clipped"] <= st["reprojected"]
    return errs


@pytest.mark.parametrize("name", list(K.TWO_FRAME))
def test_two_frames_match_numpy_reference(ctx, name):
    cams, frames, params, clip, flags = K.two_frames(name)
    w, h = K.TWO_FRAME[name][:2]
    refs = K.reference(cams, frames, params, clip)
    got = play(ctx, cams, frames, params, clip, flags)
    K.premises(name, refs[1], w, h)
    for k in range(2):
        compare(f"{name} frame {k + 1}", got[k], refs[k], w, h)
    assert got[0][3]["clipped"] == 0 and got[0][3]["box_ms"] > 0.0


def test_four_frame_chain_matches_numpy_reference(ctx):
    """The cap (1) acts from frame 3 on: a clipped pixel's history length is 2 whatever it gathered."""
    cams, frames, params, clip, flags = K.chain()
    refs = K.reference(cams, frames, params, clip)
    got = play(ctx, cams, frames, params, clip, flags)
    for k in range(4):
        compare(f"chain frame {k + 1}", got[k], refs[k], G.W, G.H, exact_n=k < 2)
    n, ref = got[3][2], refs[3]
    sure = ref["decidable"]
    assert (n[ref["clipped"] & sure] == 2.0).all() and (n[sure] > 3.0).any()


def test_launch_shapes_agree(ctx):
    cams, frames, params, clip, _ = K.two_frames("70x70_r3_tiles")
    rows = play(ctx, cams, frames, params, clip, 0)
    tiles = play(ctx, cams, frames, params, clip, K.TILES)
    for a, b in zip(rows[1][:3], tiles[1][:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert {k: v for k, v in rows[1][3].items() if not k.endswith("_ms")} == \
           {k: v for k, v in tiles[1][3].items() if not k.endswith("_ms")}


def motion_frames(moving):
    """test_gpu_motion's frames: its both_move case, or its chain's cameras with nothing moved."""
    from tests import test_gpu_motion as M
    spec = M.MOTION_CASES["both_move"][0] if moving else [(c, {}, s) for c, _, s in M.CHAIN]
    seq = M.sequence(spec)
    return M, [c for c, _, _ in seq], [vt for _, vt, _ in seq], [(rad, CR.speck(aov)) for _, _, (rad, aov) in seq]


def still_inputs(ctx):
    """Three frames under a moving camera with nothing moved, nothing deformed and no mirror, as each
    entry point takes them: entry -> (frames, keywords)."""
    M, cams, vts, frames = motion_frames(False)
    ctx.set_transforms(0, M.CARRIER.rest)
    ctx.build()
    h, w = frames[0][0].shape[:2]
    flat = [(rad, dict(aov, bounces=np.zeros((h, w), np.int32), points=np.zeros((h, w, 3), np.float32)))
            for rad, aov in frames]
    return cams, {"temporal": (frames, {}), "motion": (frames, {}), "deform": (frames, {}),
                  "path": (flat, dict(point_tol=1.0))}


@pytest.mark.parametrize("flags", [0, _lib.TEMPORAL_TILES], ids=["rows", "tiles"])
@pytest.mark.parametrize("entry", ["temporal", "motion", "deform", "path"])
def test_loose_box_is_the_unclipped_call(ctx, entry, flags):
    """gamma = 1e30 on random colours: the box never bites, and every entry point gives the bits of
    the same call with the clip off -- the next frame's too, which proves the state."""
    cams, inputs = still_inputs(ctx)
    frames, kw = inputs[entry]
    params = dict(K.PARAMS, demodulate=True)
    off = play(ctx, cams, frames, params, None, flags, entry=entry, **kw)
    loose = play(ctx, cams, frames, params, dict(radius=2, gamma=1e30, max_history=1), flags, entry=entry, **kw)
    for k in range(3):
        for a, b in zip(off[k][:3], loose[k][:3]):
            assert np.array_equal(_bits(a), _bits(b)), (entry, k)
        if off[k][4] is not None:
            assert np.array_equal(_bits(off[k][4]), _bits(loose[k][4]))
        assert off[k][3]["reprojected"] == loose[k][3]["reprojected"]
        assert loose[k][3]["clipped"] == 0 and loose[k][3]["boxed"] > 900 and loose[k][3]["box_ms"] > 0.0
        assert (off[k][3]["clipped"], off[k][3]["boxed"], off[k][3]["box_ms"]) == (0, 0, 0.0)
    assert (off[2][2] == 3.0).any()


@pytest.mark.parametrize("flags", [0, _lib.TEMPORAL_TILES], ids=["rows", "tiles"])
def test_still_scene_is_clipped_tpt_temporal(ctx, flags):
    """Nothing moved, nothing deformed, no mirror: the three other entry points give clipped tpt_temporal's bits."""
    cams, inputs = still_inputs(ctx)
    params = dict(K.PARAMS, demodulate=True)
    got = {e: play(ctx, cams, frames, params, K.CLIP, flags, entry=e, **kw) for e, (frames, kw) in inputs.items()}
    assert got["temporal"][2][3]["clipped"] >= 20
    for e in ("motion", "deform", "path"):
        for k in range(3):
            for a, b in zip(got["temporal"][k][:3], got[e][k][:3]):
                assert np.array_equal(_bits(a), _bits(b)), (e, k)
            for f in ("reprojected", "clipped", "boxed"):
                assert got["temporal"][k][3][f] == got[e][k][3][f], (e, k, f)


def test_motion_case_matches_numpy_reference(ctx):
    """test_gpu_motion's both_move (the camera and the strip move) with the clip biting."""
    M, cams, vts, frames = motion_frames(True)
    params = dict(K.PARAMS, demodulate=True)
    refs, state = [], None
    for cam, vt, (rad, aov) in zip(cams, vts, frames):
        refs.append(M.MR.temporal_motion_ref(state, cam, rad, aov, M.CARRIER, vt, clip=K.CLIP, **params))
        state = refs[-1]["state"]
    got = play(ctx, cams, frames, params, K.CLIP, entry="motion", before=lambda k: ctx.set_transforms(0, vts[k]))
    K.premises("both_move", refs[1], G.W, G.H)
    for k in range(2):
        compare(f"motion both_move frame {k + 1}", got[k], refs[k], G.W, G.H)


def test_deform_case_matches_numpy_reference(gpu_available):
    """deform_cases' camera_bulge (the camera moves, the sheet bulges) with the clip biting, on the
    GPU's own feature and world buffers."""
    from tests import deform_cases as DC
    from tests import deform_ref as DR
    from tests import test_gpu_deform as D
    spec, extra, _ = DC.CASES["camera_bulge"]
    params = dict(DC.PARAMS, **extra, demodulate=True)
    d = D.DS.scene().copySceneToDevice(0).build()
    pt = T.PathTracer("", D.W, D.H, 0)
    hist = T.History(d, D.W, D.H).set_clip(**K.CLIP)
    refs, got, state = [], [], None
    for cam, (fn, kw), seed in spec:
        D.pose(d, fn, kw)
        aov = CR.speck(pt.renderAOV(d, G._cam(cam)))
        wv, wn = d.read_world()
        rad, _ = DC.colours(aov, seed)
        got.append(call(pt, hist, cam, rad, aov, "deform", **params))
        refs.append(DR.temporal_deform_ref(state, cam, rad, aov, D.IDX, wv, wn, clip=K.CLIP, **params))
        state = refs[-1]["state"]
    hist.close()
    d.close()
    K.premises("camera_bulge", refs[1], D.W, D.H)
    for k in range(2):
        compare(f"deform camera_bulge frame {k + 1}", got[k], refs[k], D.W, D.H)


def test_path_case_matches_numpy_reference(gpu_available):
    """temporal_path_cases' hall_two (mirrors, a translated camera) with the clip biting, on the GPU's
    own mirror-path buffers: the box compares bounce counts too."""
    from tests import temporal_path_cases as PK
    from tests import temporal_path_ref as TP
    from tests import variant_scenes as V
    name, w, h, cap, _ = PK.GPU_CASES["hall_two"]
    cams = PK.case_cameras("hall_two")
    d = V.device_scene(PK.source(name)).copySceneToDevice(0).build()
    pt = T.PathTracer("", w, h, 0)
    frames = []
    for i, c in enumerate(cams):
        buf = pt.renderAOVPath(d, G._cam(c), cap, points=True)
        frames.append((PK.radiance(101 + 101 * i, buf), CR.speck(buf)))
    params = dict(PK.PARAMS, demodulate=True)
    refs, state = [], None
    for cam, (rad, aov) in zip(cams, frames):
        refs.append(TP.temporal_path_ref(state, cam, rad, aov, clip=K.CLIP, point_tol=PK.POINT_TOL, **params))
        state = refs[-1]["state"]
    got = play(d, cams, frames, params, K.CLIP, entry="path", point_tol=PK.POINT_TOL)
    d.close()
    assert (frames[1][1]["bounces"] > 0).sum() >= 100      # mirrors are in view
    K.premises("hall_two", refs[1], w, h)
    for k in range(2):
        compare(f"path hall_two frame {k + 1}", got[k], refs[k], w, h)


def test_in_place_and_device_buffers(ctx):
    """radiance_out is radiance_in, in host and in device memory, and device inputs: the bits of the
    plain call.  The box is taken from the inputs before the temporal kernel overwrites them."""
    import torch
    cams, frames, params, clip, _ = K.two_frames("pitch_roll_r3")
    want = play(ctx, cams, frames, params, clip)
    h, w = frames[0][0].shape[:2]
    pt = T.PathTracer("", w, h, 0)
    dev = torch.device("cuda", 0)
    up = lambda a: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in a.items()}
    for on_device in (False, True):
        hist = T.History(ctx, w, h).set_clip(**clip)
        for k, (cam, (rad, aov)) in enumerate(zip(cams, frames)):
            buf = torch.from_numpy(rad.copy()).to(dev) if on_device else rad.copy()
            var = torch.zeros((h, w), device=dev) if on_device else np.zeros((h, w), np.float32)
            n = torch.zeros((h, w), device=dev) if on_device else np.zeros((h, w), np.float32)
            out = pt.temporal(hist, G._cam(cam), buf, up(aov) if on_device else aov, out=buf, variance=var, history_len=n,
                              **params)
            assert out is buf
            host = (lambda t: t.cpu().numpy()) if on_device else (lambda t: t)
            for a, b in zip((host(buf), host(var), host(n)), want[k][:3]):
                assert np.array_equal(_bits(a), _bits(b)), (on_device, k)
            assert hist.clip_stats()["clipped"] == want[k][3]["clipped"]
        hist.close()


def test_set_clip_none_returns_to_the_unclipped_bits(ctx):
    """The setting survives a reset; set_clip(None) after clipped calls gives a fresh, never clipped history's bits."""
    cams, frames, params, clip, _ = K.two_frames("translate_r1")
    off = play(ctx, cams, frames, params, None)
    on = play(ctx, cams, frames, params, clip)
    assert not np.array_equal(_bits(off[1][0]), _bits(on[1][0]))
    h, w = frames[0][0].shape[:2]
    pt = T.PathTracer("", w, h, 0)
    hist = T.History(ctx, w, h).set_clip(**clip)
    run = lambda: [call(pt, hist, cam, rad, aov, **params) for cam, (rad, aov) in zip(cams, frames)]
    run()
    hist.reset()                                           # the setting survives it
    again = run()
    hist.set_clip(None).reset()
    back = run()
    hist.close()
    for a, b, c, e in zip(again[1][:3], on[1][:3], back[1][:3], off[1][:3]):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(c), _bits(e))
    assert again[1][3]["clipped"] == on[1][3]["clipped"] > 0
    assert (back[1][3]["clipped"], back[1][3]["boxed"], back[1][3]["box_ms"]) == (0, 0, 0.0)


def test_refusals(ctx):
    """Each bad argument returns TPT_ERR_INVALID_ARG, writes nothing and leaves the setting as it was."""
    L = T.lib()
    cams, frames, params, clip, _ = K.two_frames("translate_r1")
    want_on = play(ctx, cams, frames, params, clip)
    want_off = play(ctx, cams, frames, params, None)
    h, w = frames[0][0].shape[:2]
    pt = T.PathTracer("", w, h, 0)
    bad = [(0, 1.0, 4, 0), (4, 1.0, 4, 0), (-1, 1.0, 4, 0), (3, 0.0, 4, 0), (3, -1.0, 4, 0), (3, float("nan"), 4, 0),
           (3, float("inf"), 4, 0), (3, 1.0, 0, 0), (3, 1.0, 65537, 0), (3, 1.0, -3, 0), (3, 1.0, 4, 1), (3, 1.0, 4, 64)]
    words = [b"radius"] * 3 + [b"gamma"] * 4 + [b"max_history"] * 3 + [b"flag"] * 2
    for setting, want in ((clip, want_on), (None, want_off)):
        hist = T.History(ctx, w, h)
        if setting is not None:
            hist.set_clip(**setting)
        for args, word in zip(bad, words):
            p = _lib.ClipParams(*args)
            assert L.tpt_history_set_clip(hist.handle, C.byref(p)) == 1, args
            assert word in L.tpt_last_error(), (args, L.tpt_last_error())
        st = _lib.ClipStats(-1.0, 77, 77)
        assert L.tpt_history_clip_stats(hist.handle, None) == 1 and b"out" in L.tpt_last_error()
        assert L.tpt_history_clip_stats(None, C.byref(st)) == 1 and (st.box_ms, st.boxed, st.clipped) == (-1.0, 77, 77)
        with pytest.raises(T.TPTError):
            hist.set_clip(radius=7)
        got = [call(pt, hist, cam, rad, aov, **params) for cam, (rad, aov) in zip(cams, frames)]
        hist.close()
        for a, b in zip(got[1][:3], want[1][:3]):
            assert np.array_equal(_bits(a), _bits(b))
        assert got[1][3]["clipped"] == want[1][3]["clipped"]
