"""tpt_temporal: reprojection and accumulation across frames against a float64 numpy
restatement of its definition (tests/temporal_ref.py; DESIGN.md section 5
"Post-pass"), on feature buffers built analytically from three world-space patches."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import scene_path
from tests import temporal_ref as TR

pytestmark = pytest.mark.gpu

W, H = 37, 29                       # odd, no multiple of a tile or of a 64-pixel row segment
ASPECT = W / H
MOVE = (0.13, 0.05, 0.02)
CAMERAS = {"static": TR.camera(aspect=ASPECT), "translate": TR.camera(0.0, MOVE, aspect=ASPECT),
           "yaw_translate": TR.camera(1.5, MOVE, aspect=ASPECT), "yaw": TR.camera(2.0, aspect=ASPECT)}
THIRD = TR.camera(3.0, (0.26, 0.10, 0.04), aspect=ASPECT)
PARAMS = dict(alpha=0.1, depth_tol=0.1, normal_min=0.9, max_history=32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cam(c):
    return T.Camera(c["c2w"], c["vfov"], c["aspect"])


def frame(cam, seed):
    """Guides of the synthetic scene from `cam`, seeded random colours and albedo
    (1 on a miss, as tpt_render_aov writes it), one black-albedo pixel."""
    rng = np.random.default_rng(seed)
    aov = TR.synthetic_guides(cam, W, H)
    rad = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    alb = rng.uniform(0.2, 1.0, (H, W, 3)).astype(np.float32)
    alb[aov["material"] < 0] = 1.0
    assert aov["material"][20, 5] >= 0
    alb[20, 5] = 0.0                                       # demodulation divides by the floor 1e-3
    rad[20, 5] = 0.0
    aov["albedo"] = alb
    return rad, aov


@pytest.fixture(scope="module")
def ctx(gpu_available):
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0)                             # the scene supplies the device; it need not be built
    pt = T.PathTracer("", W, H, 0)
    yield d, pt
    d.close()


@pytest.fixture(scope="module")
def first():
    return frame(CAMERAS["static"], 101)


def run(pt, hist, cam, rad, aov, **kw):
    """One call; returns out, variance, history length, stats."""
    var = np.full((H, W), -3.0, np.float32)
    n = np.full((H, W), -3.0, np.float32)
    st = {}
    out = pt.temporal(hist, _cam(cam), rad, aov, variance=var, history_len=n, stats=st, **kw)
    return out, var, n, st


# Bound: the kernel's float32 reprojected coordinate and the
# reference's float64 one differ by at most 2^-14 px, which moves each of the four
# bilinear weights by that much, renormalised by wsum >= 1/16: 4 * 16 * 2^-14 = 4e-3 of
# the value range is the a-priori ceiling.  Measured on MI355X the maximum of
# max|gpu - ref| / max|ref| over colour, variance and history length, the eight
# two-frame cases and the three chains, is below; the asserted bound is ten times that
# and must stay under the ceiling.  The static cases measure float32 rounding (a single
# tap of weight 1): colour 4.5e-8 / 8.4e-8, variance 6.2e-7 (M2 - M1^2 cancels).  The
# moving cases: colour 1.1e-6 .. 2.9e-6, variance 1.3e-6 .. 3.0e-6, a chain's blended
# history lengths 3.6e-7.
CEILING = 4e-3
MEASURED_MAX = 2.952e-6             # variance, chain alpha 0.6 frame 3; the largest colour error is 2.940e-6
BOUND = 10 * MEASURED_MAX
assert BOUND <= CEILING


def compare(tag, got, ref, exact_n=True):
    """exact_n: the definition yields whole history lengths (two frames: 1 or 2), which
    must match exactly; a chain blends lengths over the taps, and those are bounded
    like the colours."""
    out, var, n, st = got
    dec = ref["decidable"]
    assert (~dec).mean() <= 0.01, f"{tag}: {(~dec).sum()} undecidable pixels"
    assert np.isfinite(out).all() and np.isfinite(var).all()
    assert np.array_equal((n > 1.0)[dec], ref["reprojected"][dec])     # the split: exact
    if dec.all():
        assert st["reprojected"] == int(ref["reprojected"].sum())
    errs = {}
    for name, g, r in (("colour", out, ref["out"]), ("variance", var, ref["variance"]),
                       ("history", n, ref["history_len"])):
        scale = np.abs(r).max()
        errs[name] = float(np.abs(g.astype(np.float64) - r)[dec].max() / (scale if scale > 0 else 1.0))
    print(f"{tag}: max|gpu - ref| / max|ref| colour {errs['colour']:.3e} variance {errs['variance']:.3e} "
          f"history {errs['history']:.3e}; reprojected {int(ref['reprojected'].sum())}, undecidable {(~dec).sum()}")
    if exact_n:
        assert np.array_equal(n[dec].astype(np.float64), ref["history_len"][dec])
    assert max(errs.values()) <= BOUND
    return errs


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_matches_numpy_reference(ctx, first, camera, demodulate):
    d, pt = ctx
    rad1, aov1 = first
    cam2 = CAMERAS[camera]
    rad2, aov2 = frame(cam2, 202)
    hist = T.History(d, W, H)
    kw = dict(PARAMS, demodulate=demodulate)
    g1 = run(pt, hist, CAMERAS["static"], rad1, aov1, **kw)
    g2 = run(pt, hist, cam2, rad2, aov2, **kw)
    hist.close()
    r1 = TR.temporal_ref(None, CAMERAS["static"], rad1, aov1, demodulate=demodulate, **PARAMS)
    r2 = TR.temporal_ref(r1["state"], cam2, rad2, aov2, demodulate=demodulate, **PARAMS)
    compare(f"{camera} demodulate {demodulate} frame 1", g1, r1)
    compare(f"{camera} demodulate {demodulate} frame 2", g2, r2)
    n = g2[2]
    if camera == "static":
        assert (n == 2.0).all() and g2[3]["reprojected"] == W * H
    else:                                                  # both branches and partial footprints are exercised
        assert (n == 1.0).any() and (n == 2.0).any()


@pytest.mark.parametrize("alpha,max_history", [(0.1, 32), (0.1, 2), (0.6, 32)])
def test_three_frame_chain(ctx, first, alpha, max_history):
    """Identity, yaw + translate, then further: N > 2 and blended history lengths, the
    cap (max_history 2), and both sides of max(alpha, 1 / N) (alpha 0.6 > 1 / 2)."""
    d, pt = ctx
    cams = [CAMERAS["static"], CAMERAS["yaw_translate"], THIRD]
    frames = [first, frame(cams[1], 202), frame(cams[2], 303)]
    params = dict(PARAMS, max_history=max_history, alpha=alpha)
    hist = T.History(d, W, H)
    state = None
    for k, (cam, (rad, aov)) in enumerate(zip(cams, frames)):
        got = run(pt, hist, cam, rad, aov, demodulate=True, **params)
        ref = TR.temporal_ref(state, cam, rad, aov, demodulate=True, **params)
        state = ref["state"]
        compare(f"chain alpha {alpha} max_history {max_history} frame {k + 1}", got, ref,
                exact_n=k < 2 or max_history == 2)
    hist.close()
    n = got[2]
    if max_history == 32:
        assert (n == 3.0).any() and ((n > 2.0) & (n < 3.0)).any()      # whole and blended history lengths
    else:
        assert n.max() == 2.0 and (n == 2.0).any()


def test_first_frame_and_reset(ctx, first):
    d, pt = ctx
    rad, aov = first
    floor_free = dict(aov, albedo=np.maximum(aov["albedo"], np.float32(1e-3)))
    hist = T.History(d, W, H)
    for demodulate, guides in ((False, aov), (True, floor_free)):
        for again in range(2):
            out, var, n, st = run(pt, hist, CAMERAS["static"], rad, guides, demodulate=demodulate, **PARAMS)
            assert np.array_equal(_bits(out), _bits(rad))
            assert (n == 1.0).all() and (var == 0.0).all() and st["reprojected"] == 0
            hist.reset()
    hist.close()


def test_static_camera_is_the_running_mean(ctx):
    d, pt = ctx
    cam = CAMERAS["static"]
    frames = [frame(cam, 400 + k) for k in range(4)]
    aov = frames[0][1]                                     # one albedo: the mean of the inputs is the mean of the colours
    hist = T.History(d, W, H)
    for rad, _ in frames:
        out, var, n, st = run(pt, hist, cam, rad, aov, alpha=1.0 / 64, depth_tol=0.1, normal_min=0.9,
                              max_history=64, demodulate=False)
    hist.close()
    stack = np.stack([r.astype(np.float64) for r, _ in frames])
    mean = stack.mean(0)
    lum = stack @ TR.LUMA
    assert (n == 4.0).all() and st["reprojected"] == W * H
    assert np.abs(out - mean).max() <= 1e-5 * np.abs(stack).max()
    assert np.abs(var - lum.var(0)).max() <= 1e-5 * (lum ** 2).max()


def test_rejection_is_exact(ctx, first):
    """Frame 1's colours changed on the near strip only: frame 2's output elsewhere
    cannot see them."""
    d, pt = ctx
    rad1, aov1 = first
    cam2 = CAMERAS["translate"]
    rad2, aov2 = frame(cam2, 202)
    other = rad1.copy()
    strip = aov1["material"] == 1
    other[strip] = np.random.default_rng(5).uniform(0.0, 2.0, (int(strip.sum()), 3)).astype(np.float32)
    outs = []
    for r1 in (rad1, other):
        hist = T.History(d, W, H)
        run(pt, hist, CAMERAS["static"], r1, aov1, **PARAMS)
        outs.append(run(pt, hist, cam2, rad2, aov2, **PARAMS)[0])
        hist.close()
    rest = aov2["material"] != 1
    assert np.array_equal(_bits(outs[0][rest]), _bits(outs[1][rest]))
    assert not np.array_equal(_bits(outs[0][~rest]), _bits(outs[1][~rest]))


def test_sky_follows_rotation(ctx, first):
    d, pt = ctx
    rad1, aov1 = first
    cam2 = CAMERAS["yaw"]
    rad2, aov2 = frame(cam2, 202)
    hist = T.History(d, W, H)
    run(pt, hist, CAMERAS["static"], rad1, aov1, **PARAMS)
    out, var, n, st = run(pt, hist, cam2, rad2, aov2, **PARAMS)
    hist.close()
    ref = TR.temporal_ref(TR.temporal_ref(None, CAMERAS["static"], rad1, aov1, demodulate=True, **PARAMS)["state"],
                          cam2, rad2, aov2, demodulate=True, **PARAMS)
    sky = (aov2["material"] < 0) & ref["reprojected"] & ref["decidable"]
    assert sky.sum() > 50                                  # most of the sky reprojects inside the frame
    assert (n[sky] == 2.0).all()


def test_device_tensors_and_in_place(ctx, first):
    import torch
    d, pt = ctx
    rad1, aov1 = first
    cam2 = CAMERAS["yaw_translate"]
    rad2, aov2 = frame(cam2, 202)
    hist = T.History(d, W, H)
    run(pt, hist, CAMERAS["static"], rad1, aov1, **PARAMS)
    ref = run(pt, hist, cam2, rad2, aov2, **PARAMS)
    dev = torch.device("cuda", 0)
    up = lambda a: {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
    hist.reset()
    t1, t2 = torch.from_numpy(rad1).to(dev), torch.from_numpy(rad2).to(dev)
    pt.temporal(hist, _cam(CAMERAS["static"]), t1, up(aov1), out=t1, **PARAMS)           # in place on the device
    assert np.array_equal(_bits(t1.cpu().numpy()), _bits(rad1))
    t_var, t_n = torch.zeros((H, W), device=dev), torch.zeros((H, W), device=dev)
    assert pt.temporal(hist, _cam(cam2), t2, up(aov2), out=t2, variance=t_var, history_len=t_n, **PARAMS) is t2
    for got, want in ((t2, ref[0]), (t_var, ref[1]), (t_n, ref[2])):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    hist.reset()                                           # in place in host memory
    b1, b2 = rad1.copy(), rad2.copy()
    pt.temporal(hist, _cam(CAMERAS["static"]), b1, aov1, out=b1, **PARAMS)
    assert pt.temporal(hist, _cam(cam2), b2, aov2, out=b2, **PARAMS) is b2
    assert np.array_equal(_bits(b2), _bits(ref[0]))
    hist.close()


def test_framebuffer_follows_copy_to_fb(ctx, first):
    d, pt = ctx
    rad1, aov1 = first
    rad2, aov2 = frame(CAMERAS["translate"], 202)
    hist = T.History(d, W, H)
    run(pt, hist, CAMERAS["static"], rad1, aov1, **PARAMS)
    fb = np.full((H, W, 4), 0x5A, np.uint8)
    out = pt.temporal(hist, _cam(CAMERAS["translate"]), rad2, aov2, framebuffer=fb, **PARAMS)
    hist.close()
    # Spectrum::toUChar (material.h:74-81): truncating clamp of c * 255 to [0, 255], float32
    x = out * np.float32(255.0)
    byte = np.maximum(np.minimum(x, np.float32(255.0)), np.float32(0.0)).astype(np.uint8)
    assert (out > 1.0).any()                               # the clamp is exercised
    assert np.array_equal(fb[..., :3], byte[::-1, :, ::-1])            # row 0 = top; B, G, R
    assert (fb[..., 3] == 0x5A).all()                      # alpha untouched


def test_deterministic_and_block_shapes_agree(ctx, first):
    """Two histories fed the same sequence agree bit for bit, and so does the
    16x16-tile launch (TPT_TEMPORAL_TILES) with the row-segment one."""
    d, pt = ctx
    cams = [CAMERAS["static"], CAMERAS["yaw_translate"], THIRD]
    frames = [first, frame(cams[1], 202), frame(cams[2], 303)]
    results = []
    for flags in (0, 0, _lib.TEMPORAL_TILES):
        hist = T.History(d, W, H)
        for cam, (rad, aov) in zip(cams, frames):
            got = run(pt, hist, cam, rad, aov, flags=flags, **PARAMS)
        hist.close()
        results.append(got)
    for other in results[1:]:
        for a, b in zip(results[0][:3], other[:3]):
            assert np.array_equal(_bits(a), _bits(b))
        assert other[3]["reprojected"] == results[0][3]["reprojected"]


def test_refusals(ctx, first):
    """Each bad argument returns TPT_ERR_INVALID_ARG, writes nothing and leaves the
    history as it was: the next valid call gives what an undisturbed history gives."""
    d, pt = ctx
    L = T.lib()
    rad1, aov1 = first
    cam2 = CAMERAS["yaw_translate"]
    rad2, aov2 = frame(cam2, 202)
    clean, hist = T.History(d, W, H), T.History(d, W, H)
    for h in (clean, hist):
        run(pt, h, CAMERAS["static"], rad1, aov1, **PARAMS)
    want = run(pt, clean, cam2, rad2, aov2, **PARAMS)
    clean.close()
    out = np.full((H, W, 3), -7.0, np.float32)
    var = np.full((H, W), -7.0, np.float32)
    n = np.full((H, W), -7.0, np.float32)
    cam = _cam(cam2).to_c()
    ok = (0.1, 0.1, 0.9, 32, 1)

    def call(guides=aov2, params=ok, handle=hist.handle, camera=C.byref(cam), rin=rad2.ctypes.data,
             rout=out.ctypes.data, no_guides=False, no_params=False):
        g = _lib.Aov(*[(guides[k].ctypes.data if guides.get(k) is not None else None)
                       for k in ("albedo", "normal", "depth")], None,
                     guides["material"].ctypes.data if guides.get("material") is not None else None)
        p = _lib.TemporalParams(*params)
        return L.tpt_temporal(handle, camera, rin, None if no_guides else C.byref(g),
                              None if no_params else C.byref(p), rout, var.ctypes.data, n.ctypes.data, None, None)

    def refused(word, **kw):
        assert call(**kw) == 1
        assert word in L.tpt_last_error(), L.tpt_last_error()

    refused(b"history", handle=None)
    refused(b"camera", camera=None)
    refused(b"radiance_in", rin=None)
    refused(b"guides", no_guides=True)
    refused(b"params", no_params=True)
    for missing in ("normal", "depth", "material"):
        refused(b"guides", guides={k: v for k, v in aov2.items() if k != missing})
    refused(b"albedo", guides={k: v for k, v in aov2.items() if k != "albedo"})
    assert call(guides={k: v for k, v in aov2.items() if k != "albedo"}, params=(0.1, 0.1, 0.9, 32, 0)) == 0
    hist.reset()                                           # that valid call moved the history: start it again
    run(pt, hist, CAMERAS["static"], rad1, aov1, **PARAMS)
    out[:], var[:], n[:] = -7.0, -7.0, -7.0
    for alpha in (0.0, -0.5, 1.5, float("nan")):
        refused(b"alpha", params=(alpha, 0.1, 0.9, 32, 1))
    for tol in (0.0, -1.0, float("nan")):
        refused(b"depth_tol", params=(0.1, tol, 0.9, 32, 1))
    for nm in (-1.5, 1.5, float("nan")):
        refused(b"normal_min", params=(0.1, 0.1, nm, 32, 1))
    for mh in (0, -1, 65537):
        refused(b"max_history", params=(0.1, 0.1, 0.9, mh, 1))
    refused(b"flag", params=(0.1, 0.1, 0.9, 32, 64))
    refused(b"output", rout=None)
    assert (out == -7.0).all() and (var == -7.0).all() and (n == -7.0).all()   # no refused call wrote anything
    got = run(pt, hist, cam2, rad2, aov2, **PARAMS)
    hist.close()
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(_bits(a), _bits(b))


def test_end_to_end_lowers_the_error(gpu_available):
    """box at 96x54: eight frames of 8 spp, seeds 1..8, the camera yawing 1 degree per
    frame, through the pass with the hosts' defaults.  The accumulated last frame is
    closer to a 2,048-spp frame at the last camera than that frame's 8 spp alone
    (the ratio is recorded in DESIGN.md, not asserted)."""
    w, h = 96, 54
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", w, h, 0)
    hist = T.History(d, w, h)
    noisy = np.zeros((h, w, 3), np.float32)
    n = np.zeros((h, w), np.float32)
    for k in range(8):
        cam = s.m_camera.yawed(1.0 * k)
        pt.doTrace(d, cam, None, 8, seed=k + 1, radiance=noisy)
        out = pt.temporal(hist, cam, noisy, pt.renderAOV(d, cam), history_len=n)
    truth = np.zeros((h, w, 3), np.float32)
    pt.doTrace(d, cam, None, 2048, seed=42, radiance=truth)
    hist.close()
    d.close()
    mse = lambda a: float(((a.astype(np.float64) - truth) ** 2).mean())
    print(f"MSE last 8-spp frame {mse(noisy):.5f}, temporal {mse(out):.5f}, ratio {mse(out) / mse(noisy):.4f}; "
          f"history >= 4 on {(n >= 4).mean():.3f} of the pixels")
    assert mse(out) < mse(noisy)
    assert (n >= 4).mean() > 0.5
