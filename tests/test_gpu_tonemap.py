"""tpt_tonemap on the device against its definition in numpy (tests/tonemap_ref.py; DESIGN.md
section 5 "Tone mapping"): the histogram and the counts exactly, the exposure value, the adaptation
across calls, the float output, the bytes, bad values, its exact properties and its refusals.  The
frames are tests/tonemap_cases.py's, whose premises tests/test_tonemap_cpu.py checks without a GPU."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T

from tests.conftest import scene_path
from tests import tonemap_cases as K
from tests import tonemap_ref as R

pytestmark = pytest.mark.gpu

COMBOS = [(op, tr) for op in R.OPS for tr in R.TRANSFERS]
SIZE_IDS = ["%dx%d" % s for s in K.SIZES]

# The exposure value.  The device does the measurement in double and reports log2_avg and log2_scale
# as floats, so what is left is the rounding of a value below 16 in magnitude to float: at most
# 2^-21 = 4.8e-7 below 8.  Measured on MI355X over the 24 frames below (four cases, six sizes), the
# largest |gpu - ref| per case:
#   log_uniform  log2_avg 9.7e-8 (1x1)    log2_scale 4.0e-8 (1x1)      constant  1.2e-9 / 4.0e-9 at every size
#   planted      log2_avg 5.2e-8 (17x16)  log2_scale 1.80e-7 (1x1)     two_bins  1.28e-7 (1x1) / 5.4e-8 (1x1)
# and 5.4e-8 over the calls of the adaptation test.
EV_MEASURED_MAX = 1.8e-7
EV_BOUND = 10 * EV_MEASURED_MAX
assert EV_BOUND <= 1e-5

# The float output: tonemap_ref.BOUND is ten times the largest |gpu y - ref y| measured on MI355X.
# Per op x transfer, the maximum over the six sizes of `planted`, aliased or not (the same bits):
#   linear   none 2.98e-8   srgb 1.608e-7   gamma 8.60e-8
#   reinhard none 1.935e-7  srgb 2.075e-7   gamma 1.237e-7
#   aces     none 2.449e-7  srgb 2.442e-7   gamma 1.293e-7
# (with powf instead of the hardware's log2 and exp2 the six figures with a transfer function were
# 1.608e-7, 7.13e-8, 2.075e-7, 1.143e-7, 2.452e-7, 1.293e-7: the curve's error is not what bounds them)
Y_MEASURED_MAX = 2.449e-7
assert R.BOUND >= 10 * Y_MEASURED_MAX and R.BOUND <= 1e-5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def d(gpu_available):
    dev = T.Scene(scene_path("box")).copySceneToDevice(0)     # not built: the call takes only its device and stream
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def other(gpu_available):
    dev = T.Scene(scene_path("box")).copySceneToDevice(0)
    yield dev
    dev.close()


def _tm(d, frame, **kw):
    h, w = frame.shape[:2]
    st = {}
    res = T.PathTracer("", w, h, 0).tonemap(d, frame, stats=st, **kw)
    return res, st


# ---- the histogram and the exposure value ----

@pytest.mark.parametrize("size", K.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("name", K.NAMES)
def test_histogram_is_exact_and_the_exposure_value_close(d, name, size):
    w, h = size
    f = K.frame(name, w, h)
    hist, counted, dark, nonfinite = R.histogram(f)
    x = T.Exposure(d)
    assert (x.histogram() == 0).all()
    _, st = _tm(d, f, exposure=x, auto=True, ev=0.25)
    assert (st["counted"], st["dark"], st["nonfinite"]) == (counted, dark, nonfinite)
    assert st["counted"] + st["dark"] + st["nonfinite"] == w * h
    got = x.histogram()
    assert got.dtype == np.uint64 and np.array_equal(got, hist)
    log2_avg, log2_scale, _ = R.measure(hist, ev=0.25)
    e_avg, e_scale = abs(st["log2_avg"] - log2_avg), abs(st["log2_scale"] - log2_scale)
    print(f"{name} {w}x{h}: |log2_avg - ref| = {e_avg:.3e}, |log2_scale - ref| = {e_scale:.3e}, "
          f"hist {st['hist_ms']:.4f} ms, map {st['map_ms']:.4f} ms")
    assert e_avg <= EV_BOUND and e_scale <= EV_BOUND
    assert st["scale"] == pytest.approx(2.0 ** st["log2_scale"], rel=2.4e-7)   # (exp2f, to two ulp)
    assert st["hist_ms"] > 0.0 and st["map_ms"] > 0.0
    # a call without a handle measures the same frame the same way
    _, st0 = _tm(d, f, auto=True, ev=0.25)
    assert {k: st0[k] for k in ("log2_scale", "scale", "log2_avg", "counted", "dark", "nonfinite")} == \
           {k: st[k] for k in ("log2_scale", "scale", "log2_avg", "counted", "dark", "nonfinite")}
    x.close()


def test_the_trim_and_the_clamp(d):
    f = K.two_bins(37, 29)
    hist = R.histogram(f)[0]
    for kw in ({"p_low": 0.0, "p_high": 0.4}, {"p_low": 0.6, "p_high": 1.0}, {"p_low": 0.25, "p_high": 0.75},
               {"min_ev": -1.0, "max_ev": 1.5}, {"min_ev": 3.0, "max_ev": 3.0}, {"key": 0.5}):
        _, st = _tm(d, f, auto=True, **kw)
        log2_avg, log2_scale, _ = R.measure(hist, **kw)
        assert abs(st["log2_avg"] - log2_avg) <= EV_BOUND and abs(st["log2_scale"] - log2_scale) <= EV_BOUND, kw


# ---- adaptation ----

def test_adaptation_follows_the_rule_call_by_call(d):
    w, h = 37, 29
    frames = [K.constant(w, h, (0.1, 0.1, 0.1)), K.constant(w, h, (10.0, 10.0, 10.0)), K.constant(w, h, (10.0, 10.0, 10.0))]
    x = T.Exposure(d)
    worst = 0.0

    def run(f, s, **kw):
        nonlocal worst
        _, st = _tm(d, f, exposure=x, auto=True, rate=0.25, **kw)
        log2_avg, log2_scale, s = R.measure(R.histogram(f)[0], rate=0.25, state=s, **kw)
        worst = max(worst, abs(st["log2_scale"] - log2_scale))
        assert abs(st["log2_scale"] - log2_scale) <= EV_BOUND
        return s, st

    s = None
    targets = []
    for f in frames:
        s, st = run(f, s)
        targets.append(s)
    # the first call starts at its target; the next two move a quarter of the way each
    t0, t1 = R.measure(R.histogram(frames[0])[0])[2], R.measure(R.histogram(frames[1])[0])[2]
    assert targets[0] == t0 and targets[1] == pytest.approx(t0 + 0.25 * (t1 - t0), abs=1e-12)
    assert targets[2] == pytest.approx(targets[1] + 0.25 * (t1 - targets[1]), abs=1e-12)
    assert abs(t1 - t0) > 6.0                                  # (two decades apart: the steps are visible)
    # an all-black frame has no counted pixel and keeps the state, with and without ev
    _, st = _tm(d, K.black(w, h), exposure=x, auto=True, rate=0.25, ev=1.0)
    assert st["counted"] == 0 and st["dark"] == w * h and abs(st["log2_scale"] - (s + 1.0)) <= EV_BOUND
    s, _ = run(frames[0], s)                                   # ... and the next call moves on from it
    # without AUTO the handle is neither read nor written
    before = x.histogram()
    _, st = _tm(d, frames[1], exposure=x, ev=2.0)
    assert st["log2_scale"] == 2.0 and st["scale"] == 4.0 and st["hist_ms"] == 0.0 and st["counted"] == 0
    assert np.array_equal(x.histogram(), before)
    s, _ = run(frames[1], s)
    # a null handle never adapts: every call is at its target
    for f in frames[:2]:
        _, st = _tm(d, f, auto=True, rate=0.25)
        assert abs(st["log2_scale"] - R.measure(R.histogram(f)[0])[1]) <= EV_BOUND
    # reset starts over; an all-black frame on a fresh state gives scale 2^ev and still no state
    x.reset()
    _, st = _tm(d, K.black(w, h), exposure=x, auto=True, rate=0.25, ev=-1.0)
    assert st["log2_scale"] == -1.0 and st["scale"] == pytest.approx(0.5, rel=2.4e-7)
    s, _ = run(frames[1], None)
    assert s == t1
    print(f"adaptation: max |log2_scale - ref| = {worst:.3e}")
    x.close()


# ---- the float output ----

@pytest.mark.parametrize("op,transfer", COMBOS, ids=["%s-%s" % c for c in COMBOS])
def test_float_output_matches_the_reference(d, op, transfer):
    worst = 0.0
    for w, h in K.SIZES:
        f = K.planted(w, h)
        for auto in (False, True):
            kw = dict(op=op, transfer=transfer, auto=auto, ev=0.5, white=3.0, gamma=2.4)
            out, st = _tm(d, f, **kw)
            ref = R.map_frame(f, st["scale"], op, transfer, white=3.0, gamma=2.4)
            assert out.dtype == np.float32 and np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
            err = float(np.abs(out.astype(np.float64) - ref).max())
            worst = max(worst, err)
            assert err <= R.BOUND, (w, h, auto, err)
            # aliasing the input: the same bits
            buf = f.copy()
            res, st2 = _tm(d, buf, out=buf, **kw)
            assert res is buf and st2["scale"] == st["scale"] and np.array_equal(_bits(buf), _bits(out))
    print(f"{op} {transfer}: max |y - ref| = {worst:.3e}")


# ---- the bytes ----

@pytest.mark.parametrize("dither", [False, True], ids=["plain", "dither"])
@pytest.mark.parametrize("op,transfer", COMBOS, ids=["%s-%s" % c for c in COMBOS])
def test_bytes_match_the_reference(d, op, transfer, dither):
    for name in ("planted", "constant"):
        for w, h in K.SIZES:
            f = K.frame(name, w, h)
            fb = np.full((h, w, 4), 77, np.uint8)
            fb[..., 3] = np.arange(w, dtype=np.uint8)[None, :] * 3 + 1
            alpha = fb[..., 3].copy()
            res, st = _tm(d, f, bgra=fb, op=op, transfer=transfer, dither=dither)
            assert res is fb and st["scale"] == 1.0
            args = R.byte_args(R.map_frame(f, st["scale"], op, transfer), dither)
            want, near = R.to_bytes(args), R.near_boundary(args)
            got = fb[..., :3]
            assert np.array_equal(fb[..., 3], alpha)                               # alpha untouched
            assert (np.abs(got.astype(int) - want.astype(int)) <= 1).all()
            assert near.mean() <= 0.02, (name, w, h, near.mean())                  # never excludes more
            assert np.array_equal(got[~near], want[~near]), (name, w, h)


def test_bytes_and_floats_together_under_auto(d):
    f = K.log_uniform(131, 9)
    fb = np.full((9, 131, 4), 255, np.uint8)
    out = np.empty_like(f)
    res, st = _tm(d, f, out=out, bgra=fb, op="aces", transfer="srgb", auto=True, dither=True)
    assert res is out
    ref = R.map_frame(f, st["scale"], "aces", "srgb")
    assert np.abs(out.astype(np.float64) - ref).max() <= R.BOUND
    args = R.byte_args(ref, True)
    near = R.near_boundary(args)
    assert near.mean() <= 0.02 and np.array_equal(fb[..., :3][~near], R.to_bytes(args)[~near])
    assert (fb[..., 3] == 255).all()
    only, _ = _tm(d, f, bgra=np.full_like(fb, 255), op="aces", transfer="srgb", auto=True, dither=True)
    assert np.array_equal(only, fb)                                                # the float output changes no byte


# ---- bad values ----

@pytest.mark.parametrize("op", R.OPS)
def test_bad_values(d, op):
    """NaN and negatives map to 0, +inf to 255 under every op and transfer; nothing non-finite comes out."""
    f = np.array([[[np.nan, 0.5, -1.0], [np.inf, -np.inf, 0.25], [np.inf, np.inf, np.inf], [-0.0, np.nan, np.nan]]],
                 np.float32)
    for transfer in R.TRANSFERS:
        for ev in (0.0, 3.0, -3.0):
            fb = np.zeros((1, 4, 4), np.uint8)
            out = np.empty_like(f)
            _tm(d, f, out=out, bgra=fb, op=op, transfer=transfer, ev=ev)
            assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
            rgb = fb[0, :, 2::-1]
            assert rgb[0, 0] == 0 and rgb[0, 2] == 0 and out[0, 0, 0] == 0.0 and out[0, 0, 2] == 0.0
            assert rgb[1, 0] == 255 and rgb[1, 1] == 0 and out[0, 1, 0] >= 1.0 - R.BOUND
            assert (rgb[2] == 255).all() and (out[0, 2] >= 1.0 - R.BOUND).all()
            assert (rgb[3] == 0).all() and (out[0, 3] == 0.0).all()


# ---- properties ----

def test_two_calls_give_equal_bits(d):
    f = K.planted(131, 9)
    runs = []
    for _ in range(2):
        fb = np.full((9, 131, 4), 255, np.uint8)
        out, st = _tm(d, f, out=np.empty_like(f), bgra=fb, auto=True, dither=True)
        runs.append((_bits(out).copy(), fb.copy(), st["log2_scale"], st["log2_avg"]))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert runs[0][2:] == runs[1][2:]


def test_device_tensors_and_numpy_arrays_give_equal_bits(d):
    import torch
    w, h = 131, 9
    f = K.planted(w, h)
    fb = np.full((h, w, 4), 200, np.uint8)
    out, st = _tm(d, f, out=np.empty_like(f), bgra=fb, auto=True, op="aces")
    tf = torch.from_numpy(f.copy()).cuda()
    tout = torch.full((h * w * 3 + 64,), -7.0, dtype=torch.float32, device="cuda")
    tfb = torch.full((h * w * 4 + 64,), 200, dtype=torch.uint8, device="cuda")
    res, st2 = _tm(d, tf, out=tout[:h * w * 3].view(h, w, 3), bgra=tfb[:h * w * 4].view(h, w, 4), auto=True, op="aces")
    torch.cuda.synchronize()
    assert res.data_ptr() == tout.data_ptr()                                       # written in place
    assert np.array_equal(_bits(tout[:h * w * 3].cpu().numpy().reshape(h, w, 3)), _bits(out))
    assert np.array_equal(tfb[:h * w * 4].cpu().numpy().reshape(h, w, 4), fb)
    assert (tout[h * w * 3:] == -7.0).all() and (tfb[h * w * 4:] == 200).all()    # nothing past the end
    assert st2["scale"] == st["scale"] and st2["counted"] == st["counted"]
    assert np.array_equal(_bits(tf.cpu().numpy()), _bits(f))                       # the input is only read
    # the device input aliased
    _tm(d, tf, out=tf, auto=True, op="aces")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(tf.cpu().numpy()), _bits(out))


def test_out_is_written_in_place_and_nothing_past_its_end(d):
    w, h = 37, 29
    f = K.planted(w, h)
    big = np.full(w * h * 3 + 32, -7.0, np.float32)
    bytes_ = np.full(w * h * 4 + 32, 9, np.uint8)
    out = big[:w * h * 3].reshape(h, w, 3)
    res, _ = _tm(d, f, out=out, bgra=bytes_[:w * h * 4].reshape(h, w, 4))
    assert res is out and (out != -7.0).all()
    assert (big[w * h * 3:] == -7.0).all() and (bytes_[w * h * 4:] == 9).all()
    assert (bytes_[:w * h * 4].reshape(h, w, 4)[..., 3] == 9).all()


# ---- refusals ----

def _raw(d, x, w, h, rad, p, out, fb):
    return T.lib().tpt_tonemap(d.handle, x.handle if x is not None else None, w, h,
                               rad.ctypes.data if rad is not None else None, C.byref(p) if p is not None else None,
                               out.ctypes.data if out is not None else None, fb.ctypes.data if fb is not None else None,
                               None)


BAD_PARAMS = [("op", 3), ("op", -1), ("transfer", 3), ("transfer", -1), ("flags", 4), ("flags", 0x10 | 1),
              ("ev", np.nan), ("ev", np.inf), ("white", 0.0), ("white", -1.0), ("white", np.nan), ("gamma", 0.0),
              ("gamma", np.nan), ("key", 0.0), ("key", -0.18), ("key", np.nan), ("p_low", -0.1), ("p_low", 0.95),
              ("p_low", np.nan), ("p_high", 1.1), ("p_high", np.nan), ("p_high", 0.05), ("min_ev", 17.0),
              ("min_ev", np.nan), ("max_ev", np.nan), ("max_ev", -17.0), ("rate", 0.0), ("rate", 1.5), ("rate", np.nan)]


def test_every_refusal_leaves_the_outputs_and_the_state(d, other):
    w, h = 17, 16
    f = K.log_uniform(w, h).copy()
    bright = K.constant(w, h, (10.0, 10.0, 10.0))
    x, foreign = T.Exposure(d), T.Exposure(other)
    _, st = _tm(d, f, exposure=x, auto=True)                   # a state and a histogram to keep
    s = R.measure(R.histogram(f)[0])[2]
    hist = x.histogram()
    out = np.full((h, w, 3), -7.0, np.float32)
    fb = np.full((h, w, 4), 9, np.uint8)
    good = lambda: T._tonemap_params({"auto": True, "rate": 0.25})   # noqa: E731
    calls = []
    for field, value in BAD_PARAMS:
        p = good()
        setattr(p, field, value)
        calls.append((field, value, (d, x, w, h, bright, p, out, fb)))
    for size in ((0, h), (w, 0), (-1, h), (w, -5), (1048577, 1), (1, 1048577), (65536, 65536)):
        calls.append(("size", size, (d, x, size[0], size[1], bright, good(), out, fb)))
    calls.append(("input", None, (d, x, w, h, None, good(), out, fb)))
    calls.append(("params", None, (d, x, w, h, bright, None, out, fb)))
    calls.append(("outputs", None, (d, x, w, h, bright, good(), None, None)))
    calls.append(("exposure", "of another scene", (d, foreign, w, h, bright, good(), out, fb)))
    for what, value, args in calls:
        assert _raw(*args) == 1, (what, value)                 # TPT_ERR_INVALID_ARG
        assert T.lib().tpt_last_error()
        assert (out == -7.0).all() and (fb == 9).all(), (what, value)
    assert np.array_equal(x.histogram(), hist)
    assert (foreign.histogram() == 0).all()
    # the state is what the one good call left: the next call moves a quarter of the way from it
    _, st = _tm(d, bright, exposure=x, auto=True, rate=0.25)
    want = R.measure(R.histogram(bright)[0], rate=0.25, state=s)[1]
    assert abs(st["log2_scale"] - want) <= EV_BOUND
    with pytest.raises(T.TPTError):
        _tm(d, bright, exposure=foreign, auto=True)
    x.close()
    foreign.close()
