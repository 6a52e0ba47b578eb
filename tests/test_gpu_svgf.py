"""tpt_denoise_svgf: the variance-guided a-trous filter against a float64 numpy
restatement of its definition (tests/svgf_ref.py svgf_ref; DESIGN.md section 5
"Post-pass"), colour and variance."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import scene_path
from tests import svgf_ref as SR

pytestmark = pytest.mark.gpu

W, H = 37, 29                       # odd, no multiple of a tile; step 16 exceeds half of either side
SIG = dict(sigma_lum=4.0, sigma_normal=0.3, sigma_depth=0.05, min_history=4)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def synthetic(w=W, h=H, seed=11):
    """test_gpu_denoise.synthetic's frame, restated (its radiance and guides bit for
    bit: the same generator, seed and order of draws), and two planes more from a
    generator of their own: `variance` uniform in [0, 0.5] with one block of zeros
    (rows 10:14, columns 3:9 of 37 x 29, scaled as the other features are), and
    `history_len`, integers 1 ... 8 as float32, of which 1 ... 3 (three in eight) are
    shorter than min_history 4.  Returns (radiance, guides, variance, history_len)."""
    rng = np.random.default_rng(seed)
    rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    alb = rng.uniform(0.2, 1.0, (h, w, 3)).astype(np.float32)
    col = lambda c: c * w // 37
    row = lambda r: r * h // 29
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[:, :col(20)] = (0.0, 0.0, 1.0)
    nrm[:, col(20):] = (0.6, 0.0, 0.8)
    x = np.arange(w, dtype=np.float32)[None, :]
    y = np.arange(h, dtype=np.float32)[:, None]
    z = (2.0 + 0.01 * x + np.where(y >= row(15), 1.5, 0.0)).astype(np.float32)
    nrm[row(3):row(9), col(25):col(33)] = 0.0
    z[row(3):row(9), col(25):col(33)] = 0.0
    alb[row(3):row(9), col(25):col(33)] = 1.0
    if w * h > 1:
        alb[row(20), col(5)] = 0.0                         # demodulation divides by the floor 1e-3
        rad[row(20), col(5)] = 0.0
    rng2 = np.random.default_rng(seed + 1000)
    var = rng2.uniform(0.0, 0.5, (h, w)).astype(np.float32)
    var[row(10):row(14), col(3):col(9)] = 0.0
    hist = rng2.integers(1, 9, (h, w)).astype(np.float32)
    return rad, {"albedo": alb, "normal": nrm, "depth": z}, var, hist


# (W x H, iterations) beyond the 37 x 29 frame, as test_gpu_denoise's: 131 x 9 is three
# row-segment blocks of the direct kernel and nine tile columns, the last ones partial;
# 65 x 5 with 8 iterations has steps beyond the frame; 16 x 16 is exactly one tile, its
# LDS halos all outside the frame; 17 x 16 adds a tile of one column; 2 x 3 and 1 x 1 are
# smaller than every halo.
NEW_CASES = [((131, 9), 5), ((65, 5), 8), ((16, 16), 5), ((17, 16), 3), ((2, 3), 8), ((1, 1), 8)]


@pytest.fixture(scope="module")
def ctx(gpu_available):
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    yield d, pt, synthetic()
    d.close()


_REFS = {}


def reference(size, iterations, demodulate, mode="both"):
    """svgf_ref of the synthetic frame, computed once per case."""
    key = (size, iterations, demodulate, mode)
    if key not in _REFS:
        rad, aov, var, hist = synthetic(*size)
        _REFS[key] = SR.svgf_ref(rad, aov["albedo"], aov["normal"], aov["depth"], var if mode != "neither" else None,
                                 hist if mode == "both" else None, iterations=iterations, demodulate=demodulate, **SIG)
    return _REFS[key]


def run(d, pt, frame, mode="both", **kw):
    """One call: (out, variance_out, stats)."""
    rad, aov, var, hist = frame
    vout = np.full(var.shape, -7.0, np.float32)
    st = {}
    out = pt.denoiseSVGF(d, rad, aov, var if mode != "neither" else None, hist if mode == "both" else None,
                         variance_out=vout, stats=st, **dict(SIG, **kw))
    return out, vout, st


def errors(out, vout, ref):
    """(max |colour - ref| / max|c|, max |variance - ref| / max v), the bounds' measures."""
    ec = np.abs(out.astype(np.float64) - ref["out"]).max() / np.abs(ref["out"]).max()
    vmax = ref["variance"].max()
    ev = np.abs(vout.astype(np.float64) - ref["variance"]).max() / (vmax if vmax > 0 else 1.0)
    return ec, ev


# Bounds.  A priori: each colour output is a weighted mean whose weights carry a few ulp
# of exp and argument error, ~1e-6 max|c| per iteration (test_gpu_denoise.py's
# derivation), so at most 1e-4 of max|c|; the variance's weights enter squared, which
# doubles their relative error: 2e-4 of max v.  The asserted bounds are ten times the
# maximum measured on MI355X over every case of this file (both kernels give the same
# bits), and have to stay under those ceilings.  Measured, colour / variance:
#   37 x 29, iterations 0 / 1 / 3 / 5   0, 2.1e-7, 1.1e-7, 1.5e-7 / 1.3e-6, 8.0e-7, 2.8e-7, 2.8e-7
#   the same, demodulated               0, 2.9e-7, 1.2e-7, 1.5e-7 / 3.1e-6, 2.1e-6, 4.1e-7, 1.5e-7
#   131 x 9 (5)    1.6e-7, 2.2e-7 / 2.9e-7, 2.6e-6      17 x 16 (3)   9.8e-8, 3.0e-7 / 1.8e-7, 1.0e-6
#   65 x 5 (8)     1.7e-7, 1.3e-7 / 4.2e-7, 2.5e-7      2 x 3 (8)     3.3e-8, 5.8e-8 / 7.1e-8, 8.2e-8
#   16 x 16 (5)    1.4e-7, 1.1e-7 / 2.5e-7, 6.5e-7      1 x 1 (8)     0 / 0 (the output is the input)
#   variance only (3)   1.2e-7, 2.0e-7 / 3.0e-7, 5.3e-7      neither (3)   1.0e-7, 1.1e-7 / 3.2e-7, 7.7e-7
# The variance's maximum is the spatial estimate itself (iterations 0): a difference of
# two float32 moments, where the reference works in float64.
MEASURED_MAX = {"colour": 2.952e-7,                        # 17 x 16, 3 iterations, demodulated
                "variance": 3.104e-6}                      # 37 x 29, iterations 0, demodulated
BOUND = {k: 10 * v for k, v in MEASURED_MAX.items()}
assert BOUND["colour"] <= 1e-4 and BOUND["variance"] <= 2e-4


def check(out, vout, st, ref, what):
    ec, ev = errors(out, vout, ref)
    print(f"{what}: max |gpu - ref| colour {ec:.3e} of max|c|, variance {ev:.3e} of max v, "
          f"estimated {st['estimated']} (reference {ref['estimated']})")
    assert np.isfinite(out).all() and np.isfinite(vout).all()
    assert ec <= BOUND["colour"]
    assert ev <= BOUND["variance"]
    assert st["estimated"] == ref["estimated"]


@pytest.mark.parametrize("flags", [0, _lib.SVGF_DIRECT], ids=["lds", "direct"])
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_matches_numpy_reference(ctx, iterations, demodulate, flags):
    d, pt, frame = ctx
    out, vout, st = run(d, pt, frame, iterations=iterations, demodulate=demodulate, flags=flags)
    ref = reference((W, H), iterations, demodulate)
    check(out, vout, st, ref, f"iterations {iterations} demodulate {demodulate} flags {flags}")
    assert 0.33 <= ref["estimated"] / (W * H) <= 0.40       # the spatial estimate has its share of the frame
    assert np.abs(out.astype(np.float64) - frame[0]).max() > 0.05 * np.abs(ref["out"]).max()   # it filtered


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("size,iterations", NEW_CASES, ids=[f"{w}x{h}-{i}" for (w, h), i in NEW_CASES])
def test_other_sizes_match_numpy_reference(ctx, size, iterations, demodulate):
    """Frames of several blocks, of exactly one tile, and smaller than a tile or its
    halos; up to the 8 iterations the call accepts.  Both kernels against the
    reference, and against each other bit for bit."""
    d = ctx[0]
    w, h = size
    pt = T.PathTracer("", w, h, 0)
    frame = synthetic(w, h)
    ref = reference(size, iterations, demodulate)
    assert np.isfinite(ref["out"]).all() and np.isfinite(ref["variance"]).all()
    got = []
    for flags in (0, _lib.SVGF_DIRECT):
        out, vout, st = run(d, pt, frame, iterations=iterations, demodulate=demodulate, flags=flags)
        check(out, vout, st, ref, f"{w} x {h} iterations {iterations} demodulate {demodulate} flags {flags}")
        got.append((out, vout))
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("mode", ["both", "variance", "neither"])
def test_input_modes(ctx, mode, demodulate):
    """Variance and history lengths; a variance alone (every history long: no estimate);
    neither (every pixel takes the estimate with N = 1)."""
    d, pt, frame = ctx
    out, vout, st = run(d, pt, frame, mode, iterations=3, demodulate=demodulate)
    ref = reference((W, H), 3, demodulate, mode)
    check(out, vout, st, ref, f"mode {mode} demodulate {demodulate}")
    assert ref["estimated"] == {"variance": 0, "neither": W * H}.get(mode, ref["estimated"])


def test_lds_and_direct_kernels_agree_bit_for_bit(ctx):
    d, pt, frame = ctx
    a = run(d, pt, frame, iterations=5)
    b = run(d, pt, frame, iterations=5, flags=_lib.SVGF_DIRECT)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_deterministic(ctx):
    d, pt, frame = ctx
    a = run(d, pt, frame, iterations=5)
    b = run(d, pt, frame, iterations=5)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert a[2]["estimated"] == b[2]["estimated"]


def test_counter_slots_wrap(ctx):
    """257 x 241 is 17 x 16 = 272 tiles over the 256 counter slots, every pixel short."""
    d = ctx[0]
    w, h = 257, 241
    rad, aov, _, _ = synthetic(w, h)
    st = {}
    T.PathTracer("", w, h, 0).denoiseSVGF(d, rad, aov, iterations=1, stats=st, **SIG)
    assert st["estimated"] == w * h


def test_no_short_pixel_takes_the_early_exit(ctx):
    """Every history long: no estimate, and the bits of a call without history lengths,
    which does not launch the estimate kernel at all."""
    d, pt, (rad, aov, var, hist) = ctx
    long_ = np.full_like(hist, 8.0)
    a = run(d, pt, (rad, aov, var, long_), iterations=3)
    b = run(d, pt, (rad, aov, var, hist), "variance", iterations=3)
    assert a[2]["estimated"] == 0 and b[2]["estimated"] == 0
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_constant_image_stays_constant(ctx):
    d, pt, (rad, aov, var, hist) = ctx
    const = np.full((H, W, 3), 0.7371, np.float32)
    out, vout, _ = run(d, pt, (const, aov, var, hist), iterations=5, demodulate=False)
    assert np.array_equal(_bits(out), _bits(const))        # exactly
    short = hist < SIG["min_history"]
    out, vout, _ = run(d, pt, (const, aov, var, hist), iterations=0, demodulate=False)
    assert (vout[short] == 0.0).all()                      # a constant window has no variance
    flat = dict(aov, albedo=np.full((H, W, 3), 0.35, np.float32))       # demodulated: constant too
    out, _, _ = run(d, pt, (const, flat, var, hist), iterations=5, demodulate=True)
    assert np.abs(out.astype(np.float64) / 0.7371 - 1.0).max() <= 1e-6


@pytest.mark.parametrize("demodulate", [False, True])
def test_zero_iterations(ctx, demodulate):
    """The colour is the input bit for bit (no demodulation round trip), the variance v0."""
    d, pt, frame = ctx
    out, vout, st = run(d, pt, frame, iterations=0, demodulate=demodulate)
    assert np.array_equal(_bits(out), _bits(frame[0]))
    ref = reference((W, H), 0, demodulate)
    check(out, vout, st, ref, f"iterations 0 demodulate {demodulate}")
    keep = ~ref["short"]
    assert np.array_equal(_bits(vout[keep]), _bits(frame[2][keep]))    # a long history keeps its variance


def test_in_place(ctx):
    d, pt, (rad, aov, var, hist) = ctx
    ref = run(d, pt, (rad, aov, var, hist), iterations=3)
    buf, vbuf = rad.copy(), var.copy()
    assert pt.denoiseSVGF(d, buf, aov, vbuf, hist, iterations=3, out=buf, variance_out=vbuf, **SIG) is buf
    assert np.array_equal(_bits(buf), _bits(ref[0])) and np.array_equal(_bits(vbuf), _bits(ref[1]))


def test_device_tensors(ctx):
    import torch
    d, pt, (rad, aov, var, hist) = ctx
    ref = run(d, pt, (rad, aov, var, hist), iterations=3)
    dev = torch.device("cuda", 0)
    t_rad, t_var, t_hist = (torch.from_numpy(a).to(dev) for a in (rad, var, hist))
    t_aov = {k: torch.from_numpy(v).to(dev) for k, v in aov.items()}
    t_out, t_vout = torch.zeros((H, W, 3), device=dev), torch.zeros((H, W), device=dev)
    st = {}
    pt.denoiseSVGF(d, t_rad, t_aov, t_var, t_hist, iterations=3, out=t_out, variance_out=t_vout, stats=st, **SIG)
    assert np.array_equal(_bits(t_out.cpu().numpy()), _bits(ref[0]))
    assert np.array_equal(_bits(t_vout.cpu().numpy()), _bits(ref[1]))
    assert st["estimated"] == ref[2]["estimated"]
    pt.denoiseSVGF(d, t_rad, t_aov, t_var, t_hist, iterations=3, out=t_rad, variance_out=t_var, **SIG)   # in place
    assert np.array_equal(_bits(t_rad.cpu().numpy()), _bits(ref[0]))
    assert np.array_equal(_bits(t_var.cpu().numpy()), _bits(ref[1]))


@pytest.mark.parametrize("size", [(131, 9), (17, 16)])
@pytest.mark.parametrize("flags", [0, _lib.SVGF_DIRECT], ids=["lds", "direct"])
def test_nothing_is_written_past_the_end(ctx, size, flags):
    """The outputs are the first H rows of device tensors one row longer: the extra row
    keeps its sentinel, and no sentinel survives inside."""
    import torch
    d = ctx[0]
    w, h = size
    rad, aov, var, hist = synthetic(w, h)
    pt = T.PathTracer("", w, h, 0)
    want = run(d, pt, (rad, aov, var, hist), iterations=3, flags=flags)
    dev = torch.device("cuda", 0)
    whole, vwhole = torch.full((h + 1, w, 3), -7.0, device=dev), torch.full((h + 1, w), -7.0, device=dev)
    t_aov = {k: torch.from_numpy(v).to(dev) for k, v in aov.items()}
    pt.denoiseSVGF(d, torch.from_numpy(rad).to(dev), t_aov, torch.from_numpy(var).to(dev),
                   torch.from_numpy(hist).to(dev), iterations=3, out=whole[:h], variance_out=vwhole[:h], flags=flags,
                   **SIG)
    got, vgot = whole.cpu().numpy(), vwhole.cpu().numpy()
    assert (got[h] == -7.0).all() and (vgot[h] == -7.0).all()
    assert not (got[:h] == -7.0).any() and not (vgot[:h] == -7.0).any()
    assert np.array_equal(_bits(got[:h]), _bits(want[0])) and np.array_equal(_bits(vgot[:h]), _bits(want[1]))


def test_framebuffer_follows_copy_to_fb(ctx):
    d, pt, (rad, aov, var, hist) = ctx
    fb = np.full((H, W, 4), 0x5A, np.uint8)
    out = pt.denoiseSVGF(d, rad, aov, var, hist, iterations=2, framebuffer=fb, **SIG)
    # Spectrum::toUChar (material.h:74-81): truncating clamp of c * 255 to [0, 255], float32
    x = out * np.float32(255.0)
    byte = np.maximum(np.minimum(x, np.float32(255.0)), np.float32(0.0)).astype(np.uint8)
    assert (out > 1.0).any()                               # the clamp is exercised
    assert np.array_equal(fb[..., :3], byte[::-1, :, ::-1])            # row 0 = top; B, G, R
    assert (fb[..., 3] == 0x5A).all()                      # alpha untouched


def test_refusals(ctx):
    d, pt, (rad, aov, var, hist) = ctx
    L = T.lib()
    out = np.full((H, W, 3), -7.0, np.float32)
    vout = np.full((H, W), -7.0, np.float32)
    fb = np.full((H, W, 4), 0x5A, np.uint8)
    ok = (3, 4.0, 0.3, 0.05, 4, 1)

    def call(params=ok, guides=aov, scene=d.handle, radiance=rad, variance=var, history=hist, size=(W, H),
             outputs=(out, fb), null_guides=False, null_params=False):
        g = _lib.Aov(*[(guides[k].ctypes.data if guides.get(k) is not None else None)
                       for k in ("albedo", "normal", "depth")], None, None)
        p = _lib.SvgfParams(*params)
        ptr = lambda a: a.ctypes.data if a is not None else None
        return L.tpt_denoise_svgf(scene, size[0], size[1], ptr(radiance), None if null_guides else C.byref(g),
                                  ptr(variance), ptr(history), None if null_params else C.byref(p),
                                  ptr(outputs[0]), vout.ctypes.data, ptr(outputs[1]), None)

    def refused(word, **kw):
        assert call(**kw) == 1                             # TPT_ERR_INVALID_ARG
        assert word in L.tpt_last_error(), (kw, L.tpt_last_error())

    refused(b"scene", scene=None)
    refused(b"radiance_in", radiance=None)
    refused(b"guides", null_guides=True)
    refused(b"params", null_params=True)
    for missing in ("normal", "depth", "albedo"):
        refused(b"guides", guides={k: v for k, v in aov.items() if k != missing})
    assert call(params=(3, 4.0, 0.3, 0.05, 4, 0), guides={k: v for k, v in aov.items() if k != "albedo"}) == 0
    out[:], vout[:], fb[:] = -7.0, -7.0, 0x5A              # (albedo is needed under DEMODULATE only)
    refused(b"history_len_in", variance=None)
    refused(b"width", size=(0, H))
    refused(b"height", size=(W, -1))
    refused(b"iterations", params=(9, 4.0, 0.3, 0.05, 4, 1))
    refused(b"iterations", params=(-1, 4.0, 0.3, 0.05, 4, 1))
    for bad in ((3, 0.0, 0.3, 0.05, 4, 1), (3, 4.0, -0.3, 0.05, 4, 1), (3, 4.0, 0.3, float("nan"), 4, 1)):
        refused(b"sigma", params=bad)
    refused(b"min_history", params=(3, 4.0, 0.3, 0.05, 0, 1))
    refused(b"min_history", params=(3, 4.0, 0.3, 0.05, 65537, 1))
    refused(b"flags", params=(3, 4.0, 0.3, 0.05, 4, 64))
    refused(b"radiance_out", outputs=(None, None))
    assert (out == -7.0).all() and (vout == -7.0).all() and (fb == 0x5A).all()   # no refused call wrote anything
    assert call() == 0
    assert not (out == -7.0).any() and not (vout == -7.0).any()


def _read_pfm(path, w, h):
    raw = open(path, "rb").read()
    assert raw.startswith(b"PF\n%d %d\n-1.0\n" % (w, h))
    return np.frombuffer(raw[-w * h * 12:], np.float32).reshape(h, w, 3)


@pytest.mark.parametrize("temporal", [True, False])
def test_cli_writes_the_filtered_frame(gpu_available, tmp_path, temporal):
    """tpt_render --svgf, alone and with --temporal and --denoise: <out>_svgf.pfm / .ppm is
    denoiseSVGF at the hosts' defaults of the frame the CLI filtered."""
    import os
    import subprocess
    from tests.conftest import ROOT
    w, h = 48, 27
    out = str(tmp_path / "f")
    cmd = [os.path.join(ROOT, "tinypathtracer_amd", "tpt_render"), scene_path("box"), "--width", str(w), "--height",
           str(h), "--spp", "4", "--seed", "7", "--out", out, "--svgf"]
    if temporal:
        cmd += ["--frames", "3", "--yaw", "1", "--temporal", "--denoise"]
    subprocess.run(cmd, check=True, capture_output=True, timeout=120)
    names = {"f.ppm", "f.pfm", "f_svgf.pfm", "f_svgf.ppm"}
    if temporal:
        names |= {"f_temporal.pfm", "f_temporal.ppm", "f_denoised.pfm", "f_denoised.ppm"}
    assert {p.name for p in tmp_path.iterdir()} == names
    got = _read_pfm(out + "_svgf.pfm", w, h)
    src = _read_pfm(out + ("_temporal.pfm" if temporal else ".pfm"), w, h)
    assert np.isfinite(got).all() and not np.array_equal(got, src)
    if not temporal:                                       # the spatial estimate alone: reproducible from the frame
        s = T.Scene(scene_path("box"))
        d = s.copySceneToDevice(0).build()
        pt = T.PathTracer("", w, h, 0)
        want = pt.denoiseSVGF(d, src.copy(), pt.renderAOV(d, s.m_camera))
        d.close()
        assert np.array_equal(_bits(got), _bits(want))


def test_end_to_end_lowers_the_error(gpu_available):
    """box at 96x54: eight frames of 8 spp, seeds 1..8, the camera yawing 1 degree per
    frame, through tpt_temporal with the hosts' defaults
    (test_gpu_temporal.test_end_to_end_lowers_the_error's setup), then denoiseSVGF with
    its defaults by that pass's variance and history length.  The filtered frame is
    closer to a 2,048-spp frame at the last camera than its input (the MSEs are
    recorded in DESIGN.md, not asserted)."""
    w, h = 96, 54
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", w, h, 0)
    hist = T.History(d, w, h)
    noisy = np.zeros((h, w, 3), np.float32)
    var, n = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    for k in range(8):
        cam = s.m_camera.yawed(1.0 * k)
        pt.doTrace(d, cam, None, 8, seed=k + 1, radiance=noisy)
        aov = pt.renderAOV(d, cam)
        acc = pt.temporal(hist, cam, noisy, aov, variance=var, history_len=n)
    st = {}
    clean = pt.denoiseSVGF(d, acc, aov, var, n, stats=st)  # the host's defaults
    truth = np.zeros((h, w, 3), np.float32)
    pt.doTrace(d, cam, None, 2048, seed=42, radiance=truth)
    hist.close()
    d.close()
    mse = lambda a: float(((a.astype(np.float64) - truth) ** 2).mean())
    print(f"MSE last 8-spp frame {mse(noisy):.5f}, temporal {mse(acc):.5f}, svgf {mse(clean):.5f}, "
          f"ratio svgf / temporal {mse(clean) / mse(acc):.4f}; estimated {st['estimated']} of {w * h}")
    assert mse(clean) < mse(acc)
