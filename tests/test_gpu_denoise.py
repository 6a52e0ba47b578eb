"""tpt_denoise: the a-trous filter against a float64 numpy restatement of its
definition (tests/post_ref.py atrous_ref; DESIGN.md section 5 "Post-pass")."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import scene_path
from tests import post_ref as R

pytestmark = pytest.mark.gpu

W, H = 37, 29                       # odd, no multiple of a tile; step 16 exceeds half of either side
SIG = dict(sigma_color=4.0, sigma_normal=0.3, sigma_depth=0.05)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def synthetic(w=W, h=H, seed=11):
    """Seeded random colour; normals in two regions; depth a ramp with a step; a
    block of miss pixels (normal 0, depth 0, albedo 1); one black-albedo pixel.  The
    features sit where they sit at 37 x 29 (columns 20 and 25:33 of 37, rows 15, 3:9
    and 20 of 29), scaled to the frame and rounded down; a frame too small for one
    goes without it: the miss block where its rows or columns round to none, one
    normal region in a single column, no depth step in a single row, and no black
    pixel in a frame of one pixel."""
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
    return rad, {"albedo": alb, "normal": nrm, "depth": z}


# (W x H, iterations) beyond the 37 x 29 frame: 131 x 9 is three x-blocks of k_atrous and
# nine tile columns, the last ones partial; 65 x 5 with 8 iterations has steps 32 to
# 128 beyond the frame and a k_atrous block that holds one pixel column; 16 x 16 is
# exactly one tile, its LDS halo all outside the frame; 17 x 16 adds a tile of one
# column; 2 x 3 and 1 x 1 are smaller than every halo.
NEW_CASES = [((131, 9), 5), ((65, 5), 8), ((16, 16), 5), ((17, 16), 3), ((2, 3), 8), ((1, 1), 8)]
NEW_SIZES = [size for size, _ in NEW_CASES]


@pytest.fixture(scope="module")
def ctx(gpu_available):
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    rad, aov = synthetic()
    yield s, d, pt, rad, aov
    d.close()


# Bound: each output is a weighted mean whose weights carry a few ulp of exp and
# argument error, at most ~1e-6 max|c| per iteration, so 1e-4 would cover five
# iterations and the hardware's approximate exp.  Measured on MI355X the maximum
# over the six cases is far lower (the kernel keeps the mean as c(p) + sum w dc /
# sum w, so weight errors scale with the colour differences, not the colours), and
# the bound is ten times that measurement.  max|c| is taken of the output-space
# reference, which is never larger than the demodulated colours'.
MEASURED_MAX = 2.294e-7             # iterations 1, no demodulation; the others 8.8e-8 .. 2.2e-7
BOUND = 10 * MEASURED_MAX


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_matches_numpy_reference(ctx, iterations, demodulate):
    s, d, pt, rad, aov = ctx
    out = pt.denoise(d, rad, aov, iterations=iterations, demodulate=demodulate, **SIG)
    ref = R.atrous_ref(rad, aov["albedo"], aov["normal"], aov["depth"], iterations, SIG["sigma_color"],
                       SIG["sigma_normal"], SIG["sigma_depth"], demodulate)
    scale = np.abs(ref).max()
    err = np.abs(out.astype(np.float64) - ref).max() / scale
    print(f"iterations {iterations} demodulate {demodulate}: max |gpu - ref| / max|c| = {err:.3e}")
    assert np.isfinite(out).all()
    assert err <= BOUND
    assert np.abs(out.astype(np.float64) - rad).max() > 0.05 * scale   # it filtered


def test_lds_and_direct_kernels_agree_bit_for_bit(ctx):
    s, d, pt, rad, aov = ctx
    a = pt.denoise(d, rad, aov, iterations=3, **SIG)
    b = pt.denoise(d, rad, aov, iterations=3, flags=_lib.DENOISE_DIRECT, **SIG)
    assert np.array_equal(_bits(a), _bits(b))


# The new sizes' own measurement, taken as MEASURED_MAX was and with the same margin;
# it has to stay below the allowance derived above, about 2e-5 per iteration: 1e-4 at
# five iterations, 1.6e-4 at eight.
# Measured on MI355X, without / with demodulation, the same under both kernels:
#   131 x 9, 5 iterations   1.08e-7 / 1.34e-7      17 x 16, 3 iterations   9.2e-8 / 1.14e-7
#   65 x 5, 8 iterations    1.49e-7 / 2.15e-7      2 x 3, 8 iterations     4.5e-8 / 6.0e-8
#   16 x 16, 5 iterations   1.29e-7 / 1.34e-7      1 x 1, 8 iterations     0 (the output is the input)
MEASURED_MAX_NEW = 2.151e-7         # 65 x 5, 8 iterations, demodulation
BOUND_NEW = 10 * MEASURED_MAX_NEW
assert BOUND_NEW <= 1e-4


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("size,iterations", NEW_CASES, ids=[f"{w}x{h}-{i}" for (w, h), i in NEW_CASES])
def test_other_sizes_match_numpy_reference(ctx, size, iterations, demodulate):
    """Frames of several blocks, of exactly one tile, and smaller than a tile or its
    halo; up to the 8 iterations the call accepts.  Both kernels against the
    reference, and against each other bit for bit."""
    s, d, _, _, _ = ctx
    w, h = size
    pt = T.PathTracer("", w, h, 0)
    rad, aov = synthetic(w, h, 11)
    ref = R.atrous_ref(rad, aov["albedo"], aov["normal"], aov["depth"], iterations, SIG["sigma_color"],
                       SIG["sigma_normal"], SIG["sigma_depth"], demodulate)
    assert np.isfinite(ref).all()
    scale = np.abs(ref).max()
    outs = []
    for flags in (0, _lib.DENOISE_DIRECT):
        out = pt.denoise(d, rad, aov, iterations=iterations, demodulate=demodulate, flags=flags, **SIG)
        err = np.abs(out.astype(np.float64) - ref).max() / scale
        print(f"{w} x {h} iterations {iterations} demodulate {demodulate} flags {flags}: "
              f"max |gpu - ref| / max|c| = {err:.3e}")
        assert np.isfinite(out).all()
        assert err <= BOUND_NEW
        if w >= 5 or h >= 5:
            assert np.abs(out.astype(np.float64) - rad).max() > 0.05 * scale   # it filtered
        outs.append(out)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    if (w, h) == (1, 1):                                   # its only tap is itself
        assert np.abs(outs[0].astype(np.float64) - rad).max() <= BOUND_NEW * scale


@pytest.mark.parametrize("size", [(131, 9), (17, 16)])
@pytest.mark.parametrize("flags", [0, _lib.DENOISE_DIRECT])
def test_nothing_is_written_past_the_end(ctx, size, flags):
    """`out` is the first H rows of a device tensor one row longer: the extra row keeps
    its sentinel, and no sentinel survives inside."""
    import torch
    s, d, _, _, _ = ctx
    w, h = size
    rad, aov = synthetic(w, h, 11)
    dev = torch.device("cuda", 0)
    whole = torch.full((h + 1, w, 3), -7.0, device=dev)
    out = whole[:h]
    t_aov = {k: torch.from_numpy(v).to(dev) for k, v in aov.items()}
    want = T.PathTracer("", w, h, 0).denoise(d, rad, aov, iterations=3, flags=flags, **SIG)
    assert T.PathTracer("", w, h, 0).denoise(d, torch.from_numpy(rad).to(dev), t_aov, iterations=3, out=out,
                                             flags=flags, **SIG) is out
    got = whole.cpu().numpy()
    assert (got[h] == -7.0).all()
    assert not (got[:h] == -7.0).any()
    assert np.array_equal(_bits(got[:h]), _bits(want))


def test_constant_image_stays_constant(ctx):
    s, d, pt, rad, aov = ctx
    const = np.full((H, W, 3), 0.7371, np.float32)
    out = pt.denoise(d, const, aov, iterations=5, demodulate=False, **SIG)
    assert np.abs(out.astype(np.float64) / 0.7371 - 1.0).max() <= 1e-6
    flat = dict(aov, albedo=np.full((H, W, 3), 0.35, np.float32))       # demodulated: constant too
    out = pt.denoise(d, const, flat, iterations=5, demodulate=True, **SIG)
    assert np.abs(out.astype(np.float64) / 0.7371 - 1.0).max() <= 1e-6


def test_edge_stop_is_exact(ctx):
    """Normals +x | +y and sigma_normal 0.05: the cross weight exp(-2 / 0.0025) is 0
    in float32, so the left half cannot see the right half's colours."""
    s, d, pt, rad, aov = ctx
    nrm = np.zeros((H, W, 3), np.float32)
    nrm[:, :18] = (1.0, 0.0, 0.0)
    nrm[:, 18:] = (0.0, 1.0, 0.0)
    g = {"albedo": aov["albedo"], "normal": nrm, "depth": np.full((H, W), 3.0, np.float32)}
    other = rad.copy()
    other[:, 18:] = np.random.default_rng(5).uniform(0.0, 2.0, (H, W - 18, 3)).astype(np.float32)
    kw = dict(iterations=5, sigma_color=4.0, sigma_normal=0.05, sigma_depth=0.05)
    a = pt.denoise(d, rad, g, **kw)
    b = pt.denoise(d, other, g, **kw)
    assert np.array_equal(_bits(a[:, :18]), _bits(b[:, :18]))
    assert not np.array_equal(_bits(a[:, 18:]), _bits(b[:, 18:]))
    assert np.abs(a[:, :18] - rad[:, :18]).max() > 0.05    # the left half was filtered within itself


def test_zero_iterations_and_in_place(ctx):
    s, d, pt, rad, aov = ctx
    out = pt.denoise(d, rad, aov, iterations=0, **SIG)
    assert np.array_equal(_bits(out), _bits(rad))          # no demodulation round trip
    ref = pt.denoise(d, rad, aov, iterations=3, **SIG)
    buf = rad.copy()
    assert pt.denoise(d, buf, aov, iterations=3, out=buf, **SIG) is buf
    assert np.array_equal(_bits(buf), _bits(ref))


def test_device_tensors(ctx):
    import torch
    s, d, pt, rad, aov = ctx
    ref = pt.denoise(d, rad, aov, iterations=3, **SIG)
    dev = torch.device("cuda", 0)
    t_rad = torch.from_numpy(rad).to(dev)
    t_aov = {k: torch.from_numpy(v).to(dev) for k, v in aov.items()}
    t_out = torch.zeros((H, W, 3), device=dev)
    pt.denoise(d, t_rad, t_aov, iterations=3, out=t_out, **SIG)
    assert np.array_equal(_bits(t_out.cpu().numpy()), _bits(ref))
    pt.denoise(d, t_rad, t_aov, iterations=3, out=t_rad, **SIG)          # in place on the device
    assert np.array_equal(_bits(t_rad.cpu().numpy()), _bits(ref))


def test_framebuffer_follows_copy_to_fb(ctx):
    s, d, pt, rad, aov = ctx
    fb = np.full((H, W, 4), 0x5A, np.uint8)
    out = pt.denoise(d, rad, aov, iterations=2, framebuffer=fb, **SIG)
    # Spectrum::toUChar (material.h:74-81): truncating clamp of c * 255 to [0, 255], float32
    x = out * np.float32(255.0)
    byte = np.maximum(np.minimum(x, np.float32(255.0)), np.float32(0.0)).astype(np.uint8)
    assert (out > 1.0).any()                               # the clamp is exercised
    assert np.array_equal(fb[..., :3], byte[::-1, :, ::-1])            # row 0 = top; B, G, R
    assert (fb[..., 3] == 0x5A).all()                      # alpha untouched


def test_deterministic(ctx):
    s, d, pt, rad, aov = ctx
    a = pt.denoise(d, rad, aov, iterations=5, **SIG)
    b = pt.denoise(d, rad, aov, iterations=5, **SIG)
    assert np.array_equal(_bits(a), _bits(b))


def test_refusals(ctx):
    s, d, pt, rad, aov = ctx
    L = T.lib()
    out = np.full((H, W, 3), -7.0, np.float32)

    def call(guides, params):
        g = _lib.Aov(*[(guides[k].ctypes.data if guides.get(k) is not None else None)
                       for k in ("albedo", "normal", "depth")], None, None)
        p = _lib.DenoiseParams(*params)
        return L.tpt_denoise(d.handle, W, H, rad.ctypes.data, C.byref(g), C.byref(p), out.ctypes.data, None, None)

    ok = (3, 4.0, 0.3, 0.05, 1)
    for missing in ("albedo", "normal", "depth"):
        assert call({k: v for k, v in aov.items() if k != missing}, ok) == 1
        assert b"guides" in L.tpt_last_error()
    assert call(aov, (9, 4.0, 0.3, 0.05, 1)) == 1 and b"iterations" in L.tpt_last_error()
    assert call(aov, (-1, 4.0, 0.3, 0.05, 1)) == 1
    for bad in ((3, 0.0, 0.3, 0.05, 1), (3, 4.0, -0.3, 0.05, 1), (3, 4.0, 0.3, float("nan"), 1)):
        assert call(aov, bad) == 1 and b"sigma" in L.tpt_last_error()
    assert call(aov, (3, 4.0, 0.3, 0.05, 64)) == 1         # unknown flag
    assert (out == -7.0).all()                             # no refused call wrote anything
    assert call(aov, ok) == 0


def test_end_to_end_lowers_the_error(gpu_available):
    """box at 96x54, seed 42: the denoised 8-spp frame is closer to a 2,048-spp frame
    than the 8-spp frame is (the ratio is recorded in DESIGN.md, not asserted)."""
    w, h = 96, 54
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", w, h, 0)
    noisy = np.zeros((h, w, 3), np.float32)
    truth = np.zeros((h, w, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, 8, seed=42, radiance=noisy)
    pt.doTrace(d, s.m_camera, None, 2048, seed=42, radiance=truth)
    aov = pt.renderAOV(d, s.m_camera)
    clean = pt.denoise(d, noisy, aov)                      # the host's defaults
    d.close()
    mse = lambda a: float(((a.astype(np.float64) - truth) ** 2).mean())
    print(f"MSE noisy {mse(noisy):.5f}, denoised {mse(clean):.5f}, ratio {mse(clean) / mse(noisy):.4f}")
    assert mse(clean) < mse(noisy)
