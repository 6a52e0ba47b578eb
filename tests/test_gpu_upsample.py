"""tpt_upsample: guided upsampling against the float64 numpy restatement of its definition
(tests/upsample_ref.py; DESIGN.md section 5 "Guided upsampling"), its exact properties, one real
scene and its refusals.  The synthetic inputs are tests/upsample_cases.py's, whose premises
tests/test_upsample_cpu.py checks without a GPU."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import scene_path
from tests import upsample_cases as K
from tests import upsample_ref as R

pytestmark = pytest.mark.gpu

# Full size from low size:
#   37x29 from 19x15   scale 2, rounded up              131x9 from 33x3   several blocks, partial tiles
#   37x29 from 13x10   scale 3: centres that coincide,  16x16 from 4x4    exactly one tile
#                      the b == 0 taps                  17x16 from 9x8    a tile of one column
#   37x29 from 24x17   a non-integer ratio              5x3 from 1x1      every tap clamped to one pixel
#   37x29 from 37x29   equal sizes                      1x1 from 1x1      a single pixel


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(gpu_available):
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    yield s, d
    d.close()


@pytest.fixture(scope="module")
def refs():
    """Every case's inputs and reference, computed once and left unchanged."""
    out = {}
    for (full, low), cid in zip(K.CASES, K.CASE_IDS):
        rad, gl, g = K.case_inputs(full, low)
        for demod in (False, True):
            out[cid, demod] = (rad, gl, g) + R.upsample_ref(rad, gl, g, demodulate=demod, **K.SIGMA)
    return out


# Bound: the output is a mean of at most four colours whose weights are b exp(-(e - e_min)).  The
# float32 e carries a few ulp of relative error, so a weight's relative error is a few ulp times e,
# and tests/test_upsample_cpu.py holds e_min <= 1,000 for these inputs: about 1e-3 at the worst, and
# the hardware's approximate exp adds a few ulp.  Measured on MI355X the maximum over the eighteen
# cases is far lower (the mean is kept as c_r + sum w dc / sum w, so weight errors scale with the
# colour differences, and the taps that matter have small e), and the bound is ten times that
# measurement.  Measured on MI355X, max |gpu - ref| / max |ref|, without / with demodulation:
#   37x29 from 19x15   1.08e-7 / 1.15e-7      16x16 from 4x4   8.8e-8 / 1.10e-7
#   37x29 from 13x10   8.8e-8 / 1.40e-7       17x16 from 9x8   9.4e-8 / 1.18e-7
#   37x29 from 24x17   1.03e-7 / 1.20e-7      5x3 from 1x1     0 / 2.3e-8
#   37x29 from 37x29   0 / 8.0e-8             1x1 from 1x1     0 / 0
#   131x9 from 33x3    7.64e-7 / 7.10e-7      box 64x48 from 32x24: 8.5e-8 first-hit, 1.34e-7 path + demodulation
MEASURED_MAX = 7.640e-7             # 131x9 from 33x3, no demodulation (its largest e_min is 162)
BOUND = 10 * MEASURED_MAX
assert BOUND <= 1e-3


@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulate"])
@pytest.mark.parametrize("case", range(len(K.CASES)), ids=K.CASE_IDS)
def test_matches_numpy_reference(ctx, refs, case, demodulate):
    s, d = ctx
    (W, H), _ = K.CASES[case]
    rad, gl, g, ref, fb = refs[K.CASE_IDS[case], demodulate]
    st = {}
    out = T.PathTracer("", W, H, 0).upsample(d, rad, gl, g, demodulate=demodulate, stats=st, **K.SIGMA)
    err = np.abs(out.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"{K.CASE_IDS[case]} demodulate {demodulate}: max |gpu - ref| / max |ref| = {err:.3e}, "
          f"fallback {st['fallback']} (reference {int(fb.sum())}) of {W * H}")
    assert np.isfinite(out).all()
    assert st["fallback"] == int(fb.sum())                 # exact: the decision is made in integers
    assert err <= BOUND                                    # every pixel, fallback ones included


def test_equal_sizes_give_the_input_bits(ctx, refs):
    s, d = ctx
    rad, gl, g, _, _ = refs["37x29-from-37x29", False]
    st = {}
    out = T.PathTracer("", 37, 29, 0).upsample(d, rad, gl, g, demodulate=False, stats=st, **K.SIGMA)
    assert np.array_equal(_bits(out), _bits(rad))
    assert st["fallback"] == 0


@pytest.mark.parametrize("case", range(len(K.CASES)), ids=K.CASE_IDS)
def test_constant_frame_gives_the_constant_bits(ctx, refs, case):
    s, d = ctx
    (W, H), (wl, hl) = K.CASES[case]
    _, gl, g, _, _ = refs[K.CASE_IDS[case], False]
    const = np.full((hl, wl, 3), 0.7371, np.float32)
    out = T.PathTracer("", W, H, 0).upsample(d, const, gl, g, demodulate=False, **K.SIGMA)
    assert np.array_equal(_bits(out), _bits(np.full((H, W, 3), 0.7371, np.float32)))


@pytest.mark.parametrize("case", range(len(K.CASES)), ids=K.CASE_IDS)
def test_material_coded_frame_keeps_each_pixels_own_code(ctx, refs, case):
    s, d = ctx
    (W, H), _ = K.CASES[case]
    _, gl, g, _, fb = refs[K.CASE_IDS[case], False]
    out = T.PathTracer("", W, H, 0).upsample(d, K.material_coded(gl), gl, g, demodulate=False, **K.SIGMA)
    want = K.material_coded(g)
    assert np.array_equal(_bits(out[~fb]), _bits(want[~fb]))


def test_deterministic_and_device_tensors(ctx, refs):
    """Two calls give equal bits; torch CUDA tensors and numpy arrays give equal bits; out= a
    preallocated buffer is written in place, and nothing past its end."""
    import torch
    s, d = ctx
    pt = T.PathTracer("", 37, 29, 0)
    for demod in (False, True):
        rad, gl, g, _, fb = refs["37x29-from-19x15", demod]
        a = pt.upsample(d, rad, gl, g, demodulate=demod, **K.SIGMA)
        b = pt.upsample(d, rad, gl, g, demodulate=demod, **K.SIGMA)
        assert np.array_equal(_bits(a), _bits(b))
        buf = np.full((29, 37, 3), -7.0, np.float32)
        assert pt.upsample(d, rad, gl, g, demodulate=demod, out=buf, **K.SIGMA) is buf
        assert np.array_equal(_bits(buf), _bits(a))
        dev = torch.device("cuda", 0)
        t = lambda aov: {k: torch.from_numpy(v).to(dev) for k, v in aov.items()}
        whole = torch.full((30, 37, 3), -7.0, device=dev)  # one row longer: the extra row keeps its sentinel
        t_out = whole[:29]
        st = {}
        assert pt.upsample(d, torch.from_numpy(rad).to(dev), t(gl), t(g), demodulate=demod, out=t_out, stats=st,
                           **K.SIGMA) is t_out
        got = whole.cpu().numpy()
        assert (got[29] == -7.0).all()
        assert np.array_equal(_bits(got[:29]), _bits(a))
        assert st["fallback"] == int(fb.sum())
        # a raw device pointer names its size
        t_rad = torch.from_numpy(rad).to(dev)
        torch.cuda.synchronize()                           # (the host does not see a raw pointer's stream)
        c = pt.upsample(d, t_rad.data_ptr(), t(gl), t(g), demodulate=demod, low_size=(19, 15), **K.SIGMA)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(c), _bits(a))


def test_framebuffer_follows_copy_to_fb(ctx, refs):
    s, d = ctx
    rad, gl, g, _, _ = refs["37x29-from-19x15", False]
    fb = np.full((29, 37, 4), 0x5A, np.uint8)
    out = T.PathTracer("", 37, 29, 0).upsample(d, rad, gl, g, framebuffer=fb, **K.SIGMA)
    x = out * np.float32(255.0)                            # Spectrum::toUChar: truncating clamp, float32
    byte = np.maximum(np.minimum(x, np.float32(255.0)), np.float32(0.0)).astype(np.uint8)
    assert (out > 1.0).any() and (out < 1.0).any()         # the clamp is exercised
    assert np.array_equal(fb[..., :3], byte[::-1, :, ::-1])            # row 0 = top; B, G, R
    assert (fb[..., 3] == 0x5A).all()                      # alpha untouched


@pytest.mark.parametrize("path", [False, True], ids=["first-hit", "mirror-path-demodulate"])
def test_real_scene(ctx, path):
    """box at 64x48 from 32x24: the GPU's own feature buffers at both sizes and a 4-spp render at
    the low size, against the reference under the same bound; once with the mirror-path guides and
    DEMODULATE."""
    s, d = ctx
    full, low = T.PathTracer("", 64, 48, 0), T.PathTracer("", 32, 24, 0)
    rad = np.zeros((24, 32, 3), np.float32)
    low.doTrace(d, s.m_camera, None, 4, seed=42, radiance=rad)
    aov = (lambda pt: pt.renderAOVPath(d, s.m_camera)) if path else (lambda pt: pt.renderAOV(d, s.m_camera))
    gl, g = aov(low), aov(full)
    st = {}
    out = full.upsample(d, rad, gl, g, demodulate=path, stats=st, **K.SIGMA)
    ref, fb = R.upsample_ref(rad, gl, g, demodulate=path, **K.SIGMA)
    err = np.abs(out.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"box 64x48 from 32x24, path guides {path}: max |gpu - ref| / max |ref| = {err:.3e}, "
          f"fallback {st['fallback']} of {64 * 48}")
    assert np.isfinite(out).all()
    assert st["fallback"] == int(fb.sum())
    assert err <= BOUND
    assert 2 * st["fallback"] < 64 * 48 and np.abs(out).max() > 0.0


def test_refusals(ctx, refs):
    """Each returns TPT_ERR_INVALID_ARG and leaves the output buffer untouched."""
    s, d = ctx
    L = T.lib()
    rad, gl, g, _, _ = refs["37x29-from-19x15", True]
    out = np.full((29, 37, 3), -7.0, np.float32)
    keys = ("albedo", "normal", "depth", "face", "material")

    def call(low=gl, full=g, params=(0.3, 0.05, 0), sizes=(19, 15, 37, 29), null_params=False, outputs=True):
        a, b = (_lib.Aov(*[(q[k].ctypes.data if q.get(k) is not None else None) for k in keys]) for q in (low, full))
        p = _lib.UpsampleParams(*params)
        return L.tpt_upsample(d.handle, sizes[0], sizes[1], rad.ctypes.data, C.byref(a), sizes[2], sizes[3], C.byref(b),
                              None if null_params else C.byref(p), out.ctypes.data if outputs else None, None, None)

    without = lambda q, k: {n: v for n, v in q.items() if n != k}
    assert call(null_params=True) == 1 and b"params" in L.tpt_last_error()
    assert call(low=without(gl, "material")) == 1 and b"material" in L.tpt_last_error()
    assert call(full=without(g, "material")) == 1 and b"material" in L.tpt_last_error()
    assert call(low=without(gl, "albedo"), params=(0.3, 0.05, 1)) == 1 and b"albedo" in L.tpt_last_error()
    assert call(full=without(g, "albedo"), params=(0.3, 0.05, 1)) == 1 and b"albedo" in L.tpt_last_error()
    assert call(low=without(gl, "albedo"), full=without(g, "albedo")) == 0             # needed only with DEMODULATE
    out[:] = -7.0
    assert call(sizes=(38, 15, 37, 29)) == 1 and b"larger" in L.tpt_last_error()
    assert call(sizes=(19, 30, 37, 29)) == 1 and b"larger" in L.tpt_last_error()
    for zero in ((0, 15, 37, 29), (19, 0, 37, 29), (19, 15, 0, 29), (19, 15, 37, 0), (19, 15, 37, -1)):
        assert call(sizes=zero) == 1 and b"size" in L.tpt_last_error()
    assert call(sizes=(19, 15, 1048577, 29)) == 1 and b"1048576" in L.tpt_last_error()
    for bad in ((0.0, 0.05, 0), (0.3, 0.0, 0), (float("nan"), 0.05, 0), (0.3, float("nan"), 0), (-0.3, 0.05, 0)):
        assert call(params=bad) == 1 and b"sigma" in L.tpt_last_error()
    assert call(params=(0.3, 0.05, 2)) == 1 and b"flags" in L.tpt_last_error()
    assert call(outputs=False) == 1 and b"output" in L.tpt_last_error()
    assert (out == -7.0).all()                             # no refused call wrote anything
    assert call() == 0 and not (out == -7.0).any()
