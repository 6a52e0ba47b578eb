"""tpt_temporal_path and tpt_render_aov_path_points on the device: accumulation that follows
reflections in mirrors, against the float64 restatement of its definition
(tests/temporal_path_ref.py; DESIGN.md section 5 "Temporal accumulation through mirrors") on
the device's own mirror-path buffers, and the terminal points against the oracle's walk.

Bound.  The a-priori ceiling is tests/test_gpu_temporal.py's: 4e-3 of the value range up to
63-pixel coordinates, doubling with each power of two after (131 pixels: 1.6e-2; 257: 3.1e-2).
The asserted bound is ten times the largest max|gpu - ref| / max|ref| measured on an MI355X
over colour, variance and history length of every case below (temporal_path_cases.GPU_BOUND)
and lies under the smallest ceiling.  Measured (undecidable pixels of the moving frames in
brackets):
  hall 80 x 45 (cap 3), two frames, both demodulate settings   colour 2.52e-6, variance 4.21e-6 / 5.46e-6 [3 of 3,600]
  hall 80 x 45, chain of three                                   colour 3.22e-6, variance 4.14e-6 [5, 2]
  box2 80 x 45 (cap 8), two frames                               colour 2.22e-6, variance 3.56e-6 [1]
  box2 80 x 45, chain of three                                   colour 3.22e-6, variance 4.47e-6 [5, 1]
  tilted 80 x 45 (cap 3), two frames                             colour 2.22e-6, variance 3.56e-6 [2]
  box 80 x 45 (cap 8: the mirror ball), two frames               colour 3.37e-6, variance 4.23e-6 [3]
  tir 80 x 45 (no mirror), chain of three                        colour 1.87e-6, variance 3.81e-6 [0]
  hall 131 x 9                                                   colour 1.66e-6, variance 2.68e-6 [0]
  hall 16 x 16, 3 x 2, 1 x 1                                     colour 0 .. 3.3e-7, variance 0 .. 1.05e-6 [0]
  hall 257 x 241 static, either block shape                      colour 1.20e-7, variance 8.99e-7 [0]
Every first frame is exact, every whole history length too, and the two block shapes agree bit
for bit.  The largest value is 5.464e-6 (variance, hall two frames demodulated, frame 2).
tpt_render_aov_path_points at 128 x 72 against the restatement: see test_points_match_the_restatement.
"""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests import path_ref as P
from tests import temporal_path_cases as K
from tests import temporal_path_ref as TP
from tests import variant_scenes as V
from tests.test_gpu_temporal import CEILING, compare

pytestmark = pytest.mark.gpu

BOUND = K.GPU_BOUND
assert BOUND <= CEILING
AOV_KEYS = ("albedo", "normal", "depth", "face", "material", "bounces")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cam(c):
    return T.Camera(c["c2w"], c["vfov"], c["aspect"])


@pytest.fixture(scope="module")
def scenes(gpu_available):
    """name -> built device scene; built on first use, read only."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = V.device_scene(K.source(name)).copySceneToDevice(0).build()
        return made[name]

    yield get
    for d in made.values():
        d.close()


_FRAMES = {}


def device_frames(scenes, case, cap=None):
    """The case's cameras and, per camera, seeded random radiance and the device's own
    mirror-path buffers with points; rendered once per (case, cap), never written to."""
    name, w, h, case_cap, _ = K.GPU_CASES[case]
    cap = case_cap if cap is None else cap
    if (case, cap) not in _FRAMES:
        cams = K.case_cameras(case)
        pt = T.PathTracer("", w, h, 0)
        bufs = [pt.renderAOVPath(scenes(name), _cam(c), cap, points=True) for c in cams]
        _FRAMES[case, cap] = cams, [(K.radiance(101 + 101 * i, b), b) for i, b in enumerate(bufs)]
    return _FRAMES[case, cap]


def run(d, cams, frames, demodulate, flags=0, point_tol=K.POINT_TOL, first_hit_calls=()):
    """A new history through the frames; returns (out, variance, history length, stats) per
    frame.  first_hit_calls: the frames that go through tpt_temporal instead."""
    h, w = frames[0][0].shape[:2]
    pt = T.PathTracer("", w, h, 0)
    hist = T.History(d, w, h)
    got = []
    for i, (cam, (rad, aov)) in enumerate(zip(cams, frames)):
        var, n, st = np.full((h, w), -3.0, np.float32), np.full((h, w), -3.0, np.float32), {}
        kw = dict(K.PARAMS, demodulate=demodulate, flags=flags, variance=var, history_len=n, stats=st)
        if i in first_hit_calls:
            out = pt.temporal(hist, _cam(cam), rad, aov, **kw)
        else:
            out = pt.temporalPath(hist, _cam(cam), rad, aov, point_tol=point_tol, **kw)
        got.append((out, var, n, st))
    hist.close()
    return got


MOVING = [c for c in K.GPU_CASES if not c.endswith("static")]


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("case", MOVING)
def test_matches_numpy_reference(scenes, case, demodulate):
    """Two frames, or a chain of three, under the translated camera: row segments against the
    reference on decidable pixels, 16x16 tiles against row segments bit for bit."""
    name = K.GPU_CASES[case][0]
    cams, frames = device_frames(scenes, case)
    refs = K.run_reference(frames, cams, demodulate)
    rows = run(scenes(name), cams, frames, demodulate)
    tiles = run(scenes(name), cams, frames, demodulate, flags=_lib.TEMPORAL_TILES)
    for i, (g, r) in enumerate(zip(rows, refs)):
        compare(f"{case} demodulate {demodulate} frame {i + 1}", g, r, exact_n=i < 2, bound=BOUND)
    for g, t in zip(rows, tiles):
        for a, b in zip(g[:3], t[:3]):
            assert np.array_equal(_bits(a), _bits(b))
        assert g[3]["reprojected"] == t[3]["reprojected"]
    w, h = K.GPU_CASES[case][1:3]
    if w * h >= 256 and name != "tir":                     # both branches, on the mirrors too
        k, n = frames[-1][1]["bounces"], rows[-1][2]
        assert (n[k > 0] > 1.0).any() and (n[k > 0] == 1.0).any() and (n[k == 0] > 1.0).any()


@pytest.mark.parametrize("flags", [0, _lib.TEMPORAL_TILES], ids=["rows", "tiles"])
def test_counter_wraps_static(scenes, flags):
    """257 x 241: more blocks than counter slots under either block shape.  A static camera
    snaps every pixel onto one tap of weight 1 whose k', material and point are its own: the
    count is the frame, exactly."""
    case = "hall_257x241_static"
    name, w, h = K.GPU_CASES[case][:3]
    cams, frames = device_frames(scenes, case)
    refs = K.run_reference(frames, cams, True)
    got = run(scenes(name), cams, frames, True, flags=flags)
    assert refs[1]["decidable"].all() and refs[1]["reprojected"].all()
    assert got[1][3]["reprojected"] == w * h and (got[1][2] == 2.0).all()
    assert (frames[1][1]["bounces"] > 0).sum() > 5000
    for i in range(2):
        compare(f"{case} flags {flags} frame {i + 1}", got[i], refs[i], bound=BOUND)


def mirror_block(aov, want_hit):
    """The followed pixels of a frame that end on a surface (want_hit) or in the sky."""
    return (aov["bounces"] > 0) & ((aov["material"] >= 0) == want_hit)


@pytest.mark.parametrize("field", ["k", "material", "point", "direction"])
def test_rejection_is_exact(scenes, field):
    """A static camera; frame 1's buffers are frame 2's with one field changed on a block of
    mirror pixels.  Exactly those pixels come back with N = 1 and the input's bits; every
    other pixel has N = 2."""
    case = "box2_two" if field == "direction" else "hall_two"
    name, w, h = K.GPU_CASES[case][:3]
    cams, frames = device_frames(scenes, case)
    cam, (rad2, aov2) = cams[0], frames[0]
    block = mirror_block(aov2, field != "direction")
    assert block.sum() >= 20
    aov1 = {k: v.copy() for k, v in aov2.items()}
    tol = K.POINT_TOL * TP.footprint(cam, h)
    if field == "k":
        aov1["bounces"][block] += 1
    elif field == "material":
        aov1["material"][block] += 1
    elif field == "point":                                 # two tolerances along x
        aov1["points"][block, 0] += (2.0 * tol * aov2["depth"][block]).astype(np.float32)
    else:                                                  # turned by two tolerances: a unit vector still
        d = aov2["points"][block].astype(np.float64)
        side = np.cross(d, [0.0, 1.0, 0.0])
        side /= np.linalg.norm(side, axis=-1, keepdims=True)
        a = 2.0 * tol
        aov1["points"][block] = (np.cos(a) * d + np.sin(a) * side).astype(np.float32)
    rad1 = K.radiance(55, aov1)
    for flags in (0, _lib.TEMPORAL_TILES):
        out, var, n, st = run(scenes(name), (cam, cam), ((rad1, aov1), (rad2, aov2)), False, flags=flags)[1]
        assert (n[block] == 1.0).all() and (n[~block] == 2.0).all()
        assert np.array_equal(_bits(out[block]), _bits(rad2[block]))
        assert st["reprojected"] == w * h - int(block.sum())


@pytest.mark.parametrize("case,cap", [("tir_chain", 8), ("box2_chain", 0)])
def test_equals_temporal_bit_for_bit(scenes, case, cap):
    """No mirror followed -- tir has none, box2's buffers at cap 0 are first-hit buffers --
    over a three-frame translated chain: outputs, variance, history lengths and the count are
    tpt_temporal's, and so is the state (the later frames read it)."""
    name = K.GPU_CASES[case][0]
    cams, frames = device_frames(scenes, case, cap)
    assert all((aov["bounces"] == 0).all() for _, aov in frames)
    for demodulate in (False, True):
        for flags in (0, _lib.TEMPORAL_TILES):
            path = run(scenes(name), cams, frames, demodulate, flags=flags)
            first = run(scenes(name), cams, frames, demodulate, flags=flags, first_hit_calls=(0, 1, 2))
            # and alternating: the state either entry point leaves is the other's
            mixed = run(scenes(name), cams, frames, demodulate, flags=flags, first_hit_calls=(1,))
            for other in (first, mixed):
                for g, f in zip(path, other):
                    for a, b in zip(g[:3], f[:3]):
                        assert np.array_equal(_bits(a), _bits(b))
                    assert g[3]["reprojected"] == f[3]["reprojected"]
    assert (path[2][2] > 2.0).any() and (path[2][2] == 1.0).any()


def test_a_first_hit_call_disoccludes_the_mirror_pixels(scenes):
    """tpt_temporal leaves k' = 0 everywhere: the path call after it starts every k > 0 pixel
    over, and a static camera's k = 0 pixels all keep their history."""
    name, w, h = K.GPU_CASES["hall_two"][:3]
    cams, frames = device_frames(scenes, "hall_two")
    cam, frame = cams[0], frames[0]
    got = run(scenes(name), (cam, cam, cam), (frame, frame, frame), True, first_hit_calls=(1,))
    k = frame[1]["bounces"]
    assert (k > 0).sum() > 300
    assert (got[1][2] == 2.0).all()                        # the first-hit call reprojects a path call's state
    n = got[2][2]
    assert (n[k > 0] == 1.0).all() and (n[k == 0] == 3.0).all()
    assert np.array_equal(_bits(got[2][0][k > 0]), _bits(frame[0][k > 0]))
    assert got[2][3]["reprojected"] == int((k == 0).sum())


_WALKS = {}


@pytest.mark.parametrize("name,cap", [("hall", 3), ("tinted", 3), ("tilted", 3)])
def test_points_match_the_restatement(scenes, name, cap):
    """tpt_render_aov_path_points at 128 x 72: over path_ref.comparable pixels the points are the
    restatement's within tests/test_gpu_aov.py's 1e-4 relative (hits: of the distance
    travelled; directions: of 1), and every other output is tpt_render_aov_path's bytes."""
    w, h = 128, 72
    d = scenes(name)
    pt = T.PathTracer("", w, h, 0)
    cam = _cam(K.scene_camera(name))
    st_a, st_b = {}, {}
    plain = pt.renderAOVPath(d, cam, cap, stats=st_a)
    with_points = pt.renderAOVPath(d, cam, cap, stats=st_b, points=True)
    for key in AOV_KEYS:
        assert np.array_equal(_bits(plain[key]), _bits(with_points[key])), key
    assert (st_a["followed"], st_a["deepest"]) == (st_b["followed"], st_b["deepest"])
    ref = TP.oracle_aov_path_points(K.packed(name), w, h, cap, tracer=K.tracer(name))
    ok = P.comparable(ref)
    hit = ok & (ref["face"] >= 0)
    miss = ok & (ref["face"] < 0)
    followed = ok & (ref["bounces"] > 0)
    assert ok.mean() >= 0.7 and followed.sum() >= 300 and (followed & hit).sum() >= 200
    got = with_points["points"].astype(np.float64)
    err_hit = np.linalg.norm(got[hit] - ref["points"][hit], axis=-1) / ref["depth"][hit]
    print(f"{name} cap {cap}: points, max relative error on hits {err_hit.max():.3e}", end="")
    assert err_hit.max() <= 1e-4
    if miss.any():
        err_miss = np.linalg.norm(got[miss] - ref["points"][miss], axis=-1)
        print(f", on directions {err_miss.max():.3e} ({int(miss.sum())} pixels, {int((miss & followed).sum())} followed)")
        assert err_miss.max() <= 1e-4


# the direct calls below: the cases' tolerance, not the hosts' default
DIRECT = dict(K.PARAMS, point_tol=K.POINT_TOL)


def test_device_tensors_and_in_place(scenes):
    import torch
    name, w, h = K.GPU_CASES["hall_two"][:3]
    d = scenes(name)
    cams, frames = device_frames(scenes, "hall_two")
    want = run(d, cams, frames, True)[1]
    dev = torch.device("cuda", 0)
    up = lambda a: {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
    pt = T.PathTracer("", w, h, 0)
    hist = T.History(d, w, h)
    t1, t2 = (torch.from_numpy(f[0]).to(dev) for f in frames)
    pt.temporalPath(hist, _cam(cams[0]), t1, up(frames[0][1]), out=t1, **DIRECT)
    assert np.array_equal(_bits(t1.cpu().numpy()), _bits(frames[0][0]))
    t_var, t_n = torch.zeros((h, w), device=dev), torch.zeros((h, w), device=dev)
    assert pt.temporalPath(hist, _cam(cams[1]), t2, up(frames[1][1]), out=t2, variance=t_var, history_len=t_n,
                           **DIRECT) is t2
    for got, ref in ((t2, want[0]), (t_var, want[1]), (t_n, want[2])):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref))
    hist.reset()                                           # in place in host memory
    b1, b2 = frames[0][0].copy(), frames[1][0].copy()
    pt.temporalPath(hist, _cam(cams[0]), b1, frames[0][1], out=b1, **DIRECT)
    assert pt.temporalPath(hist, _cam(cams[1]), b2, frames[1][1], out=b2, **DIRECT) is b2
    assert np.array_equal(_bits(b2), _bits(want[0]))
    hist.close()
    # the points into a device tensor one row longer: nothing is written past the end
    whole = torch.full((h + 1, w, 3), -7.0, device=dev)
    got = pt.renderAOVPath(d, _cam(cams[0]), 3, out={"points": whole[:h]})
    assert set(got) == {"points"}
    back = whole.cpu().numpy()
    assert (back[h] == -7.0).all() and not (back[:h] == -7.0).any()
    assert np.array_equal(_bits(back[:h]), _bits(frames[0][1]["points"]))


def test_nothing_is_written_past_the_end(scenes):
    """131 x 9, out, variance and history_len the first H rows of device tensors one row
    longer: the extra row keeps its sentinel, and no sentinel survives inside."""
    import torch
    case = "hall_131x9"
    name, w, h = K.GPU_CASES[case][:3]
    d = scenes(name)
    cams, frames = device_frames(scenes, case)
    dev = torch.device("cuda", 0)
    up = lambda a: {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
    pt = T.PathTracer("", w, h, 0)
    for flags in (0, _lib.TEMPORAL_TILES):
        want = run(d, cams, frames, True, flags=flags)[1]
        hist = T.History(d, w, h)
        for cam, (rad, aov) in zip(cams, frames):
            whole = [torch.full((h + 1, w, 3), -7.0, device=dev), torch.full((h + 1, w), -7.0, device=dev),
                     torch.full((h + 1, w), -7.0, device=dev)]
            pt.temporalPath(hist, _cam(cam), torch.from_numpy(rad).to(dev), up(aov), out=whole[0][:h],
                            variance=whole[1][:h], history_len=whole[2][:h], flags=flags, **DIRECT)
        hist.close()
        for t, ref in zip(whole, want[:3]):
            got = t.cpu().numpy()
            assert (got[h] == -7.0).all() and not (got[:h] == -7.0).any()
            assert np.array_equal(_bits(got[:h]), _bits(ref))


def test_refusals(scenes):
    """Each bad argument returns TPT_ERR_INVALID_ARG, writes nothing and leaves the history as
    it was: the next valid call gives what an undisturbed history gives."""
    L = T.lib()
    name, w, h = K.GPU_CASES["hall_two"][:3]
    d = scenes(name)
    cams, frames = device_frames(scenes, "hall_two")
    (rad1, aov1), (rad2, aov2) = frames
    want = run(d, cams, frames, True)[1]
    pt = T.PathTracer("", w, h, 0)
    hist = T.History(d, w, h)
    pt.temporalPath(hist, _cam(cams[0]), rad1, aov1, **DIRECT)
    out = np.full((h, w, 3), -7.0, np.float32)
    var = np.full((h, w), -7.0, np.float32)
    n = np.full((h, w), -7.0, np.float32)
    cam = _cam(cams[1]).to_c()
    ok = (0.1, 0.1, 0.9, 32, 1, K.POINT_TOL)

    def call(guides=aov2, params=ok, handle=hist.handle, camera=C.byref(cam), rin=rad2.ctypes.data,
             rout=out.ctypes.data, bounces=aov2["bounces"].ctypes.data, points=aov2["points"].ctypes.data,
             no_guides=False, no_params=False):
        g = _lib.Aov(*[(guides[k].ctypes.data if guides.get(k) is not None else None)
                       for k in ("albedo", "normal", "depth")], None,
                     guides["material"].ctypes.data if guides.get("material") is not None else None)
        p = _lib.TemporalPathParams(*params)
        return L.tpt_temporal_path(handle, camera, rin, None if no_guides else C.byref(g), bounces, points,
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
    refused(b"bounce", bounces=None)
    refused(b"points", points=None)
    for tol in (0.0, -1.0, float("nan")):
        refused(b"point_tol", params=(0.1, 0.1, 0.9, 32, 1, tol))
    for alpha in (0.0, 1.5, float("nan")):
        refused(b"alpha", params=(alpha, 0.1, 0.9, 32, 1, 1.0))
    refused(b"depth_tol", params=(0.1, 0.0, 0.9, 32, 1, 1.0))
    refused(b"normal_min", params=(0.1, 0.1, 1.5, 32, 1, 1.0))
    refused(b"max_history", params=(0.1, 0.1, 0.9, 0, 1, 1.0))
    refused(b"flag", params=(0.1, 0.1, 0.9, 32, 64, 1.0))
    refused(b"output", rout=None)
    assert (out == -7.0).all() and (var == -7.0).all() and (n == -7.0).all()   # no refused call wrote anything
    got = pt.temporalPath(hist, _cam(cams[1]), rad2, aov2, variance=var, history_len=n, **DIRECT)
    hist.close()
    for a, b in zip((got, var, n), want[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    # tpt_render_aov_path_points refuses what tpt_render_aov_path refuses
    c0 = _cam(cams[0]).to_c()
    pts = np.full((h, w, 3), -7.0, np.float32)
    for params, word in ((_lib.AovPathParams(65, 0), b"max_bounces"), (_lib.AovPathParams(3, 1), b"flags")):
        assert L.tpt_render_aov_path_points(d.handle, C.byref(c0), w, h, C.byref(params), None, None,
                                            pts.ctypes.data, None) == 1
        assert word in L.tpt_last_error()
    assert L.tpt_render_aov_path_points(d.handle, C.byref(c0), w, h, C.byref(_lib.AovPathParams(3, 0)), None, None,
                                        None, None) == 1
    assert (pts == -7.0).all()


def test_end_to_end_on_a_trucking_camera(scenes):
    """box2 at 96 x 54: eight frames of 8 spp, seeds 1..8, the camera trucking a seventh of the
    tests' translation per frame, against 2,048 spp at the last camera; the MSE over the pixels
    whose first hit is a mirror, for the last frame alone, for tpt_temporal on first-hit guides
    and for tpt_temporal_path at the hosts' defaults.  tools/temporal_path_quality.py measures
    the same on the CPU with the oracle and the numpy references: first hit 0.02129, path
    0.02219 at point_tol 8, the sweep's best -- a ratio of 1.042, which is not below 0.9.  So
    nothing is asserted about the quality against tpt_temporal (DESIGN.md records the negative,
    and the pass stays opt-in); asserted is what accumulation must give on any guides: the
    mirror's pixels keep a history under the moving camera and end closer to the truth than
    the last frame alone."""
    w, h, frames = 96, 54, 8
    d = scenes("box2")
    base = _cam(K.scene_camera("box2"))
    step = K.translation("box2") / (frames - 1)
    pt = T.PathTracer("", w, h, 0)
    hists = T.History(d, w, h), T.History(d, w, h)
    noisy = np.zeros((h, w, 3), np.float32)
    n_path = np.zeros((h, w), np.float32)
    for i in range(frames):
        cam = base.moved(*(i * step))
        pt.doTrace(d, cam, None, 8, seed=i + 1, radiance=noisy)
        first = pt.temporal(hists[0], cam, noisy, pt.renderAOV(d, cam))
        path = pt.temporalPath(hists[1], cam, noisy, pt.renderAOVPath(d, cam, 8, points=True), history_len=n_path)
    truth = np.zeros((h, w, 3), np.float32)
    pt.doTrace(d, cam, None, 2048, seed=42, radiance=truth)
    for hist in hists:
        hist.close()
    guides = pt.renderAOVPath(d, cam, 8)
    mirror = guides["bounces"] > 0                         # box2's mirrors: followed at the first hit
    mse = lambda a: float(((a.astype(np.float64) - truth) ** 2)[mirror].mean())
    print(f"mirror pixels {int(mirror.sum())}: MSE last 8-spp frame {mse(noisy):.5f}, tpt_temporal {mse(first):.5f}, "
          f"tpt_temporal_path {mse(path):.5f}, ratio path / first hit {mse(path) / mse(first):.4f}; "
          f"mean history on the mirror {n_path[mirror].mean():.2f}")
    assert mirror.sum() >= 300
    assert mse(path) < mse(noisy)
    assert n_path[mirror].mean() > 4.0
