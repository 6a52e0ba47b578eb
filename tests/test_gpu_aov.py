"""tpt_render_aov: the first-hit feature buffers against the CPU oracle.

The reference rays are built in numpy float32 in sampleRays' order of operations
(tests/post_ref.py) and traced with orc_trace_ray over the oracle's BVH.  A pixel is
comparable when the 3x3 neighbourhood of the oracle's face image around it is
uniform (edge pixels replicated): a last-bit difference in ray generation cannot
change what such a pixel hits, while wrong rays, flipped rows and wrong lookups
still show."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib
from oracle import oracle as O

from tests.conftest import scene_path
from tests import post_ref as R

pytestmark = pytest.mark.gpu

W, H = 256, 144
KEYS = ("albedo", "normal", "depth", "face", "material")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def comparable(face):
    p = np.pad(face, 1, mode="edge")
    same = np.ones(face.shape, bool)
    for dy in range(3):
        for dx in range(3):
            same &= p[dy:dy + face.shape[0], dx:dx + face.shape[1]] == face
    return same


@pytest.fixture(scope="module")
def frames(gpu_available):
    """Per scene: the device scene, the GPU buffers and the oracle's (computed once, read only)."""
    out = {}
    for name in ("box", "box2"):
        s = T.Scene(scene_path(name))
        d = s.copySceneToDevice(0).build()
        pt = T.PathTracer("", W, H, 0)
        gpu = pt.renderAOV(d, s.m_camera)
        ref = R.oracle_aov(O.load_scene(scene_path(name)), W, H)
        out[name] = (s, d, pt, gpu, ref)
    yield out
    for _, d, _, _, _ in out.values():
        d.close()


@pytest.mark.parametrize("name", ["box", "box2"])
def test_aov_matches_oracle(frames, name):
    s, d, pt, gpu, ref = frames[name]
    ok = comparable(ref["face"])
    hit = ok & (ref["face"] >= 0)
    print(f"{name}: comparable {ok.mean():.3f}, comparable hits {hit.mean():.3f}")
    assert ok.mean() >= 0.75 and hit.mean() >= 0.25
    assert np.array_equal(gpu["face"][ok], ref["face"][ok])
    assert np.array_equal(gpu["material"][ok], ref["material"][ok])
    assert np.array_equal(_bits(gpu["albedo"][ok]), _bits(ref["albedo"][ok]))
    rel = np.abs(gpu["depth"][hit].astype(np.float64) - ref["depth"][hit]) / ref["depth"][hit]
    dn = np.abs(gpu["normal"][hit].astype(np.float64) - ref["normal"][hit])
    print(f"{name}: max relative depth error {rel.max():.3e}, max normal error {dn.max():.3e}")
    assert rel.max() <= 1e-4
    assert dn.max() <= 1e-4


def test_aov_matches_oracle_at_another_camera(frames):
    """A camera the scene does not ship: box2 at 128 x 72 from the scene's camera yawed
    10 degrees, its aspect changed from 16:9 to 1.5 (the frame's stays 16:9, so the
    pixels are not square).  With the oracle alone 79.9 % of the pixels are comparable
    and 28.0 % are comparable hits.  (The camera's vertical field of view is 23 degrees:
    at a yaw of 20 degrees only 11.5 % are comparable hits, at 15 degrees 19.6 %, below
    the floor of test_aov_matches_oracle, which this test keeps.)"""
    s, d, _, _, _ = frames["box2"]
    w, h = 128, 72
    cam = s.m_camera.yawed(10.0)
    cam.aspect = 1.5
    gpu = T.PathTracer("", w, h, 0).renderAOV(d, cam)
    ref = R.oracle_aov(O.load_scene(scene_path("box2")), w, h,
                       cam={"c2w": np.asarray(cam.c2w, np.float32), "vfov": cam.vfov, "aspect": cam.aspect})
    ok = comparable(ref["face"])
    hit = ok & (ref["face"] >= 0)
    miss = ok & (ref["face"] < 0)
    print(f"box2 yawed: comparable {ok.mean():.3f}, comparable hits {hit.mean():.3f}")
    assert ok.mean() >= 0.75 and hit.mean() >= 0.25
    assert np.array_equal(gpu["face"][ok], ref["face"][ok])
    assert np.array_equal(gpu["material"][ok], ref["material"][ok])
    assert np.array_equal(_bits(gpu["albedo"][ok]), _bits(ref["albedo"][ok]))
    rel = np.abs(gpu["depth"][hit].astype(np.float64) - ref["depth"][hit]) / ref["depth"][hit]
    dn = np.abs(gpu["normal"][hit].astype(np.float64) - ref["normal"][hit])
    print(f"box2 yawed: max relative depth error {rel.max():.3e}, max normal error {dn.max():.3e}")
    assert rel.max() <= 1e-4
    assert dn.max() <= 1e-4
    assert miss.sum() > 0 and (gpu["face"][miss] == -1).all() and (_bits(gpu["depth"][miss]) == 0).all()


@pytest.mark.parametrize("name", ["box", "box2"])
def test_aov_miss_convention(frames, name):
    s, d, pt, gpu, ref = frames[name]
    miss = comparable(ref["face"]) & (ref["face"] < 0)
    assert miss.sum() > 0
    assert (gpu["face"][miss] == -1).all() and (gpu["material"][miss] == -1).all()
    assert (_bits(gpu["depth"][miss]) == 0).all()
    assert (_bits(gpu["normal"][miss]) == 0).all()
    assert (gpu["albedo"][miss] == 1.0).all()


def _with_sentinel(w, h):
    """Each output with one more row past its end, filled with a sentinel."""
    bufs = {"albedo": np.full((h + 1, w, 3), -7.0, np.float32), "normal": np.full((h + 1, w, 3), -7.0, np.float32),
            "depth": np.full((h + 1, w), -7.0, np.float32), "face": np.full((h + 1, w), -77, np.int32),
            "material": np.full((h + 1, w), -77, np.int32)}
    return bufs, {k: v[:h] for k, v in bufs.items()}


def test_aov_odd_size_writes_every_pixel_and_nothing_else(frames):
    s, d, _, _, _ = frames["box"]
    w, h = 50, 38                                          # not multiples of the 16 x 16 tile
    bufs, views = _with_sentinel(w, h)
    T.PathTracer("", w, h, 0).renderAOV(d, s.m_camera, out=views)
    for k in KEYS:
        assert (bufs[k][h] == (-7.0 if bufs[k].dtype == np.float32 else -77)).all(), k
        assert not (views[k] == (-7.0 if bufs[k].dtype == np.float32 else -77)).any(), k
    assert (views["face"] >= 0).mean() > 0.25              # the box fills the middle of the frame
    assert ((views["face"] >= 0) == (views["depth"] > 0)).all()


def test_aov_device_outputs_equal_host_outputs(frames):
    import torch
    s, d, pt, gpu, _ = frames["box"]
    dev = torch.device("cuda", 0)
    out = {"albedo": torch.full((H, W, 3), -7.0, device=dev), "normal": torch.full((H, W, 3), -7.0, device=dev),
           "depth": torch.full((H, W), -7.0, device=dev),
           "face": torch.full((H, W), -77, dtype=torch.int32, device=dev),
           "material": torch.full((H, W), -77, dtype=torch.int32, device=dev)}
    pt.renderAOV(d, s.m_camera, out=out)
    for k in KEYS:
        assert np.array_equal(_bits(out[k].cpu().numpy()), _bits(gpu[k])), k


def test_aov_deterministic(frames):
    s, d, pt, gpu, _ = frames["box2"]
    st = {}
    again = pt.renderAOV(d, s.m_camera, stats=st)
    for k in KEYS:
        assert np.array_equal(_bits(again[k]), _bits(gpu[k])), k
    assert st["trace_ms"] > 0.0


def test_aov_nullable_outputs(frames):
    s, d, pt, gpu, _ = frames["box"]
    depth = np.full((H, W), -7.0, np.float32)
    out = pt.renderAOV(d, s.m_camera, out={"depth": depth})
    assert set(out) == {"depth"}
    assert np.array_equal(_bits(depth), _bits(gpu["depth"]))


@pytest.mark.parametrize("w,h", [(17, 16), (37, 29)])
def test_same_camera_reprojects_every_pixel_onto_itself(frames, w, h):
    """The feature buffers' ray and the temporal pass's are one text (post.hip centre_ray):
    a second frame of a static scene from the same camera -- box, the scene's camera yawed 7
    degrees -- finds its history at its own pixel everywhere, hit or miss, and where the
    motion vector is asked for it is zero.  tests/temporal_ref.py, fed the same buffers, says
    the same of this camera (with the oracle's buffers too: 272 of 272 and 1,073 of 1,073)."""
    from tests import temporal_ref as TR
    s, d, _, _, _ = frames["box"]
    cam = s.m_camera.yawed(7.0)
    cd = {"c2w": np.asarray(cam.c2w, np.float32), "vfov": cam.vfov, "aspect": cam.aspect}
    params = dict(alpha=0.1, depth_tol=0.1, normal_min=0.9, max_history=32, demodulate=True)
    pt = T.PathTracer("", w, h, 0)
    aov = pt.renderAOV(d, cam)
    assert 0.25 < (aov["face"] >= 0).mean() < 0.75         # hits and misses both
    rng = np.random.default_rng(5)
    rads = [rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32) for _ in range(2)]
    state = None
    for rad in rads:
        ref = TR.temporal_ref(state, cd, rad, aov, **params)
        state = ref["state"]
    assert ref["decidable"].all() and ref["reprojected"].all()
    for motion in (False, True):
        hist = T.History(d, w, h)
        for rad in rads:
            st = {}
            n = np.zeros((h, w), np.float32)
            mv = np.full((h, w, 2), -7.0, np.float32) if motion else None
            pt.temporal(hist, cam, rad, aov, history_len=n, stats=st, motion=motion, motion_out=mv, **params)
        hist.close()
        assert st["reprojected"] == w * h and (n == 2.0).all(), motion
        if motion:
            assert (mv == 0.0).all()


def test_aov_refusals(frames):
    s, d, pt, _, _ = frames["box"]
    L = T.lib()
    cam = s.m_camera.to_c()
    depth = np.zeros((H, W), np.float32)
    a = _lib.Aov(None, None, depth.ctypes.data, None, None)

    def refused(rc, word):
        assert rc == 1                                     # TPT_ERR_INVALID_ARG
        assert word in L.tpt_last_error(), L.tpt_last_error()

    unbuilt = T.Scene(scene_path("box")).copySceneToDevice(0)
    refused(L.tpt_render_aov(unbuilt.handle, C.byref(cam), W, H, C.byref(a), None), b"not built")
    unbuilt.close()
    refused(L.tpt_render_aov(d.handle, C.byref(cam), 0, H, C.byref(a), None), b"frame size")
    refused(L.tpt_render_aov(d.handle, C.byref(cam), W, -3, C.byref(a), None), b"frame size")
    refused(L.tpt_render_aov(d.handle, C.byref(cam), W, H, None, None), b"null")
    none = _lib.Aov()
    refused(L.tpt_render_aov(d.handle, C.byref(cam), W, H, C.byref(none), None), b"every pointer")
    assert (depth == 0).all()                              # no refused call wrote anything
