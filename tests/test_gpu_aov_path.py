"""tpt_render_aov_path: the mirror-path feature buffers against the CPU restatement of
their definition (tests/path_ref.py), on the scenes of tests/path_scenes.py whose
premises tests/test_path_scenes_cpu.py states.

A pixel is comparable when its first-hit face, its terminal face and its bounce count
are each uniform over its 3x3 neighbourhood in the oracle's images: a last-bit
difference in a ray cannot change such a pixel's path."""
import ctypes as C

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib
from oracle import oracle as O

from tests.conftest import scene_path
from tests import path_ref as P
from tests import path_scenes as S
from tests import post_ref as R
from tests import variant_scenes as V

pytestmark = pytest.mark.gpu

AOV_KEYS = ("albedo", "normal", "depth", "face", "material")
KEYS = AOV_KEYS + ("bounces",)
BUILT = ("box2", "hall", "tinted", "tilted", "lamp_mirror")
SHIPPED = ("box", "tir", "ball")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def scenes(gpu_available):
    """name -> (host scene, device scene, the oracle's packed scene); built once, read only."""
    out = {}
    for name in BUILT:
        src = S.scene(name)
        s = V.device_scene(src)
        out[name] = (s, s.copySceneToDevice(0).build(), V.oracle_scene(src))
    for name in SHIPPED:
        s = T.Scene(scene_path(name))
        out[name] = (s, s.copySceneToDevice(0).build(), O.load_scene(scene_path(name)))
    yield out
    for _, d, _ in out.values():
        d.close()


_REFS = {}


def oracle_path(scenes, name, w, h, cap):
    key = (name, w, h, cap)
    if key not in _REFS:
        _REFS[key] = P.oracle_aov_path(scenes[name][2], w, h, cap)
    return _REFS[key]


def render(scenes, name, w, h, cap, **kw):
    s, d, _ = scenes[name]
    return T.PathTracer("", w, h, 0).renderAOVPath(d, s.m_camera, cap, **kw)


@pytest.mark.parametrize("name,w,h,cap", [("box2", 256, 144, 8), ("hall", 128, 72, 3), ("hall", 128, 72, 8),
                                          ("tinted", 128, 72, 3), ("tinted", 128, 72, 8), ("tilted", 128, 72, 3)])
def test_path_matches_oracle(scenes, name, w, h, cap):
    """Measured on an MI355X (max relative depth error, max normal error): see DESIGN.md
    section 5 "Post-pass", the table under "Mirror-path feature buffers"."""
    gpu = render(scenes, name, w, h, cap)
    ref = oracle_path(scenes, name, w, h, cap)
    ok = P.comparable(ref)
    followed = ok & (ref["bounces"] > 0)
    print(f"{name} {w}x{h} cap {cap}: comparable {ok.mean():.3f}, comparable followed {followed.sum()}, "
          f"bounces {np.bincount(ref['bounces'].ravel()).tolist()}")
    assert ok.mean() >= 0.7 and followed.sum() >= 300
    assert np.array_equal(gpu["bounces"][ok], ref["bounces"][ok])
    assert np.array_equal(gpu["face"][ok], ref["face"][ok])
    assert np.array_equal(gpu["material"][ok], ref["material"][ok])
    assert np.array_equal(_bits(gpu["albedo"][ok]), _bits(ref["albedo"][ok]))
    hit = ok & (ref["face"] >= 0)
    rel = np.abs(gpu["depth"][hit].astype(np.float64) - ref["depth"][hit]) / ref["depth"][hit]
    dn = np.abs(gpu["normal"][hit].astype(np.float64) - ref["normal"][hit])
    fh = followed & hit
    relf = np.abs(gpu["depth"][fh].astype(np.float64) - ref["depth"][fh]) / ref["depth"][fh]
    print(f"{name} cap {cap}: max relative depth error {rel.max():.3e} (followed pixels {relf.max():.3e}), "
          f"max normal error {dn.max():.3e}")
    assert rel.max() <= 1e-4
    assert dn.max() <= 1e-4
    miss = followed & (ref["face"] < 0)                     # left the scene after at least one mirror
    if name == "box2":
        assert miss.sum() >= 50
    if miss.any():
        assert (gpu["face"][miss] == -1).all() and (gpu["material"][miss] == -1).all()
        assert (_bits(gpu["normal"][miss]) == 0).all()
        assert (gpu["depth"][miss] > 0).all()
        relm = np.abs(gpu["depth"][miss].astype(np.float64) - ref["depth"][miss]) / ref["depth"][miss]
        assert relm.max() <= 1e-4
        # the tint product, restated: one mirror met, its base colour
        one = miss & (ref["bounces"] == 1)
        tint = P.material_table(scenes[name][2])[ref["first_material"][one], :3]
        assert np.array_equal(_bits(gpu["albedo"][one]), _bits(tint))


@pytest.mark.parametrize("name,w,h,cap", [("box", 256, 144, 0), ("hall", 128, 72, 0), ("tir", 256, 144, 8),
                                          ("ball", 256, 144, 8)])
def test_equals_render_aov_bit_for_bit(scenes, name, w, h, cap):
    """With max_bounces 0, and at 8 on the shipped scenes without a mirror: tir (diffuse walls
    around glass, which is terminal) and ball (no material at all).  box1 is none: its whitWall
    has no metallicFactor, which glTF reads as 1 (tests/test_path_scenes_cpu.py)."""
    s, d, _ = scenes[name]
    pt = T.PathTracer("", w, h, 0)
    first = pt.renderAOV(d, s.m_camera)
    st = {}
    path = pt.renderAOVPath(d, s.m_camera, cap, stats=st)
    for k in AOV_KEYS:
        assert np.array_equal(_bits(path[k]), _bits(first[k])), k
    assert (path["bounces"] == 0).all()
    assert st["followed"] == 0 and st["deepest"] == 0 and st["trace_ms"] > 0.0
    assert (first["face"] >= 0).mean() > 0.02


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_cap(scenes, cap):
    s, d, ps = scenes["hall"]
    st = {}
    gpu = render(scenes, "hall", 128, 72, cap, stats=st)
    assert gpu["bounces"].max() == cap and gpu["bounces"].min() == 0
    assert st["deepest"] == cap
    # a pixel capped at a mirror reports that mirror: its material, and a face of that material
    tab = P.material_table(ps)
    fm = R.face_material(ps, len(ps.indices) // 3)
    capped = (gpu["bounces"] == cap) & (gpu["material"] >= 0)
    on_mirror = capped & P.is_mirror(tab)[np.maximum(gpu["material"], 0)]
    assert on_mirror.sum() >= 20
    assert np.array_equal(fm[gpu["face"][on_mirror]], gpu["material"][on_mirror])
    assert (np.abs(np.linalg.norm(gpu["normal"][on_mirror], axis=-1) - 1.0) < 1e-2).all()
    # below the cap no path stops on a mirror
    below = (gpu["bounces"] < cap) & (gpu["material"] >= 0)
    assert not P.is_mirror(tab)[gpu["material"][below]].any()


def test_emitter_ends_the_path(scenes):
    s, d, ps = scenes["lamp_mirror"]
    pt = T.PathTracer("", 128, 72, 0)
    first = pt.renderAOV(d, s.m_camera)
    gpu = pt.renderAOVPath(d, s.m_camera, 8)
    lamp = first["material"] == S.emitter_ids(ps.src)[0]
    assert lamp.sum() >= 20
    assert (gpu["bounces"][lamp] == 0).all()
    assert np.array_equal(gpu["face"][lamp], first["face"][lamp])
    assert (gpu["bounces"] > 0).sum() >= 300                # the scene's own mirror is still followed


def test_statistics_over_wrapping_counter_slots(scenes):
    """257 x 241 is 17 x 16 = 272 tiles: the 256 counter slots wrap."""
    st = {}
    gpu = render(scenes, "hall", 257, 241, 8, stats=st)
    assert (gpu["bounces"] > 0).sum() >= 1000
    assert st["followed"] == int((gpu["bounces"] > 0).sum())
    assert st["deepest"] == int(gpu["bounces"].max())


def _with_sentinel(w, h):
    """Each output with one more row past its end, filled with a sentinel."""
    bufs = {k: np.full((h + 1, w) + ((3,) if ch == 3 else ()), -7.0 if dt == "float32" else -77, dt)
            for k, (ch, dt) in dict(T.AOV_LAYOUT, bounces=(1, "int32")).items()}
    return bufs, {k: v[:h] for k, v in bufs.items()}


@pytest.mark.parametrize("w,h", [(50, 38), (17, 16), (1, 1)])
def test_sizes_write_every_pixel_and_nothing_else(scenes, w, h):
    bufs, views = _with_sentinel(w, h)
    render(scenes, "hall", w, h, 3, out=views)
    for k in KEYS:
        sentinel = -7.0 if bufs[k].dtype == np.float32 else -77
        assert (bufs[k][h] == sentinel).all(), k
        assert not (views[k] == sentinel).any(), k
    ref = oracle_path(scenes, "hall", w, h, 3)
    ok = P.comparable(ref)
    assert np.array_equal(views["bounces"][ok], ref["bounces"][ok])
    assert np.array_equal(views["face"][ok], ref["face"][ok])


def test_device_outputs_equal_host_outputs(scenes):
    import torch
    w, h = 128, 72
    host = render(scenes, "tinted", w, h, 8)
    dev = torch.device("cuda", 0)
    out = {"albedo": torch.full((h, w, 3), -7.0, device=dev), "normal": torch.full((h, w, 3), -7.0, device=dev),
           "depth": torch.full((h, w), -7.0, device=dev),
           "face": torch.full((h, w), -77, dtype=torch.int32, device=dev),
           "material": torch.full((h, w), -77, dtype=torch.int32, device=dev),
           "bounces": torch.full((h, w), -77, dtype=torch.int32, device=dev)}
    render(scenes, "tinted", w, h, 8, out=out)
    for k in KEYS:
        assert np.array_equal(_bits(out[k].cpu().numpy()), _bits(host[k])), k


def test_nullable_outputs(scenes):
    w, h = 128, 72
    host = render(scenes, "tinted", w, h, 8)
    bounces = np.full((h, w), -77, np.int32)
    out = render(scenes, "tinted", w, h, 8, out={"bounces": bounces})
    assert set(out) == {"bounces"} and np.array_equal(bounces, host["bounces"])
    depth = np.full((h, w), -7.0, np.float32)
    render(scenes, "tinted", w, h, 8, out={"depth": depth, "albedo": None})
    assert np.array_equal(_bits(depth), _bits(host["depth"]))
    with pytest.raises(ValueError):
        render(scenes, "tinted", w, h, 8, out={"colour": depth})
    # the C entry point takes a null `out` when bounces_out is given
    s, d, _ = scenes["tinted"]
    cam = s.m_camera.to_c()
    p = _lib.AovPathParams(8, 0)
    again = np.full((h, w), -77, np.int32)
    assert T.lib().tpt_render_aov_path(d.handle, C.byref(cam), w, h, C.byref(p), None, again.ctypes.data, None) == 0
    assert np.array_equal(again, host["bounces"])


def test_deterministic(scenes):
    a = render(scenes, "hall", 128, 72, 8)
    b = render(scenes, "hall", 128, 72, 8)
    for k in KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_refusals(scenes):
    s, d, _ = scenes["hall"]
    L = T.lib()
    w, h = 32, 18
    cam = s.m_camera.to_c()
    depth = np.full((h, w), -7.0, np.float32)
    bounces = np.full((h, w), -77, np.int32)
    a = _lib.Aov(None, None, depth.ctypes.data, None, None)
    st = _lib.AovPathStats()
    good = _lib.AovPathParams(8, 0)

    def call(scene=d.handle, camera=C.byref(cam), W=w, H=h, params=C.byref(good), out=C.byref(a),
             k=bounces.ctypes.data):
        return L.tpt_render_aov_path(scene, camera, W, H, params, out, k, C.byref(st))

    def refused(rc, word):
        assert rc == 1                                     # TPT_ERR_INVALID_ARG
        assert word in L.tpt_last_error(), L.tpt_last_error()

    unbuilt = V.device_scene(S.scene("hall")).copySceneToDevice(0)
    refused(call(scene=unbuilt.handle), b"not built")
    unbuilt.close()
    refused(call(camera=None), b"camera")
    refused(call(W=0), b"frame size")
    refused(call(H=-3), b"frame size")
    refused(call(params=None), b"params")
    refused(call(params=C.byref(_lib.AovPathParams(-1, 0))), b"max_bounces")
    refused(call(params=C.byref(_lib.AovPathParams(65, 0))), b"max_bounces")
    refused(call(params=C.byref(_lib.AovPathParams(8, 1))), b"flags")
    none = _lib.Aov()
    refused(call(out=C.byref(none), k=None), b"every pointer")
    refused(call(out=None, k=None), b"every pointer")
    assert (depth == -7.0).all() and (bounces == -77).all()  # no refused call wrote anything
    assert call(params=C.byref(_lib.AovPathParams(64, 0))) == 0   # the range's upper end is accepted
    assert not (depth == -7.0).any() and bounces.max() <= 64


def test_denoise_with_path_guides_end_to_end(scenes):
    """box 96 x 54, 8 spp, seed 42, against the library's own 2,048-spp frame; tpt_denoise at
    DENOISE_DEFAULTS with first-hit and with mirror-path guides.  The render is bit-identical
    to the oracle's, so the CPU figures (tools/aov_path_quality.py; DESIGN.md section 5
    "Post-pass") carry over: MSE over the pixels whose first hit is the mirror 0.0713 with path
    guides against 0.0934, ratio 0.763; the bound is 0.9."""
    s, d, ps = scenes["box"]
    w, h = 96, 54
    pt = T.PathTracer("", w, h, 0)
    noisy = np.zeros((h, w, 3), np.float32)
    truth = np.zeros((h, w, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, 8, seed=42, max_depth=8, radiance=noisy)
    pt.doTrace(d, s.m_camera, None, 2048, seed=42, max_depth=8, radiance=truth)
    first = pt.renderAOV(d, s.m_camera)
    st = {}
    path = pt.renderAOVPath(d, s.m_camera, stats=st)
    mirror = (first["material"] >= 0) & P.is_mirror(P.material_table(ps))[np.maximum(first["material"], 0)]
    assert mirror.sum() >= 100 and st["followed"] == mirror.sum() and ((path["bounces"] > 0) == mirror).all()
    den_first = pt.denoise(d, noisy, first)
    den_path = pt.denoise(d, noisy, path)
    mse = lambda x, m: float(((x.astype(np.float64) - truth)[m] ** 2).mean())
    everywhere = np.ones((h, w), bool)
    mf, mp = mse(den_first, mirror), mse(den_path, mirror)
    ff, fp = mse(den_first, everywhere), mse(den_path, everywhere)
    print(f"mirror pixels {mirror.sum()}: noisy {mse(noisy, mirror):.4f}, first-hit guides {mf:.4f}, path guides "
          f"{mp:.4f} (ratio {mp / mf:.3f}); whole frame {ff:.5f} -> {fp:.5f}")
    assert mp / mf <= 0.9
    assert fp <= ff
    # outside the mirror's reach the guides are the same, and so is the filter's input
    same = ~mirror
    for k in AOV_KEYS:
        assert np.array_equal(_bits(path[k][same]), _bits(first[k][same])), k
