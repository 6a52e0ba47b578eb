"""tpt_scene_refit on the device (DESIGN.md section 5 "BVH refit"): the state it leaves against
the numpy restatement (tests/refit_ref.py) and against a fresh scene built from the same arrays,
on the scenes, poses and ray sets of tests/refit_cases.py (tests/test_refit_cpu.py shows that the
ray sets hold almost no near-ties).

What a refit may answer differently from a rebuild is an exact tie only: two different triangles
at a bit-equal closest t, which the kernel resolves to the larger sorted position -- after a refit
the last full build's.  Such rays (pixels) are counted and bounded; any other difference fails.
Measured on MI355X: no tie and no other difference in any ray set, pose and mode, and no differing
pixel in the box frames."""
import os
import subprocess

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import ROOT, scene_path
from tests import deform_cases as DC
from tests import refit_cases as RC
from tests import refit_ref as RR
from tests import test_gpu_temporal as G

pytestmark = pytest.mark.gpu

F = np.float32
CASES = [(name, pose) for name in RC.SCENES for pose in RC.scene(name)["poses"] if pose != "sliver"]
MAX_TIES = 1e-3                     # of a ray set, per trace mode


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_tree(a, b):
    """Floats with == (so +0 and -0 agree), links and padding bit for bit."""
    return bool(a.shape == b.shape and (a[:, :24] == b[:, :24]).all() and
                np.array_equal(bits(a[:, 24:]), bits(b[:, 24:])))


def state(d):
    """(world vertices, world normals, nodes36, keys, main tree, emissive tree)"""
    return d.read_world() + d.read_bvh() + d.read_wide()


def same_state(a, b):
    return all(same_bits(x, y) if x.dtype != T.NODE_DTYPE else x.tobytes() == y.tobytes() for x, y in zip(a, b))


def frame(d, cam, w=16, h=16, spp=4, seed=7, flags=0):
    rad = np.zeros((h, w, 3), F)
    T.PathTracer("", w, h, 0).doTrace(d, cam, None, spp, seed=seed, radiance=rad, flags=flags)
    return rad


def built(name, vertices=None, normals=None):
    s = RC.make(name, vertices, normals)
    return s, s.copySceneToDevice(0).build()


def leaf_boxes(name, d):
    """The exact min/max of every triangle's read_world corners, by sorted position."""
    wv, _ = d.read_world()
    nodes, _ = d.read_bvh()
    nint = (len(nodes) - 1) // 2
    tri = RC.scene(name)["indices"].reshape(-1, 3).astype(np.int64)[nodes["a"][nint:]]
    c = wv[tri]                                              # [positions, 3 corners, 3]
    return np.concatenate([c.min(1), c.max(1)], -1).astype(F)


@pytest.fixture(scope="module")
def posed(gpu_available):
    """Per (scene, pose), made once and then only read: the scene built at rest, posed and refitted;
    the state before the pose; the refit's stats; a fresh scene built from the posed arrays."""
    made = {}

    def get(name, pose):
        if (name, pose) not in made:
            v, n = RC.scene(name)["poses"][pose]
            s, d = built(name)
            pre = state(d)
            d.set_vertices(0, v, n)
            st = d.refit()
            made[(name, pose)] = (s, d, pre, st, built(name, v, n)[1])
        return made[(name, pose)]

    yield get
    for _, d, _, _, f in made.values():
        d.close()
        f.close()


def check_refitted_state(name, d, pre, st, fresh):
    wv, wn, nodes, keys, main, emit = state(d)
    fwv, fwn = fresh.read_world()
    assert same_bits(wv, fwv) and same_bits(wn, fwn)
    for word in ("parent", "a", "b"):                        # the topology is the pre-deformation build's
        assert np.array_equal(nodes[word], pre[2][word])
    assert np.array_equal(keys, pre[3])                      # (stale, and said to be)
    nint = (len(nodes) - 1) // 2
    lb = leaf_boxes(name, d)
    got = np.concatenate([nodes["bmin"], nodes["bmax"]], -1)
    assert same_bits(got[nint:], lb)
    assert (got == RR.refit_lbvh(nodes, lb)).all()
    assert same_tree(main, RR.refit_wide(pre[4], lb, nint, 0))
    assert len(emit) == len(pre[5])
    if len(emit):
        assert same_tree(emit, RR.refit_wide(pre[5], lb, nint, len(main)))
    want = RR.cost(main)
    print(f"{name}: cost {st['cost']:.6f} (numpy {want:.6f}), built {st['cost_built']:.6f}, {st['launches']} launches, "
          f"{len(main)} + {len(emit)} nodes, {st['ms']:.3f} ms")
    assert abs(st["cost"] - want) <= 1e-9 * want
    assert abs(st["cost_built"] - RR.cost(pre[4])) <= 1e-9 * want
    assert st["rebuilt"] == 0 and st["launches"] > 0


def compare_rays(name, pose, d, fresh, modes=(0, 1, 2, 3)):
    keep = RC.usable(name, pose)
    o, dd = (a[keep] for a in RC.rays(name))
    hits = 0
    for mode in modes:
        h1, t1, uv1 = d.trace_rays(o, dd, mode)
        h2, t2, uv2 = fresh.trace_rays(o, dd, mode)
        if mode == 2:                                        # any hit: the verdict alone
            assert np.array_equal(h1 >= 0, h2 >= 0)
            continue
        t_same = bits(t1) == bits(t2)
        same = (h1 == h2) & t_same & (bits(uv1) == bits(uv2)).all(-1)
        tie = ~same & t_same & (h1 != h2)
        print(f"{name} {pose} mode {mode}: {len(o)} rays, {int((h1 >= 0).sum())} hits, {int(tie.sum())} ties, "
              f"{int((~same & ~tie).sum())} other differences")
        assert (same | tie).all()
        assert tie.sum() <= MAX_TIES * len(o)
        hits += int((h1 >= 0).sum())
    assert hits > 0


# ---- 1. the state after a refit, 3. rays ----

@pytest.mark.parametrize("name,pose", CASES)
def test_state_after_refit(posed, name, pose):
    s, d, pre, st, fresh = posed(name, pose)
    check_refitted_state(name, d, pre, st, fresh)
    _, _, nodes, _, main, emit = state(d)
    assert not same_tree(main, pre[4])                       # the pose moved boxes
    if name == "sheet_emit":
        assert len(RR.levels(emit, len(main))) - 1 >= 2      # a multi-level emissive tree
    if name != "two":
        assert len(RR.levels(main, 0)) - 1 >= 3


@pytest.mark.parametrize("name,pose", CASES)
def test_rays_equal_a_fresh_scene(posed, name, pose):
    s, d, pre, st, fresh = posed(name, pose)
    compare_rays(name, pose, d, fresh)


# ---- 2. identity and round trip ----

@pytest.mark.parametrize("name", RC.SCENES)
def test_identity_and_round_trip(gpu_available, name):
    sc = RC.scene(name)
    s, d = built(name)
    want = state(d) + (frame(d, s.m_camera),)
    d.set_vertices(0, sc["vertices"], sc["normals"])         # bit-identical data
    st = d.refit()
    assert same_state(state(d), want[:6]) and same_bits(frame(d, s.m_camera), want[6])
    assert st["rebuilt"] == 0 and st["cost"] == st["cost_built"] and st["cost"] > 0
    pose = next(iter(sc["poses"]))
    d.set_vertices(0, *sc["poses"][pose])
    moved = d.refit()
    assert moved["cost"] != moved["cost_built"] and moved["cost_built"] == st["cost_built"]
    d.set_vertices(0, sc["vertices"], sc["normals"])
    back = d.refit()
    assert same_state(state(d), want[:6]) and same_bits(frame(d, s.m_camera), want[6])   # nothing accumulates
    assert back["rebuilt"] == 0 and back["cost"] == back["cost_built"] == st["cost"]
    d.close()


# ---- 4. slivers and the cull slack ----

@pytest.mark.parametrize("name", ["sheet", "sheet_emit"])
def test_slivers_come_and_go(gpu_available, name):
    sc = RC.scene(name)
    s, d = built(name)
    v, n = sc["poses"]["sliver"]
    d.set_vertices(0, *sc["poses"]["bulge"])
    assert d.refit()["slivers"] == 0
    d.set_vertices(0, v, n)
    st = d.refit()
    assert st["rebuilt"] == 0 and st["slivers"] >= 1
    fresh = built(name, v, n)[1]
    compare_rays(name, "sliver", d, fresh, modes=(1, 3))
    fresh.close()
    d.set_vertices(0, *sc["poses"]["bulge"])                 # the reverse pose
    assert d.refit()["slivers"] == 0
    d.close()


def test_cull_slack_after_a_scaling(gpu_available):
    """The sheet's object scaled by 64 through set_transforms: cull_eps is scene_build's formula
    over the world coordinates the triangle records hold -- 4 ulps of a float below 2^ex, max < 2^ex."""
    s, d = built("sheet")
    before = d.refit()["cull_eps"]
    m = np.diag([64.0, 64.0, 64.0, 1.0]).astype(F).T.reshape(1, 16)
    d.set_transforms(0, m)
    st = d.refit()
    wv, _ = d.read_world()
    tri = RC.scene("sheet")["indices"].reshape(-1, 3).astype(np.int64)
    v0 = wv[tri[:, 0]].astype(np.float64)
    e1 = (wv[tri[:, 1]] - wv[tri[:, 0]]).astype(np.float64)  # float32 edges, as the records hold them
    e2 = (wv[tri[:, 2]] - wv[tri[:, 0]]).astype(np.float64)
    top = max(np.abs(v0).max(), np.abs(v0 + e1).max(), np.abs(v0 + e2).max())
    _, ex = np.frexp(top)
    assert top > 100 and st["cull_eps"] == float(F(np.ldexp(4.0, int(ex) - 24))) and st["cull_eps"] > before > 0
    assert st["rebuilt"] == 0
    fresh = s.copySceneToDevice(0)
    fresh.set_transforms(0, m).build()
    assert same_bits(wv, fresh.read_world()[0])
    fresh.close()
    d.close()


# ---- 5. feature buffers and the temporal pass ----

def test_feature_buffers_and_temporal_deform(posed):
    s, d, pre, st, fresh = posed("sheet", "bulge")
    w, h = DC.W, DC.H
    pt = T.PathTracer("", w, h, 0)
    cam = G._cam(DC.STATIC)
    a, b = pt.renderAOV(d, cam), pt.renderAOV(fresh, cam)
    tie = (bits(a["depth"]) == bits(b["depth"])) & (a["face"] != b["face"])
    assert tie.mean() <= 0.01
    for k in ("albedo", "normal", "depth", "face", "material"):
        assert np.array_equal(bits(a[k])[~tie], bits(b[k])[~tie]), k
    assert (a["face"] >= 0).sum() > 400
    # two frames of tpt_temporal_deform: rest, then the bulge -- by a build and by a refit
    outs = {}
    for how in ("build", "refit"):
        s2, d2 = built("sheet")
        hist = T.History(d2, w, h)
        per = []
        for k, pose in enumerate((None, "bulge")):
            if pose is not None:
                d2.set_vertices(0, *RC.scene("sheet")["poses"][pose])
                if how == "build":
                    d2.build()
                else:
                    assert d2.refit()["rebuilt"] == 0
            aov = pt.renderAOV(d2, cam)
            rad, _ = DC.colours(aov, 101 + k)
            mv = np.full((h, w, 2), -3.0, F)
            per.append(G.run(pt, hist, DC.STATIC, rad, aov, deform=True, motion_out=mv, demodulate=True, **DC.PARAMS)[:3]
                       + (mv, aov["face"]))
        hist.close()
        d2.close()
        outs[how] = per
    for x, y in zip(outs["build"], outs["refit"]):
        ok = x[4] == y[4]                                    # (the ties' pixels name another face)
        assert ok.mean() >= 0.99
        for p, q in zip(x[:4], y[:4]):
            assert np.array_equal(bits(p)[ok], bits(q)[ok])
    assert (outs["refit"][1][2] == 2.0).sum() > 400          # the refitted frame found its history


# ---- 6. frames ----

@pytest.mark.parametrize("flags", [0, _lib.FLAG_REF_ORDER], ids=["ordered", "ref_order"])
def test_box_frames_equal_a_rebuild(posed, flags):
    """box at 64 x 36, 8 spp, a fixed seed, ball1 waved: the refitted scene's frame is the rebuilt
    scene's bit for bit (TPT_FLAG_REF_ORDER walks `inner`)."""
    s, d, pre, st, fresh = posed("box", "wave1")
    a = frame(d, s.m_camera, 64, 36, 8, 42, flags)
    b = frame(fresh, s.m_camera, 64, 36, 8, 42, flags)
    print(f"box flags {flags}: {int((bits(a) != bits(b)).any(-1).sum())} differing pixels")
    assert same_bits(a, b) and a.max() > 0


# ---- 7. fallbacks ----

def one_triangle():
    v = np.array([[-1.0, -1.0, -3.0], [1.0, -1.0, -3.0], [0.0, 1.0, -3.0]], F)
    n = np.tile(np.array([0.0, 0.0, 1.0], F), (3, 1))
    eye = np.eye(4, dtype=F).reshape(1, 16)
    from tests import variant_scenes as VS
    return T.Scene.from_arrays(np.arange(3, dtype=np.uint32), v, n, np.array([[0, 0]], np.int32), eye, eye.copy(),
                               np.stack([VS.material_row((0.8, 0.6, 0.4))]))


def test_refit_on_a_never_built_scene(gpu_available):
    s, fresh = built("sheet")
    d = s.copySceneToDevice(0)
    st = d.refit()
    assert st["rebuilt"] == 1 and same_state(state(d), state(fresh))
    assert st["cost"] == st["cost_built"] > 0
    d.close()
    fresh.close()


def test_refit_after_a_superseded_asynchronous_build(gpu_available):
    v, n = RC.scene("sheet")["poses"]["half"]
    s = RC.make("sheet")
    d = s.copySceneToDevice(0)
    d.build(asynchronous=True)
    d.set_vertices(0, v, n)                                  # supersedes it before its trees are uploaded
    st = d.refit()
    fresh = built("sheet", v, n)[1]
    assert st["rebuilt"] == 1 and same_state(state(d), state(fresh))
    d.close()
    fresh.close()


def test_refit_on_one_triangle(gpu_available):
    s = one_triangle()
    d = s.copySceneToDevice(0).build()
    fresh = s.copySceneToDevice(0).build()
    d.set_vertices(0, np.asarray(s.vertices, F))
    st = d.refit()
    assert st["rebuilt"] == 1 and same_state(state(d), state(fresh))
    d.close()
    fresh.close()


def test_refit_with_a_nan_vertex(gpu_available):
    sc = RC.scene("sheet")
    v = sc["vertices"].copy()
    v[40, 1] = np.nan                                        # a middle corner of eight triangles (often their second)
    s, d = built("sheet")
    d.set_vertices(0, v, sc["normals"])
    st = d.refit()
    fresh = built("sheet", v, sc["normals"])[1]
    assert st["rebuilt"] == 1 and same_state(state(d), state(fresh))   # as tpt_scene_build leaves it
    d.set_vertices(0, sc["vertices"], sc["normals"])         # and the scene recovers
    d.refit()
    clean = built("sheet")[1]
    assert same_bits(frame(d, s.m_camera), frame(clean, s.m_camera))
    for x in (d, fresh, clean):
        x.close()


def test_refit_finishes_a_pending_build_first(gpu_available):
    v, n = RC.scene("sheet")["poses"]["bend"]
    s = RC.make("sheet")
    d = s.copySceneToDevice(0)
    d.set_vertices(0, v, n)
    d.build(asynchronous=True)                               # pending, not superseded
    st = d.refit()
    fresh = built("sheet", v, n)[1]
    assert st["rebuilt"] == 0 and st["launches"] > 0 and st["cost"] == st["cost_built"]
    assert same_state(state(d), state(fresh))
    d.close()
    fresh.close()


def test_set_transforms_alone_then_refit(gpu_available):
    """The sheet's object moved by a matrix: the state as in test_state_after_refit, the rays as in
    test_rays_equal_a_fresh_scene."""
    s, d = built("sheet")
    pre = state(d)
    m = RC.scene("sheet")["matrices"]["turned"][:1]
    d.set_transforms(0, m)
    st = d.refit()
    fresh = s.copySceneToDevice(0)
    fresh.set_transforms(0, m).build()
    check_refitted_state("sheet", d, pre, st, fresh)
    assert not same_tree(d.read_wide()[0], pre[4])
    compare_rays("sheet", "turned", d, fresh)
    d.close()
    fresh.close()


# ---- 8. the CLI ----

def test_cli_refit_writes_the_same_bytes(gpu_available, tmp_path):
    exe = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
    files = {}
    for how, extra in (("build", []), ("refit", ["--refit"])):
        out = tmp_path / how
        out.mkdir()
        r = subprocess.run([exe, scene_path("box"), "--width", "48", "--height", "27", "--spp", "8", "--seed", "5",
                            "--frames", "4", "--wave", "3", "0.05", "--temporal", "--out", str(out / "f")] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        files[how] = {p.name: p.read_bytes() for p in sorted(out.iterdir())}
        lines = [l for l in r.stderr.splitlines() if "refit" in l]
        assert len(lines) == (3 if extra else 0), r.stderr   # one line per frame after the first
        assert all("cost" in l and " ms" in l and "rebuilt" not in l for l in lines)
    assert files["build"] and files["build"].keys() == files["refit"].keys()
    for name in files["build"]:
        assert files["build"][name] == files["refit"][name], name
