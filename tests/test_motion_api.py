"""Moving objects without a GPU: tpt_motion_matrices against numpy float64, the new symbols
as the library, the ctypes layer and the CLI declare them, and the numpy restatement of
tpt_temporal_motion (tests/motion_ref.py) where nothing moves."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import tinypathtracer_amd as T
from tinypathtracer_amd import _lib

from tests.conftest import ROOT, scene_path
from tests import motion_ref as MR
from tests import temporal_ref as TR
from tests import test_gpu_motion as M

EXE = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
BOX = scene_path("box")

REST = MR.translation((0.3, -1.2, 2.0)) @ MR.rotation_y(25.0)
SINGULAR = np.diag([1.0, 0.0, 1.0, 1.0])
PROJECTIVE = np.eye(4)
PROJECTIVE[3, 0] = 0.1
# name -> (M', M, the flag)
PAIRS = {
    "translation": (REST, MR.translation((0.11, 0.03, -0.4)) @ REST, MR.TRACKED),
    "rotation_y": (REST, MR.rotation_y(4.0, centre=(0.05, 0.0, -2.5)) @ REST, MR.TRACKED),
    "rotation_translation_scale": (REST, MR.translation((1.0, 0.5, -0.25)) @ MR.rotation_y(-33.0, (0.2, 0.1, 0.3), 1.7) @ REST,
                                   MR.TRACKED),
    "bit_equal": (REST, REST, MR.IDENTITY),
    "bit_equal_singular": (SINGULAR, SINGULAR, MR.IDENTITY),
    "singular": (REST, SINGULAR, MR.UNTRACKED),
    "projective": (REST, PROJECTIVE @ REST, MR.UNTRACKED),
    "projective_previous": (PROJECTIVE @ REST, REST, MR.UNTRACKED),
    "singular_previous": (SINGULAR, REST, MR.UNTRACKED),   # D exists, G = (D_lin)^-T does not
}


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_motion_matrices_against_numpy():
    """D and G within 4 float32 ulp of the rounded float64 result, entry by entry; flags and
    the return value exact; exact unit matrices for a bit-equal pair.  An entry that cancels
    to (nearly) nothing has no ulp of its own to speak of -- two float64 evaluations of it
    differ by the rounding of its terms, 2^-53 of the row's largest entry each -- so an entry
    is measured with the ulp of at least 2^-24 of its row's largest entry."""
    names = list(PAIRS)
    prev = np.stack([MR.col_major(PAIRS[k][0]) for k in names])
    cur = np.stack([MR.col_major(PAIRS[k][1]) for k in names])
    D, G, flags, untracked = T.motion_matrices(prev, cur)
    Dr, Gr, fr = MR.motion_matrices_ref(prev, cur)
    assert list(flags) == [PAIRS[k][2] for k in names] == list(fr)
    assert untracked == sum(PAIRS[k][2] == MR.UNTRACKED for k in names) == 4
    for k, name in enumerate(names):
        if flags[k] == MR.IDENTITY:
            assert np.array_equal(D[k].view(np.uint32), np.eye(4, dtype=np.float32)[:3].view(np.uint32))
            assert np.array_equal(G[k].view(np.uint32), np.eye(3, dtype=np.float32).view(np.uint32))
        if flags[k] != MR.TRACKED:
            continue
        for got, ref in ((D[k], Dr[k]), (G[k], Gr[k])):
            floor = np.abs(ref).max(-1, keepdims=True) * 2.0 ** -24
            ulp = _ulp32(np.maximum(np.abs(ref), floor))
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ulp
            print(f"{name}: largest error {err.max():.2f} ulp")
            assert err.max() <= 4.0
    # D takes this frame's points to the previous frame's, G its normals
    k = names.index("rotation_translation_scale")
    mp, m = MR.mat(prev[k]), MR.mat(cur[k])
    x = np.array([0.3, -0.7, 1.9, 1.0])
    assert np.abs(D[k].astype(np.float64) @ (m @ x) - (mp @ x)[:3]).max() < 1e-5
    nl = np.array([0.36, 0.48, 0.8])
    n_cur = np.linalg.inv(m[:3, :3]).T @ nl
    n_prev = np.linalg.inv(mp[:3, :3]).T @ nl
    g = G[k].astype(np.float64) @ n_cur
    assert np.abs(g / np.linalg.norm(g) - n_prev / np.linalg.norm(n_prev)).max() < 1e-6


def test_motion_matrices_raw_layout_and_nulls():
    """24 floats per object: D's rows of four, G's rows of three, the flag's bits, zeros."""
    L = T.lib()
    prev = np.stack([MR.col_major(REST), MR.col_major(REST)])
    cur = np.stack([MR.col_major(MR.translation((1.0, 2.0, 3.0)) @ REST), MR.col_major(SINGULAR)])
    out = np.full((2, 24), -7.0, np.float32)
    assert L.tpt_motion_matrices(2, prev.ctypes.data, cur.ctypes.data, out.ctypes.data) == 1
    assert np.allclose(out[0, :12].reshape(3, 4), [[1, 0, 0, -1], [0, 1, 0, -2], [0, 0, 1, -3]], atol=1e-6)
    assert np.allclose(out[0, 12:21].reshape(3, 3), np.eye(3), atol=1e-6)
    assert list(out[:, 21].view(np.int32)) == [MR.TRACKED, MR.UNTRACKED]
    assert (out[:, 22:] == 0.0).all() and np.isfinite(out).all()
    assert L.tpt_motion_matrices(0, None, None, None) == 0
    assert L.tpt_motion_matrices(1, None, cur.ctypes.data, out.ctypes.data) == -1
    with pytest.raises(ValueError):
        T.motion_matrices(prev, cur[:1])
    assert (_lib.MOTION_TRACKED, _lib.MOTION_IDENTITY, _lib.MOTION_UNTRACKED) == (0, 1, 2)


def test_symbols_exported():
    L = T.lib()
    sigs = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert len(sigs["tpt_motion_matrices"][1]) == 4 and L.tpt_motion_matrices.restype is C.c_int32
    assert len(sigs["tpt_scene_set_transforms"][1]) == 5 and L.tpt_scene_set_transforms.restype is C.c_int
    assert len(sigs["tpt_temporal_motion"][1]) == 11 and L.tpt_temporal_motion.restype is C.c_int
    assert len(sigs["tpt_temporal"][1]) == 10              # as it was
    header = open(os.path.join(ROOT, "include", "tpt.h")).read()
    assert "TPT_FLAG_ACCUMULATE) does not survive" in header
    assert hasattr(T.DeviceScene, "set_transforms") and callable(T.motion_matrices)


def test_null_handles_fail_cleanly():
    """No device is needed to be refused."""
    L = T.lib()
    m = MR.col_major(REST)
    assert L.tpt_scene_set_transforms(None, 0, 1, m.ctypes.data, None) == 1
    assert b"scene" in L.tpt_last_error()
    cam = T.Camera(np.eye(4, dtype=np.float32).reshape(16), 0.8, 1.0).to_c()
    buf = np.full((4, 4, 3), -7.0, np.float32)
    z = np.zeros((4, 4), np.float32)
    i = np.zeros((4, 4), np.int32)
    g = _lib.Aov(buf.ctypes.data, buf.ctypes.data, z.ctypes.data, i.ctypes.data, i.ctypes.data)
    p = _lib.TemporalParams(0.1, 0.1, 0.9, 32, _lib.TEMPORAL_DEMODULATE)
    out = np.full((4, 4, 3), -7.0, np.float32)
    mv = np.full((4, 4, 2), -7.0, np.float32)
    assert L.tpt_temporal_motion(None, C.byref(cam), buf.ctypes.data, C.byref(g), C.byref(p), out.ctypes.data, None,
                                 None, mv.ctypes.data, None, None) == 1
    assert b"history" in L.tpt_last_error()
    assert (out == -7.0).all() and (mv == -7.0).all()


def test_cli_usage_names_the_motion_options():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--move OBJ DX DY DZ" in r.stderr and "--spin OBJ DEG" in r.stderr


@pytest.mark.parametrize("args,words", [
    (["--frames", "4", "--move", "5", "0.1", "0", "0"], ("--move", "--temporal")),
    (["--frames", "4", "--spin", "5", "3"], ("--spin", "--temporal")),
    (["--temporal", "--move", "5", "0.1", "0", "0"], ("--move", "--frames")),
    (["--frames", "4", "--temporal", "--progressive", "--move", "5", "0.1", "0", "0"], ("--move", "--progressive")),
    (["--frames", "4", "--temporal", "--progressive", "--spin", "5", "3"], ("--spin", "--progressive")),
])
def test_cli_refuses(tmp_path, args, words):
    """--move and --spin need --frames and --temporal and are refused with --progressive,
    before anything is loaded or rendered."""
    r = subprocess.run([EXE, BOX, "--out", str(tmp_path / "x")] + args, capture_output=True, text=True)
    assert r.returncode == 2
    assert all(w in r.stderr for w in words), r.stderr
    assert not list(tmp_path.iterdir())


def test_object_indices_used_by_the_tests():
    """Objects are the glTF file's mesh nodes in node order: box's ball1 is object 5, box2's
    back, Cube and Cube.001 are objects 4, 6 and 7."""
    def names(scene):
        with open(scene_path(scene)) as f:
            return [n.get("name") for n in json.load(f)["nodes"] if "mesh" in n]
    assert names("box")[M.BALL1] == "ball1"
    assert [names("box2")[o] for o in MR.PATCH_OBJECTS] == ["back", "Cube", "Cube.001"]
    assert (M.BACK, M.CUBE, M.CUBE1) == MR.PATCH_OBJECTS
    assert len(names("box2")) == M.CARRIER.n_objects == 8 and M.CARRIER.n_faces == 36


@pytest.mark.parametrize("demodulate", [False, True])
def test_reference_with_nothing_moving_is_temporal_ref(demodulate):
    """All objects static: temporal_ref.temporal_ref on the same inputs, array for array, over
    three frames of a moving camera; the guides are temporal_ref's too, and the motion is the
    camera's alone."""
    cams = [M.STATIC, M.G.CAMERAS["yaw_translate"], M.G.THIRD]
    seq = M.sequence([(c, {}, seed) for c, seed in zip(cams, (101, 202, 303))])
    params = dict(M.PARAMS, demodulate=demodulate)
    mine = M.reference(seq, params)
    state = None
    for k, (cam, vt, (rad, aov)) in enumerate(seq):
        theirs = TR.synthetic_guides(cam, M.W, M.H)
        for key in ("normal", "depth", "material"):
            assert np.array_equal(aov[key], theirs[key])
        assert np.array_equal(aov["face"] >= 0, aov["material"] >= 0)
        ref = TR.temporal_ref(state, cam, rad, aov, **params)
        state = ref["state"]
        for key in ("out", "variance", "history_len", "reprojected", "decidable"):
            assert np.array_equal(mine[k][key], ref[key]), (k, key)
        for key in ("C", "N", "M1", "M2", "n", "z", "m"):
            assert np.array_equal(mine[k]["state"][key], ref["state"][key]), (k, key)
    assert (mine[0]["motion"] == 0.0).all() and np.abs(mine[1]["motion"]).max() > 0.5
    assert mine[2]["reprojected"].any() and (~mine[2]["reprojected"]).any()


def test_reference_follows_a_translated_patch():
    """A property of the restatement itself: under a static camera the moved strip's motion
    vectors are minus its step in pixels, the static patches' are zero."""
    seq, params, refs = M.case("strip_translate")
    aov = seq[1][2][1]
    faces = MR.patch_faces(M.CARRIER)
    strip, rest = aov["face"] == faces[MR.STRIP], (aov["face"] >= 0) & (aov["face"] != faces[MR.STRIP])
    mv = refs[1]["motion"]
    assert np.abs(mv[rest]).max() < 1e-6
    sw, sh, _, _ = (float(v) for v in TR.sensor(0.8, M.ASPECT))
    step = -np.array([0.08 / 2.5 / sw * M.W, 0.075 / 2.5 / sh * M.H])
    assert np.abs(mv[strip] - step).max() < 2e-3           # the snap moves a coordinate by up to 2^-10
