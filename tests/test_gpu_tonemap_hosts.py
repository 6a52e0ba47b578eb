"""GPU: tpt_tonemap through the C++ host and the CLI (include/tpt.hpp PathTracer::tonemap and
Exposure, which tpt_render --tonemap calls) against the Python host: the printed scales and
<out>_display.ppm are the Python host's for the same chain, and every other file has the bytes it
has without the new options."""
import os
import re
import subprocess

import numpy as np
import pytest

import tinypathtracer_amd as T
from tests.conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
W, H, SEED, SPP = 64, 48, 42, 8


def _read_ppm(path, w, h):
    raw = open(path, "rb").read()
    assert raw.startswith(b"P6\n%d %d\n255\n" % (w, h))
    return np.frombuffer(raw[-w * h * 3:], np.uint8).reshape(h, w, 3)        # R, G, B; row 0 = top


def _cli(tmp_path, name, options):
    out = tmp_path / name
    out.mkdir()
    r = subprocess.run([EXE, scene_path("box"), "--width", str(W), "--height", str(H), "--seed", str(SEED), "--spp",
                        str(SPP), "--out", str(out / "f")] + options, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return {p.name: p.read_bytes() for p in sorted(out.iterdir())}, r.stderr, str(out / "f")


def _same_but_display(with_, without):
    assert set(with_) == set(without) | {"f_display.ppm"} and "f_display.ppm" not in without
    for name in without:
        assert with_[name] == without[name], name


def test_cli_frames_through_one_exposure_are_the_python_hosts(gpu_available, tmp_path):
    chain = ["--frames", "3", "--temporal"]
    files, err, out = _cli(tmp_path, "with", chain + ["--auto-exposure", "--adapt", "0.5", "--tonemap", "aces", "--srgb"])
    plain, _, _ = _cli(tmp_path, "without", chain)
    _same_but_display(files, plain)
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    hist, x = T.History(d, W, H), T.Exposure(d)
    rad, acc = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    fb = np.full((H, W, 4), 255, np.uint8)
    scales = []
    for i in range(3):
        pt.doTrace(d, s.m_camera, None, SPP, seed=SEED + i, radiance=rad)
        pt.temporal(hist, s.m_camera, rad, pt.renderAOV(d, s.m_camera), out=acc)
        st = {}
        pt.tonemap(d, acc, exposure=x, bgra=fb, stats=st, op="aces", transfer="srgb", auto=True, rate=0.5)
        scales.append((st["scale"], st["log2_scale"]))
    printed = re.findall(r"frame (\d+): exposure scale (\S+) \(log2 (\S+)\)", err)
    assert [int(p[0]) for p in printed] == [0, 1, 2]
    assert [(np.float32(p[1]), np.float32(p[2])) for p in printed] == [(np.float32(a), np.float32(b)) for a, b in scales]
    assert len({sc for sc, _ in scales}) == 3                              # (it adapts: three different scales)
    assert np.array_equal(_read_ppm(out + "_display.ppm", W, H), fb[..., 2::-1])
    x.close()
    hist.close()
    d.close()


def test_cli_single_frame_maps_the_filtered_frame(gpu_available, tmp_path):
    files, err, out = _cli(tmp_path, "with", ["--denoise", "--tonemap", "--ev", "1", "--gamma", "2.2", "--dither"])
    plain, _, _ = _cli(tmp_path, "without", ["--denoise"])
    _same_but_display(files, plain)
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    rad = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, SPP, seed=SEED, radiance=rad)
    clean = pt.denoise(d, rad, pt.renderAOV(d, s.m_camera))
    fb = np.full((H, W, 4), 255, np.uint8)
    pt.tonemap(d, clean, bgra=fb, op="reinhard", transfer="gamma", gamma=2.2, ev=1.0, dither=True)
    assert "exposure scale 2 (log2 1)" in err
    assert np.array_equal(_read_ppm(out + "_display.ppm", W, H), fb[..., 2::-1])
    d.close()
