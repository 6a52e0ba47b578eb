"""GPU: tpt_render_adaptive through the C++ host and the CLI (include/tpt.hpp
PathTracer::doTraceAdaptive, which tpt_render --adaptive calls) against the Python host:
the same frame bit for bit, <out>_spp.pfm the tiles' sample counts per pixel, the JSON line
the call's statistics, and --denoise / --svgf on the adaptive frame as on a fixed-spp one."""
import json
import os
import subprocess

import numpy as np
import pytest

import tinypathtracer_amd as T
from tests import adaptive_ref as R
from tests.conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tinypathtracer_amd", "tpt_render")
W, H, SEED, TARGET = 37, 29, 42, R.CASES["box_37x29"][5]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _read_pfm(path, w, h, ch):
    raw = open(path, "rb").read()
    assert raw.startswith(b"%s\n%d %d\n-1.0\n" % (b"PF" if ch == 3 else b"Pf", w, h))
    a = np.frombuffer(raw[-w * h * 4 * ch:], np.float32)
    return a.reshape(h, w, 3) if ch == 3 else a.reshape(h, w)


@pytest.fixture(scope="module")
def python_host(gpu_available):
    """The Python host's adaptive frame of box at 37x29 (the case tests/test_gpu_adaptive.py holds
    to the reference), with the scene and tracer the filters below run on."""
    s = T.Scene(scene_path("box"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    tx, ty = R.tiles_of(W, H)
    rad = np.zeros((H, W, 3), np.float32)
    spp = np.zeros((ty, tx), np.int32)
    st = pt.doTraceAdaptive(d, s.m_camera, None, min_spp=R.MIN_SPP, max_spp=R.MAX_SPP, target=TARGET, seed=SEED,
                            max_depth=R.DEPTH, radiance=rad, tile_spp=spp)
    yield s, d, pt, rad, spp, st
    d.close()


def test_cli_adaptive_is_the_python_hosts_frame(python_host, tmp_path):
    s, d, pt, rad, spp, st = python_host
    out = str(tmp_path / "f")
    cmd = [EXE, scene_path("box"), "--width", str(W), "--height", str(H), "--seed", str(SEED), "--depth", str(R.DEPTH),
           "--out", out, "--adaptive", repr(TARGET), "--min-spp", str(R.MIN_SPP), "--max-spp", str(R.MAX_SPP),
           "--denoise", "--svgf"]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=120)
    assert {p.name for p in tmp_path.iterdir()} == {"f.ppm", "f.pfm", "f_spp.pfm", "f_denoised.pfm", "f_denoised.ppm",
                                                    "f_svgf.pfm", "f_svgf.ppm"}
    got = _read_pfm(out + ".pfm", W, H, 3)
    assert np.array_equal(_bits(got), _bits(rad))
    per_pixel = np.repeat(np.repeat(spp, R.TILE, 0), R.TILE, 1)[:H, :W]
    assert len(np.unique(spp)) >= 3                        # tiles at different counts
    assert np.array_equal(_read_pfm(out + "_spp.pfm", W, H, 1), per_pixel.astype(np.float32))
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert (line["width"], line["height"], line["min_spp"], line["max_spp"]) == (W, H, R.MIN_SPP, R.MAX_SPP)
    assert line["target"] == pytest.approx(TARGET, rel=1e-6)
    assert (line["passes"], line["unconverged_tiles"], line["rays"]) == (st["passes"], st["unconverged_tiles"],
                                                                        st["traversals"])
    assert line["mean_spp"] == pytest.approx(st["samples"] / (W * H), abs=0.005)
    assert line["out"] == out + ".ppm"
    # the filters ran on the adaptive frame with the hosts' defaults
    aov = pt.renderAOV(d, s.m_camera)
    assert np.array_equal(_bits(_read_pfm(out + "_denoised.pfm", W, H, 3)), _bits(pt.denoise(d, rad.copy(), aov)))
    assert np.array_equal(_bits(_read_pfm(out + "_svgf.pfm", W, H, 3)), _bits(pt.denoiseSVGF(d, rad.copy(), aov)))
