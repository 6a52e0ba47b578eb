#!/usr/bin/env python3
"""Quality of the variance-guided filter's defaults, on the CPU alone (DESIGN.md section
5 "Post-pass"): the oracle renders box at 96x54 as eight frames of 8 spp (seeds 1..8,
the camera yawing 1 degree per frame) and at 2,048 spp from the last camera; the numpy
references accumulate the frames (tests/temporal_ref.py, the hosts' defaults) and
filter the result with the plain a-trous filter (tests/post_ref.py, DENOISE_DEFAULTS)
and with the variance-guided one (tests/svgf_ref.py, SVGF_DEFAULTS, by the temporal
pass's variance and history length).  Prints the MSE against the 2,048-spp frame of
each, then the same for the last 8-spp frame alone (no temporal input: the spatial
estimate everywhere).  --sweep tries other sigma_lum."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import post_ref as R  # noqa: E402
from tests import svgf_ref as SR  # noqa: E402
from tests import temporal_ref as TR  # noqa: E402
from tinypathtracer_amd import Camera, DENOISE_DEFAULTS, SVGF_DEFAULTS, TEMPORAL_DEFAULTS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=54)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--yaw", type=float, default=1.0)
    ap.add_argument("--truth-spp", type=int, default=2048)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    ps = O.load_scene(a.scene)
    W, H = a.width, a.height
    base = Camera(np.asarray(ps.src.camera_c2w, np.float32), float(ps.src.vfov), float(ps.src.aspect))
    state = None
    for k in range(a.frames):
        c = base.yawed(a.yaw * k)
        cam = {"c2w": c.c2w, "vfov": c.vfov, "aspect": c.aspect}
        noisy, _, _ = O.render(ps, W, H, a.spp, 8, k + 1, trig_mode=1, cam=cam)
        aov = R.oracle_aov(ps, W, H, cam)
        t = TR.temporal_ref(state, cam, noisy, aov, **TEMPORAL_DEFAULTS)
        state = t["state"]
    truth, _, _ = O.render(ps, W, H, a.truth_spp, 8, 42, trig_mode=1, cam=cam)
    mse = lambda x: float(((np.asarray(x, np.float64) - truth) ** 2).mean())
    d, sv = DENOISE_DEFAULTS, SVGF_DEFAULTS
    guides = (aov["albedo"], aov["normal"], aov["depth"])
    # SVGF_DEFAULTS and TEMPORAL_DEFAULTS both demodulate: the variance is of the colour the filter works on
    var, hist = t["variance"].astype(np.float32), t["history_len"].astype(np.float32)

    def plain(x):
        return mse(R.atrous_ref(x, *guides, d["iterations"], d["sigma_color"], d["sigma_normal"], d["sigma_depth"],
                                d["demodulate"]))

    def svgf(x, v, h, **over):
        r = SR.svgf_ref(x, *guides, v, h, **dict(sv, **over))
        return mse(r["out"]), r["estimated"]

    sigmas = [sv["sigma_lum"]] + ([0.125, 0.25, 0.35, 0.5, 0.7, 1.0, 1.4, 2.0, 4.0, 8.0, 16.0] if a.sweep else [])
    for name, x, v, h in (("temporal", t["out"], var, hist), ("single frame", noisy, None, None)):
        res = {"input": name, "mse_last_frame": mse(noisy), "mse_input": mse(x), "mse_atrous": plain(x),
               "history_ge_min": float((hist >= sv["min_history"]).mean()) if h is not None else 0.0}
        res["mse_svgf"], res["estimated"] = svgf(x, v, h)
        res["svgf_over_input"] = res["mse_svgf"] / res["mse_input"]
        res["atrous_over_input"] = res["mse_atrous"] / res["mse_input"]
        print(json.dumps(res))
        for sl in sigmas[1:]:
            m, _ = svgf(x, v, h, sigma_lum=sl)
            print(json.dumps({"input": name, "sigma_lum": sl, "mse_svgf": m, "svgf_over_input": m / res["mse_input"]}))


if __name__ == "__main__":
    main()
