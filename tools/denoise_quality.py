#!/usr/bin/env python3
"""Quality of the denoiser's defaults, on the CPU alone (DESIGN.md section 5
"Post-pass"): the oracle renders box at 96x54 with 8 spp and with 2,048 spp (seed
42), the numpy reference filter (tests/post_ref.py) denoises the 8-spp frame with
the host's defaults, and the script prints MSE(noisy, truth) and MSE(denoised,
truth).  --sweep tries neighbouring settings."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import post_ref as R  # noqa: E402
from tinypathtracer_amd import DENOISE_DEFAULTS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=54)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--truth-spp", type=int, default=2048)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    ps = O.load_scene(a.scene)
    W, H = a.width, a.height
    noisy, _, _ = O.render(ps, W, H, a.spp, 8, 42, trig_mode=1)
    truth, _, _ = O.render(ps, W, H, a.truth_spp, 8, 42, trig_mode=1)
    aov = R.oracle_aov(ps, W, H)
    mse = lambda x: float(((np.asarray(x, np.float64) - truth) ** 2).mean())
    d = DENOISE_DEFAULTS
    sets = [(d["iterations"], d["sigma_color"], d["sigma_normal"], d["sigma_depth"], d["demodulate"])]
    if a.sweep:
        sets += [(it, sc, sn, sz, dm) for it in (3, 5) for sc in (0.3, 0.6, 1.2, 2.4) for sn in (0.1, 0.3)
                 for sz in (0.05,) for dm in (True, False)]
    base = mse(noisy)
    for it, sc, sn, sz, dm in sets:
        den = R.atrous_ref(noisy, aov["albedo"], aov["normal"], aov["depth"], it, sc, sn, sz, dm)
        m = mse(den)
        print(json.dumps({"iterations": it, "sigma_color": sc, "sigma_normal": sn, "sigma_depth": sz,
                          "demodulate": dm, "mse_noisy": base, "mse_denoised": m, "ratio": m / base}))


if __name__ == "__main__":
    main()
