#!/usr/bin/env python3
"""Quality of guided upsampling at equal sample cost, on the CPU alone (DESIGN.md section 5
"Guided upsampling"): the oracle renders box at full size with n spp, at half size
(low_size(W, H, 2)) with 4 n and at third size with 9 n, tests/post_ref.py oracle_aov gives the
feature buffers of each size, tests/upsample_ref.py upsamples the low frames with the hosts'
defaults, and every frame is compared with a --truth-spp frame of another seed: raw, and through
the numpy a-trous reference at DENOISE_DEFAULTS, beside plain bilinear upsampling of the same low
frame.  --sweep tries the two sigmas and demodulation.  One JSON line per frame."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import post_ref as R  # noqa: E402
from tests import upsample_ref as U  # noqa: E402
from tinypathtracer_amd import DENOISE_DEFAULTS, UPSAMPLE_DEFAULTS, low_size  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--sizes", default="96x54,384x216")
    ap.add_argument("--spp", type=int, default=8, help="n: the full-size frame's samples per pixel")
    ap.add_argument("--truth-spp", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--truth-seed", type=int, default=4242)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    ps = O.load_scene(a.scene)
    dn = DENOISE_DEFAULTS
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        truth, _, _ = O.render(ps, W, H, a.truth_spp, 8, a.truth_seed, trig_mode=1)
        aov = R.oracle_aov(ps, W, H)
        mse = lambda x: float(((np.asarray(x, np.float64) - truth) ** 2).mean())
        filt = lambda x: R.atrous_ref(x, aov["albedo"], aov["normal"], aov["depth"], dn["iterations"], dn["sigma_color"],
                                      dn["sigma_normal"], dn["sigma_depth"], dn["demodulate"])

        def report(**kw):
            frame = kw.pop("frame")
            print(json.dumps(dict(kw, width=W, height=H, mse=mse(frame), mse_denoised=mse(filt(frame)))), flush=True)

        full, _, _ = O.render(ps, W, H, a.spp, 8, a.seed, trig_mode=1)
        report(frame=full, kind="full", spp=a.spp)
        for scale in (2, 3):
            wl, hl = low_size(W, H, scale)
            spp = a.spp * scale * scale
            low, _, _ = O.render(ps, wl, hl, spp, 8, a.seed, trig_mode=1)
            aov_low = R.oracle_aov(ps, wl, hl)
            base = dict(scale=scale, low_width=wl, low_height=hl, spp=spp)
            report(frame=U.bilinear_ref(low, W, H), kind="bilinear", **base)
            sets = [(UPSAMPLE_DEFAULTS["sigma_normal"], UPSAMPLE_DEFAULTS["sigma_depth"], UPSAMPLE_DEFAULTS["demodulate"])]
            if a.sweep:
                sets += [(sn, sz, dm) for dm in (False, True) for sn in (0.1, 0.3, 1.0) for sz in (0.02, 0.05, 0.2)
                         if (sn, sz, dm) != sets[0]]
            for sn, sz, dm in sets:
                up, fb = U.upsample_ref(low, aov_low, aov, sn, sz, dm)
                report(frame=up, kind="guided", sigma_normal=sn, sigma_depth=sz, demodulate=dm,
                       fallback=int(fb.sum()), **base)


if __name__ == "__main__":
    main()
