#!/usr/bin/env python3
"""What adaptive sampling costs in quality, on the CPU alone (DESIGN.md section 5 "Adaptive
sampling"): the oracle renders box at every level of the schedule (a pixel's first n samples
are the n-spp render, so the composition by tests/adaptive_ref.py is exactly the device's
frame), and per target the script prints the share of a uniform max_spp frame's samples, the
histogram of stop levels, the mean squared error against a reference frame of another seed,
raw and through tpt_denoise's numpy reference (tests/post_ref.py, the hosts' defaults), next
to the uniform frames of min_spp, max_spp and of about the adaptive frame's mean sample count.
Two things bias an adaptive frame: stopping on a noisy estimate biases the mean (a tile stops
when its two halves happen to agree), and neighbouring tiles at different levels can show
seams; `seam` is the mean squared error over the pixels on tile borders where the two tiles'
levels differ, against `inner`, the rest.  One JSON line per target."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import adaptive_ref as A  # noqa: E402
from tests import post_ref as R  # noqa: E402
from tinypathtracer_amd import DENOISE_DEFAULTS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--height", type=int, default=216)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=512)
    ap.add_argument("--targets", type=float, nargs="+", default=[0.4, 0.2, 0.1])
    ap.add_argument("--ref-spp", type=int, default=4096)
    a = ap.parse_args()
    ps = O.load_scene(a.scene)
    W, H = a.width, a.height
    levels = {n: O.render(ps, W, H, n, 8, 42, trig_mode=1)[0] for n in A.spp_levels(a.min_spp, a.max_spp)}
    ref = O.render(ps, W, H, a.ref_spp, 8, 4242, trig_mode=1)[0].astype(np.float64)
    aov = R.oracle_aov(ps, W, H)
    d = DENOISE_DEFAULTS
    den = lambda x: R.atrous_ref(x, aov["albedo"], aov["normal"], aov["depth"], d["iterations"], d["sigma_color"],
                                 d["sigma_normal"], d["sigma_depth"], d["demodulate"])
    se = lambda x: ((np.asarray(x, np.float64) - ref) ** 2).mean(-1)
    uniform = {n: {"mse": float(se(f).mean()), "mse_denoised": float(se(den(f)).mean())} for n, f in levels.items()
               if n >= a.min_spp}
    for target in a.targets:
        r = A.schedule(levels, target, a.min_spp, a.max_spp)
        spp = r["tile_spp"]
        frame = A.compose(spp, {int(n): levels[int(n)] for n in np.unique(spp)})
        per_pixel = np.repeat(np.repeat(spp, A.TILE, 0), A.TILE, 1)[:H, :W]
        border = np.zeros((H, W), bool)
        border[:, 1:] |= per_pixel[:, 1:] != per_pixel[:, :-1]
        border[:, :-1] |= per_pixel[:, 1:] != per_pixel[:, :-1]
        border[1:, :] |= per_pixel[1:, :] != per_pixel[:-1, :]
        border[:-1, :] |= per_pixel[1:, :] != per_pixel[:-1, :]
        e, ed = se(frame), se(den(frame))
        lv, cnt = np.unique(spp, return_counts=True)
        mean_spp = r["samples"] / (W * H)
        near = min(uniform, key=lambda n: abs(np.log2(n / mean_spp)))
        print(json.dumps({"target": target, "width": W, "height": H, "min_spp": a.min_spp, "max_spp": a.max_spp,
                          "ref_spp": a.ref_spp, "sample_share": r["samples"] / (W * H * a.max_spp),
                          "mean_spp": mean_spp, "levels": {int(k): int(v) for k, v in zip(lv, cnt)},
                          "unconverged": r["unconverged"], "mse": float(e.mean()), "mse_denoised": float(ed.mean()),
                          "seam": {"pixels": int(border.sum()), "mse": float(e[border].mean()) if border.any() else None,
                                   "mse_denoised": float(ed[border].mean()) if border.any() else None},
                          "inner": {"mse": float(e[~border].mean()), "mse_denoised": float(ed[~border].mean())},
                          "uniform_min": uniform[a.min_spp], "uniform_max": uniform[a.max_spp],
                          "uniform_near_mean": dict(uniform[near], spp=near)}))


if __name__ == "__main__":
    main()
