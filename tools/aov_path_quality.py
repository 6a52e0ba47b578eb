#!/usr/bin/env python3
"""What mirror-path guides buy the filters, on the CPU alone (DESIGN.md section 5
"Post-pass"): the oracle renders box at 96x54 with 8 spp and with 2,048 spp (seed 42);
the numpy a-trous filter (tests/post_ref.py, DENOISE_DEFAULTS) denoises the 8-spp frame
guided by the first-hit buffers (tests/post_ref.oracle_aov), by the mirror-path buffers
(tests/path_ref.oracle_aov_path) and by the variant that follows glass too, which DESIGN.md
records as a negative.  The MSE against the 2,048-spp frame is printed over the pixels whose
first hit is a mirror, over those whose first hit is glass, and over the whole frame.  Then
tools/svgf_quality.py's accumulated frames (eight frames of 8 spp, the camera yawing) through
the variance-guided filter (tests/svgf_ref.py, SVGF_DEFAULTS) with either set of guides for
the last frame; the temporal pass itself keeps first-hit guides."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import path_ref as P  # noqa: E402
from tests import post_ref as R  # noqa: E402
from tests import svgf_ref as SR  # noqa: E402
from tests import temporal_ref as TR  # noqa: E402
from tinypathtracer_amd import AOV_PATH_DEFAULTS, Camera, DENOISE_DEFAULTS, SVGF_DEFAULTS, TEMPORAL_DEFAULTS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=54)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--truth-spp", type=int, default=2048)
    ap.add_argument("--max-bounces", type=int, default=AOV_PATH_DEFAULTS["max_bounces"])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--yaw", type=float, default=1.0)
    ap.add_argument("--no-svgf", action="store_true")
    a = ap.parse_args()
    ps = O.load_scene(a.scene)
    W, H = a.width, a.height
    tr = P.Tracer(ps)
    d, sv = DENOISE_DEFAULTS, SVGF_DEFAULTS

    def guide_sets(cam):
        first = R.oracle_aov(ps, W, H, cam)
        return {"first hit": first,
                "mirror path": P.oracle_aov_path(ps, W, H, a.max_bounces, cam=cam, tracer=tr),
                "mirror and glass path": P.oracle_aov_path(ps, W, H, a.max_bounces, cam=cam, tracer=tr,
                                                           follow_glass=True)}

    def regions(first):
        fm = first["material"]
        mirror = (fm >= 0) & P.is_mirror(tr.mtl)[np.maximum(fm, 0)]
        glass = (fm >= 0) & (tr.mtl[np.maximum(fm, 0), 4] > 0)
        return {"mirror": mirror, "glass": glass, "frame": np.ones_like(mirror)}

    def report(label, x, truth, reg):
        e = (np.asarray(x, np.float64) - truth) ** 2
        row = {"image": label}
        for name, m in reg.items():
            row[f"mse_{name}"] = float(e[m].mean()) if m.any() else None
            row[f"pixels_{name}"] = int(m.sum())
        print(json.dumps(row), flush=True)
        return row

    noisy, _, _ = O.render(ps, W, H, a.spp, 8, 42, trig_mode=1)
    truth, _, _ = O.render(ps, W, H, a.truth_spp, 8, 42, trig_mode=1)
    sets = guide_sets(None)
    reg = regions(sets["first hit"])
    report("noisy", noisy, truth, reg)
    rows = {}
    for name, g in sets.items():
        den = R.atrous_ref(noisy, g["albedo"], g["normal"], g["depth"], d["iterations"], d["sigma_color"],
                           d["sigma_normal"], d["sigma_depth"], d["demodulate"])
        rows[name] = report(f"atrous, {name} guides", den, truth, reg)
    print(json.dumps({"mirror_ratio_path_over_first_hit": rows["mirror path"]["mse_mirror"] /
                      rows["first hit"]["mse_mirror"]}), flush=True)
    if a.no_svgf:
        return
    base = Camera(np.asarray(ps.src.camera_c2w, np.float32), float(ps.src.vfov), float(ps.src.aspect))
    state = None
    for k in range(a.frames):
        c = base.yawed(a.yaw * k)
        cam = {"c2w": c.c2w, "vfov": c.vfov, "aspect": c.aspect}
        frame, _, _ = O.render(ps, W, H, a.spp, 8, k + 1, trig_mode=1, cam=cam)
        t = TR.temporal_ref(state, cam, frame, R.oracle_aov(ps, W, H, cam), **TEMPORAL_DEFAULTS)
        state = t["state"]
    truth, _, _ = O.render(ps, W, H, a.truth_spp, 8, 42, trig_mode=1, cam=cam)
    sets = guide_sets(cam)
    reg = regions(sets["first hit"])
    var, hist = t["variance"].astype(np.float32), t["history_len"].astype(np.float32)
    report("accumulated", t["out"], truth, reg)
    for name in ("first hit", "mirror path"):
        g = sets[name]
        r = SR.svgf_ref(t["out"], g["albedo"], g["normal"], g["depth"], var, hist, **sv)
        report(f"svgf of the accumulated frame, {name} guides", r["out"], truth, reg)


if __name__ == "__main__":
    main()
