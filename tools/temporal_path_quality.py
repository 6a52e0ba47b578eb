#!/usr/bin/env python3
"""What accumulation through mirrors buys under a trucking camera, on the CPU alone (DESIGN.md
section 5 "Temporal accumulation through mirrors").  The oracle renders box2 at 96x54: eight
frames of 8 spp, seeds 1..8, the camera moving per frame by a seventh of the tests' translation
(3 % of the median first-hit depth along x, 0.4 of that along y, 0.2 along z), and 2,048 spp
(seed 42) at the last camera.  The frames go through the numpy references of both passes:
tests/temporal_ref.py on first-hit guides (tpt_temporal) and tests/temporal_path_ref.py on
mirror-path guides (tpt_temporal_path), the latter at each point_tol of the sweep.  Printed, as
one JSON line each: the MSE of the last accumulated frame against the 2,048-spp frame over the
pixels whose first hit is a mirror and over the whole frame, the ratio path / first hit over
the mirror's pixels, the sweep's best point_tol, and the same frames through the
variance-guided filter (tests/svgf_ref.py, SVGF_DEFAULTS) with first-hit and with mirror-path
guides -- which re-examines the earlier negative, that path guides lose on an accumulated
frame."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import path_ref as P  # noqa: E402
from tests import svgf_ref as SR  # noqa: E402
from tests import temporal_path_ref as TP  # noqa: E402
from tests import temporal_ref as TR  # noqa: E402
from tinypathtracer_amd import AOV_PATH_DEFAULTS, Camera, SVGF_DEFAULTS, TEMPORAL_DEFAULTS  # noqa: E402

MOVE = np.array([1.0, 0.4, 0.2]) * 0.03
SWEEP = (0.5, 1.0, 2.0, 4.0, 8.0)


def frames_and_truth(ps, W, H, spp, truth_spp, frames, cap, tracer):
    """The cameras, each frame's render, first-hit and mirror-path buffers, and the truth at the
    last camera."""
    src = ps.src
    base = Camera(np.asarray(src.camera_c2w, np.float32), float(src.vfov), float(src.aspect))
    first0 = TP.oracle_aov_path_points(ps, W, H, 0, tracer=tracer)
    z_med = float(np.median(first0["depth"][first0["material"] >= 0]))
    step = MOVE * z_med / max(frames - 1, 1)
    out = []
    for k in range(frames):
        c = base.moved(*(k * step))
        cam = {"c2w": c.c2w, "vfov": c.vfov, "aspect": c.aspect}
        rad, _, _ = O.render(ps, W, H, spp, 8, k + 1, trig_mode=1, cam=cam)
        out.append((cam, rad, TP.oracle_aov_path_points(ps, W, H, 0, cam=cam, tracer=tracer),
                    TP.oracle_aov_path_points(ps, W, H, cap, cam=cam, tracer=tracer)))
    truth, _, _ = O.render(ps, W, H, truth_spp, 8, 42, trig_mode=1, cam=out[-1][0])
    return out, truth, z_med


def accumulate_first_hit(frames, params):
    state = None
    for cam, rad, first, _ in frames:
        r = TR.temporal_ref(state, cam, rad, first, **params)
        state = r["state"]
    return r


def accumulate_path(frames, params, point_tol):
    state = None
    for cam, rad, _, path in frames:
        r = TP.temporal_path_ref(state, cam, rad, path, point_tol=point_tol, **params)
        state = r["state"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box2.gltf"))
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=54)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--truth-spp", type=int, default=2048)
    ap.add_argument("--max-bounces", type=int, default=AOV_PATH_DEFAULTS["max_bounces"])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--no-svgf", action="store_true")
    a = ap.parse_args()
    ps = O.load_scene(a.scene)
    W, H = a.width, a.height
    tr = P.Tracer(ps)
    frames, truth, z_med = frames_and_truth(ps, W, H, a.spp, a.truth_spp, a.frames, a.max_bounces, tr)
    last_first, last_path = frames[-1][2], frames[-1][3]
    fm = last_first["material"]
    mirror = (fm >= 0) & P.is_mirror(tr.mtl)[np.maximum(fm, 0)]
    print(json.dumps({"median_first_hit_depth": z_med, "mirror_pixels": int(mirror.sum()), "pixels": W * H}), flush=True)

    def report(label, x, extra=None):
        e = (np.asarray(x, np.float64) - truth) ** 2
        row = {"image": label, "mse_mirror": float(e[mirror].mean()), "mse_frame": float(e.mean())}
        row.update(extra or {})
        print(json.dumps(row), flush=True)
        return row

    report("last 8-spp frame", frames[-1][1])
    t_first = accumulate_first_hit(frames, TEMPORAL_DEFAULTS)
    first = report("tpt_temporal, first-hit guides", t_first["out"],
                   {"mean_history_mirror": float(t_first["history_len"][mirror].mean())})
    sweep = {}
    for tol in SWEEP:
        t = accumulate_path(frames, TEMPORAL_DEFAULTS, tol)
        sweep[tol] = (report(f"tpt_temporal_path, point_tol {tol}", t["out"],
                             {"mean_history_mirror": float(t["history_len"][mirror].mean())}), t)
    best = min(SWEEP, key=lambda tol: sweep[tol][0]["mse_mirror"])
    print(json.dumps({"best_point_tol": best,
                      "mirror_ratio_path_over_first_hit": sweep[best][0]["mse_mirror"] / first["mse_mirror"],
                      "mirror_ratio_at": {str(tol): sweep[tol][0]["mse_mirror"] / first["mse_mirror"]
                                          for tol in SWEEP}}), flush=True)
    if a.no_svgf:
        return
    t_path = sweep[best][1]
    for label, t, g in (("svgf of tpt_temporal's frame, first-hit guides", t_first, last_first),
                        ("svgf of tpt_temporal's frame, mirror-path guides", t_first, last_path),
                        ("svgf of tpt_temporal_path's frame, mirror-path guides", t_path, last_path)):
        r = SR.svgf_ref(t["out"], g["albedo"], g["normal"], g["depth"], t["variance"].astype(np.float32),
                        t["history_len"].astype(np.float32), **SVGF_DEFAULTS)
        report(label, r["out"])


if __name__ == "__main__":
    main()
