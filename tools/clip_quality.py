#!/usr/bin/env python3
"""What history clipping buys and costs when an object moves, on the CPU alone (DESIGN.md section 5
"History clipping").  The oracle renders box at 96x54 from its own camera: eight frames of 8 spp,
seeds 1..8, ball1 rising 0.055 per frame (test_gpu_motion's end-to-end sequence), and 2,048 spp
(seed 42) of the first and of the last pose.  The frames go through tpt_temporal_motion's
definition (tests/motion_ref.py) with the clip off and, through tests/clip_ref.py, at every
setting of a sweep of gamma, radius and cap.  Printed, one JSON line each: the MSE of the last
accumulated frame against the last pose's 2,048-spp frame over three regions --

  changed  the pixels whose first hit is the same face, not ball1's, in the first and the last
           pose, and whose converged luminance differs between the two by more than 10 %: the
           ball's shadow and its reflections, what the clip is for;
  ball     ball1's pixels in the last pose;
  rest     every other pixel: what the clip costs in noise

-- and the same frame through the variance-guided filter (tests/svgf_ref.py, SVGF_DEFAULTS) on the
pass's variance and history lengths: the clip shortens histories, so more pixels take the spatial
estimate.  The last line names the sweep's choice: the lowest `changed` MSE among the settings
whose `ball` and `rest` MSE, unfiltered and filtered, all stay within --budget (1.1) times the
unclipped ones: what the clip wins where shading changed may not be paid for elsewhere."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import motion_ref as MR  # noqa: E402
from tests import path_ref as P  # noqa: E402
from tests import svgf_ref as SR  # noqa: E402
from tests import temporal_path_ref as TP  # noqa: E402
from tests import temporal_ref as TR  # noqa: E402

BALL1 = 5
BALL_STEP = (0.0, 0.055, 0.0)
GAMMAS = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0)
RADII = (1, 2, 3)
CAPS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=54)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--truth-spp", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--budget", type=float, default=1.1)
    ap.add_argument("--no-svgf", action="store_true")
    a = ap.parse_args()
    W, H = a.width, a.height
    ps = O.load_scene(a.scene)
    carrier = MR.Carrier(T.Scene(a.scene))
    vt = ps.vt.reshape(-1, 16)                               # the oracle reads the scene's matrices in place
    rest = vt.copy()
    src = ps.src
    cam = {"c2w": np.asarray(src.camera_c2w, np.float32).reshape(16), "vfov": float(src.vfov), "aspect": float(src.aspect)}

    def pose(k):
        vt[BALL1] = MR.col_major(MR.translation(np.multiply(BALL_STEP, k)) @ MR.mat(rest[BALL1]))
        return vt.copy()

    frames, truths = [], {}
    for k in range(a.frames):
        m = pose(k)
        rad, _, _ = O.render(ps, W, H, a.spp, 8, k + 1, trig_mode=1, cam=cam)
        frames.append((m, rad, TP.oracle_aov_path_points(ps, W, H, 0, cam=cam, tracer=P.Tracer(ps))))
        if k in (0, a.frames - 1):
            truths[k], _, _ = O.render(ps, W, H, a.truth_spp, 8, 42, trig_mode=1, cam=cam)
    first, last = frames[0][2], frames[-1][2]
    truth = truths[a.frames - 1].astype(np.float64)
    lo, hi = carrier.faces_of(BALL1)
    ball = (last["face"] >= lo) & (last["face"] < hi)
    was_ball = (first["face"] >= lo) & (first["face"] < hi)
    l0, l1 = truths[0].astype(np.float64) @ TR.LUMA, truth @ TR.LUMA
    changed = (first["face"] == last["face"]) & ~ball & ~was_ball & (np.abs(l1 - l0) > 0.1 * np.maximum(np.maximum(l0, l1), 1e-6))
    regions = {"changed": changed, "ball": ball, "rest": ~changed & ~ball}
    print(json.dumps({"pixels": W * H, **{k: int(v.sum()) for k, v in regions.items()}}), flush=True)
    params = {k: T.TEMPORAL_DEFAULTS[k] for k in ("alpha", "depth_tol", "normal_min", "max_history", "demodulate")}

    def accumulate(clip):
        state = None
        for m, rad, aov in frames:
            r = MR.temporal_motion_ref(state, cam, rad, aov, carrier, m, clip=clip, **params)
            state = r["state"]
        return r

    def mse(x):
        e = ((np.asarray(x, np.float64) - truth) ** 2).mean(-1)
        return {k: float(e[v].mean()) for k, v in regions.items()}

    def report(label, r, extra=None):
        row = {"setting": label, "mse": mse(r["out"]), "mean_history": float(r["history_len"].mean()),
               "clipped_fraction": float(r["clipped"].mean())}
        if not a.no_svgf:
            g = frames[-1][2]
            f = SR.svgf_ref(r["out"], g["albedo"], g["normal"], g["depth"], r["variance"].astype(np.float32),
                            r["history_len"].astype(np.float32), **T.SVGF_DEFAULTS)
            row["mse_svgf"] = mse(f["out"])
        row.update(extra or {})
        print(json.dumps(row), flush=True)
        return row

    print(json.dumps({"setting": "last 8-spp frame", "mse": mse(frames[-1][1])}), flush=True)
    off = report("clip off", accumulate(None))
    rows = {}
    for gamma, radius, cap in itertools.product(GAMMAS, RADII, CAPS):
        clip = dict(radius=radius, gamma=gamma, max_history=cap)
        rows[gamma, radius, cap] = report(f"gamma {gamma} radius {radius} cap {cap}", accumulate(clip), {"clip": clip})
    kinds = ("mse",) if a.no_svgf else ("mse", "mse_svgf")
    ok = [k for k, r in rows.items()
          if all(r[kind][region] <= a.budget * off[kind][region] for kind in kinds for region in ("ball", "rest"))]
    wins = [k for k, r in rows.items() if r["mse"]["changed"] < off["mse"]["changed"]]
    best = min(ok, key=lambda k: rows[k]["mse"]["changed"]) if ok else None
    print(json.dumps({"settings": len(rows), "lower_changed_mse": len(wins), "within_budget": len(ok),
                      "choice": rows[best]["clip"] if best else None,
                      "choice_over_off": {k: rows[best]["mse"][k] / off["mse"][k] for k in regions} if best else None,
                      "choice_over_off_svgf": ({k: rows[best]["mse_svgf"][k] / off["mse_svgf"][k] for k in regions}
                                               if best and not a.no_svgf else None)}), flush=True)


if __name__ == "__main__":
    main()
