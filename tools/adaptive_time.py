#!/usr/bin/env python3
"""What adaptive sampling buys on the device (DESIGN.md section 5 "Adaptive sampling"): box.gltf
at 1920x1080 as a uniform max_spp frame (and uniform frames at fewer spp, for what the same time
buys without the estimate) and as tpt_render_adaptive frames (min_spp 16, max_spp 1024) at a
sweep of targets.  Per frame: wall time, trace time, rays, the histogram of stop
levels, the tiles of every pass and the lane mode the planner's rule predicts for it (on 256 x
tiles pixels: four lanes per pixel up to tpt_stats.resident_lanes; predicted, not observed: the
library reports no lane mode per pass), the cost of the estimate kernel, and the mean squared error against a reference frame of another seed.
Every frame is rendered `reps` times (after one warm-up); times are medians.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--targets", type=float, nargs="+", default=[0.4, 0.2, 0.1, 0.05])
    ap.add_argument("--uniform-spp", type=int, nargs="*", default=[32, 64, 128, 256, 512],
                    help="uniform frames timed beside the max_spp one")
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("adaptive_time.py: no HIP device (a time measured elsewhere says nothing)")
    W, H = a.width, a.height
    s = T.Scene(a.scene)
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    tx, ty = (W + 15) // 16, (H + 15) // 16
    med = statistics.median
    rad = np.zeros((H, W, 3), np.float32)

    ref = np.zeros((H, W, 3), np.float32)
    pt.doTrace(d, s.m_camera, None, a.ref_spp, seed=4242, radiance=ref)
    mse = lambda x: float(np.mean((x.astype(np.float64) - ref) ** 2))

    def uniform(n):
        wall, trace = [], []
        for i in range(1 + a.reps):
            t0 = time.perf_counter()
            st = pt.doTrace(d, s.m_camera, None, n, seed=42, radiance=rad)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
                trace.append(st["trace_ms"])
        return {"spp": n, "wall_ms": med(wall), "trace_ms": med(trace), "rays": st["traversals"],
                "samples": st["samples"], "lanes_per_pixel": st["lanes_per_pixel"], "mse": mse(rad)}, st

    # uniform frames below max_spp too: what the same time buys without the estimate
    sweep = [uniform(n)[0] for n in a.uniform_spp if n < a.max_spp]
    top, st = uniform(a.max_spp)
    resident = st["resident_lanes"]
    res = {"width": W, "height": H, "scene": os.path.basename(a.scene), "reps": a.reps, "min_spp": a.min_spp,
           "max_spp": a.max_spp, "ref_spp": a.ref_spp, "tiles": tx * ty, "resident_lanes": resident,
           "uniform": top, "uniform_sweep": sweep, "adaptive": [], "build": T.build_identity()}
    spp = np.zeros((ty, tx), np.int32)
    for target in a.targets:
        wall, trace, err = [], [], []
        for i in range(1 + a.reps):
            t0 = time.perf_counter()
            st = pt.doTraceAdaptive(d, s.m_camera, None, min_spp=a.min_spp, max_spp=a.max_spp, target=target,
                                    seed=42, radiance=rad, tile_spp=spp)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
                trace.append(st["trace_ms"])
                err.append(st["error_ms"])
        levels, counts = np.unique(spp, return_counts=True)
        # The passes, from the stop levels: both halves of min_spp take every tile, the pass to n > min_spp
        # the tiles that end at n or beyond.  The library reports no lane mode per pass, so the mode here is
        # PREDICTED by the planner's automatic rule for this tool's case alone (lanes_per_pixel 0 on a scene
        # without delta lights, env IS or reference order whose stacks fit LDS, as box is; launch_plan.cpp,
        # pinned by tests/test_adaptive_plan_cpu.py): four lanes per pixel up to resident_lanes pixels.
        predicted = lambda tiles: 4 if 256 * tiles <= resident else 1
        passes = [{"to_spp": a.min_spp // 2, "tiles": tx * ty, "lanes_per_pixel_predicted": predicted(tx * ty)}]
        n = a.min_spp
        while n <= a.max_spp:
            tiles = int((spp >= n).sum())
            if tiles:
                passes.append({"to_spp": n, "tiles": tiles, "lanes_per_pixel_predicted": predicted(tiles)})
            n *= 2
        res["adaptive"].append({"target": target, "wall_ms": med(wall), "trace_ms": med(trace), "error_ms": med(err),
                                "rays": st["traversals"], "samples": st["samples"],
                                "sample_share": st["samples"] / res["uniform"]["samples"],
                                "passes": st["passes"], "unconverged_tiles": st["unconverged_tiles"],
                                "levels": {int(k): int(v) for k, v in zip(levels, counts)}, "pass_tiles": passes,
                                "mse": mse(rad)})
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
