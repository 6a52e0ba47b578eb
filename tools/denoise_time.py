#!/usr/bin/env python3
"""What the post-pass costs (DESIGN.md section 5 "Post-pass"): at 1920x1080 on
box.gltf, tpt_render_aov's trace_ms and tpt_denoise's pack / filter / resolve times
(HIP events inside the library) as medians of repeated calls after a warm-up, for
the LDS-staged and the direct a-trous kernels in alternation, and the wall time of
a 64-spp tpt_render of the same frame in the same process as the yardstick.  The
filter is judged against the L2-gather ceiling: 25 taps x 32 B per pixel per
iteration over 18.8 TB/s.  Prints one JSON line."""
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
from tinypathtracer_amd import _lib  # noqa: E402

L2_GATHER_TBS = 18.8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("denoise_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    s = T.Scene(a.scene)
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    rad = torch.zeros((H, W, 3), device=dev)
    out = torch.zeros((H, W, 3), device=dev)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    aov = {"albedo": torch.zeros((H, W, 3), device=dev), "normal": torch.zeros((H, W, 3), device=dev),
           "depth": torch.zeros((H, W), device=dev), "face": torch.zeros((H, W), dtype=torch.int32, device=dev),
           "material": torch.zeros((H, W), dtype=torch.int32, device=dev)}
    med = statistics.median

    render_wall, render_trace = [], []
    for i in range(a.warmup + max(a.reps // 4, 3)):
        t0 = time.perf_counter()
        st = pt.doTrace(d, s.m_camera, fb, a.spp, seed=42, radiance=rad)   # complete when it returns
        if i >= a.warmup:
            render_wall.append((time.perf_counter() - t0) * 1e3)
            render_trace.append(st["trace_ms"])

    aov_ms, aov_wall = [], []
    for i in range(a.warmup + a.reps):
        st = {}
        t0 = time.perf_counter()
        pt.renderAOV(d, s.m_camera, out=aov, stats=st)
        if i >= a.warmup:
            aov_wall.append((time.perf_counter() - t0) * 1e3)
            aov_ms.append(st["trace_ms"])

    # per-variant, per-iteration-count filter times: the cost of iteration i is the increment
    variants = {"lds": 0, "direct": _lib.DENOISE_DIRECT}
    times = {v: {n: {"pack_ms": [], "filter_ms": [], "resolve_ms": [], "wall_ms": []}
                 for n in range(1, a.iterations + 1)} for v in variants}
    for i in range(a.warmup + a.reps):
        for n in range(1, a.iterations + 1):
            for v, fl in variants.items():             # alternating: both see the same machine state
                st = {}
                t0 = time.perf_counter()
                pt.denoise(d, rad, aov, iterations=n, out=out, framebuffer=fb, flags=fl, stats=st)
                if i >= a.warmup:
                    st["wall_ms"] = (time.perf_counter() - t0) * 1e3
                    for k in times[v][n]:
                        times[v][n][k].append(st[k])
    npix = W * H
    ceiling_ms = npix * 25 * 32 / (L2_GATHER_TBS * 1e12) * 1e3
    res = {"width": W, "height": H, "scene": os.path.basename(a.scene), "reps": a.reps,
           "render_spp": a.spp, "render_wall_ms": med(render_wall), "render_trace_ms": med(render_trace),
           "aov_trace_ms": med(aov_ms), "aov_wall_ms": med(aov_wall),
           "l2_gather_ceiling_ms_per_iteration": ceiling_ms, "build": T.build_identity()}
    for v in variants:
        full = times[v][a.iterations]
        filt = [med(times[v][n]["filter_ms"]) for n in range(1, a.iterations + 1)]
        per_it = [filt[0]] + [filt[k] - filt[k - 1] for k in range(1, len(filt))]
        res[v] = {"pack_ms": med(full["pack_ms"]), "filter_ms": med(full["filter_ms"]),
                  "resolve_ms": med(full["resolve_ms"]), "wall_ms": med(full["wall_ms"]),
                  "filter_ms_min": min(full["filter_ms"]), "filter_ms_max": max(full["filter_ms"]),
                  "filter_ms_by_iteration": per_it,
                  "ms_per_iteration": med(full["filter_ms"]) / a.iterations,
                  "ceiling_fraction": ceiling_ms / (med(full["filter_ms"]) / a.iterations)}
    best = min(variants, key=lambda v: res[v]["filter_ms"])
    post = res["aov_trace_ms"] + res[best]["pack_ms"] + res[best]["filter_ms"] + res[best]["resolve_ms"]
    res["post_pass_ms"] = post
    res["post_pass_over_render"] = post / res["render_wall_ms"]
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
