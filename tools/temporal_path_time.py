#!/usr/bin/env python3
"""What accumulation through mirrors costs (DESIGN.md section 5 "Temporal accumulation through
mirrors"), at 1920x1080 with every buffer in device memory, kernel times by HIP events inside
the library, medians of repeated calls after a warm-up, the variants of a comparison
alternating call by call in one process:

  * tpt_temporal against tpt_temporal_path on box2's cap-0 buffers (no pixel follows a mirror:
    the path pass's only extra is the 4-byte bounce count per pixel), each on a history of its
    own, fed the frames of a trucking sequence there and back so that every call reprojects;
  * tpt_temporal_path on box2 and on hall (box2 with two facing mirror walls) at cap 8: the
    waves with mirror pixels gather and write the fourth plane too;
  * tpt_render_aov_path_points against tpt_render_aov_path on both scenes at cap 8.

Radiance is seeded noise: the pass's time does not depend on its values.  Prints one JSON
line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402
from tests import path_scenes as S  # noqa: E402
from tests import variant_scenes as V  # noqa: E402

MOVE = np.array([1.0, 0.4, 0.2]) * 0.03 * 6.69 / 7.0       # the tests' translation on box2, a seventh per frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("temporal_path_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    npix = W * H
    pt = T.PathTracer("", W, H, 0)
    med = statistics.median
    order = list(range(a.frames)) + list(range(a.frames - 2, 0, -1))   # 0 1 2 3 2 1 | 0 1 ...
    gen = torch.Generator(device=dev).manual_seed(1)
    rads = [torch.rand((H, W, 3), device=dev, generator=gen) * 2.0 for _ in range(a.frames)]
    out = torch.zeros((H, W, 3), device=dev)
    var, n = torch.zeros((H, W), device=dev), torch.zeros((H, W), device=dev)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    outputs = dict(out=out, variance=var, history_len=n, framebuffer=fb)

    def buffers():
        b = {"albedo": torch.zeros((H, W, 3), device=dev), "normal": torch.zeros((H, W, 3), device=dev),
             "depth": torch.zeros((H, W), device=dev), "material": torch.zeros((H, W), dtype=torch.int32, device=dev),
             "face": torch.zeros((H, W), dtype=torch.int32, device=dev),
             "bounces": torch.zeros((H, W), dtype=torch.int32, device=dev)}
        return b

    res = {"width": W, "height": H, "reps": a.reps, "build": T.build_identity()}
    for name in ("box2", "hall"):
        src = S.scene(name)
        d = V.device_scene(src).copySceneToDevice(0).build()
        base = V.device_scene(src).m_camera
        cams = [base.moved(*(k * MOVE)) for k in range(a.frames)]

        # the feature-buffer kernels, alternating, on the first camera
        plain, with_points = buffers(), dict(buffers(), points=torch.zeros((H, W, 3), device=dev))
        t_plain, t_points = [], []
        for i in range(a.warmup + a.reps):
            sa, sb = {}, {}
            pt.renderAOVPath(d, cams[0], 8, out=plain, stats=sa)
            pt.renderAOVPath(d, cams[0], 8, out=with_points, stats=sb)
            if i >= a.warmup:
                t_plain.append(sa["trace_ms"])
                t_points.append(sb["trace_ms"])
        res[f"{name}_aov_path_ms"] = med(t_plain)
        res[f"{name}_aov_path_points_ms"] = med(t_points)
        res[f"{name}_followed_fraction"] = sb["followed"] / npix

        def sequence(cap):
            seq = []
            for cam in cams:
                b = dict(buffers(), points=torch.zeros((H, W, 3), device=dev))
                pt.renderAOVPath(d, cam, cap, out=b)
                seq.append(b)
            return seq

        def alternate(variants, seq):
            """variants: name -> call(history, k, stats); returns name -> (median ms, reprojected fraction)"""
            hists = {v: T.History(d, W, H) for v in variants}
            times, found = {v: [] for v in variants}, {v: [] for v in variants}
            for i in range(a.warmup + a.reps):
                k = order[i % len(order)]
                for v, call in variants.items():
                    st = {}
                    call(hists[v], k, seq, st)
                    if i >= a.warmup:
                        times[v].append(st["kernel_ms"])
                        found[v].append(st["reprojected"] / npix)
            for h in hists.values():
                h.close()
            return {v: {"ms": med(times[v]), "ms_min": min(times[v]), "ms_max": max(times[v]),
                        "reprojected_fraction": med(found[v])} for v in variants}

        first_hit = lambda h, k, seq, st: pt.temporal(h, cams[k], rads[k], seq[k], stats=st, **outputs)
        path = lambda h, k, seq, st: pt.temporalPath(h, cams[k], rads[k], seq[k], stats=st, **outputs)
        if name == "box2":
            r = alternate({"temporal": first_hit, "temporal_path": path}, sequence(0))
            res["box2_cap0"] = r
            res["box2_cap0_path_over_temporal"] = r["temporal_path"]["ms"] / r["temporal"]["ms"]
        r = alternate({"temporal_on_path_guides": first_hit, "temporal_path": path}, sequence(8))
        res[f"{name}_cap8"] = r
        d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
