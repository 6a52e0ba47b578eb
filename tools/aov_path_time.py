#!/usr/bin/env python3
"""What the mirror-path feature buffers cost (DESIGN.md section 5 "Post-pass"): at
1920x1080, into device buffers, the kernel times (HIP events inside the library) of
tpt_render_aov on box, of tpt_render_aov_path on box at max_bounces 0 and 8, and of
tpt_render_aov_path at 8 on the hall (tests/path_scenes.py: box2 between two facing
mirrors), as medians of repeated calls after a warm-up, the variants alternating in
one process.  The yardstick is tpt_render_aov in the same process.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402
from tests import path_scenes as S  # noqa: E402
from tests import variant_scenes as V  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-bounces", type=int, default=T.AOV_PATH_DEFAULTS["max_bounces"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("aov_path_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    box = T.Scene(a.scene)
    d_box = box.copySceneToDevice(0).build()
    hall = V.device_scene(S.scene("hall"))
    d_hall = hall.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    out = {"albedo": torch.zeros((H, W, 3), device=dev), "normal": torch.zeros((H, W, 3), device=dev),
           "depth": torch.zeros((H, W), device=dev), "face": torch.zeros((H, W), dtype=torch.int32, device=dev),
           "material": torch.zeros((H, W), dtype=torch.int32, device=dev)}
    path_out = dict(out, bounces=torch.zeros((H, W), dtype=torch.int32, device=dev))

    def first_hit(st):
        pt.renderAOV(d_box, box.m_camera, out=out, stats=st)

    def path(scene, d, cap):
        return lambda st: pt.renderAOVPath(d, scene.m_camera, cap, out=path_out, stats=st)

    variants = {"aov_box": first_hit, "path_box_0": path(box, d_box, 0),
                f"path_box_{a.max_bounces}": path(box, d_box, a.max_bounces),
                f"path_hall_{a.max_bounces}": path(hall, d_hall, a.max_bounces)}
    times = {v: [] for v in variants}
    stats = {}
    for i in range(a.warmup + a.reps):
        for v, fn in variants.items():                     # alternating: all see the same machine state
            st = {}
            fn(st)
            if i >= a.warmup:
                times[v].append(st["trace_ms"])
            stats[v] = {k: st[k] for k in ("followed", "deepest") if k in st}
    base = statistics.median(times["aov_box"])
    res = {"width": W, "height": H, "reps": a.reps, "build": T.build_identity()}
    for v in variants:
        m = statistics.median(times[v])
        res[v] = dict(stats[v], ms=m, ms_min=min(times[v]), ms_max=max(times[v]), over_aov=m / base)
    d_box.close()
    d_hall.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
