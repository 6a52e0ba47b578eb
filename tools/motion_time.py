#!/usr/bin/env python3
"""What following moving objects costs (DESIGN.md section 5 "Moving objects"): at 1920x1080
on box.gltf with device tensors, the kernel time (HIP events inside the library) of
tpt_temporal, of tpt_temporal_motion with nothing moved, and of tpt_temporal_motion with
ball1 moving, without and with motion_out -- medians of repeated calls after a warm-up, the
variants alternating in one process, tpt_temporal being the yardstick.  ball1 swings between
two poses --step apart, each with its own 8-spp frame and feature buffers rendered
beforehand, so the moving variants reproject it every call.  Also the wall time of
set_transforms + build per frame for box and box2 (TPT_BUILD_TIMING=1 adds the build's
phases on stderr).  Prints one JSON line."""
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

BALL1, CUBE = 5, 6                  # box's ball1, box2's Cube: the scenes' mesh nodes in node order


def moved(rest, obj, step):
    m = np.asarray(rest, np.float32).copy()
    m[obj, 12:15] += np.asarray(step, np.float32)
    return m


def rebuild_ms(name, obj, reps, warmup):
    """Median wall time of set_transforms + build (and of + build_async, which returns before
    the host trees are done) over a pose that changes every time."""
    s = T.Scene(os.path.join(ROOT, "tests", "golden", "scenes", name + ".gltf"))
    d = s.copySceneToDevice(0).build()
    out = {}
    for mode in ("build", "build_async"):
        ts = []
        for i in range(warmup + reps):
            vt = moved(s.vert_trans, obj, (0.01 * (i % 7), 0.0, 0.0))
            t0 = time.perf_counter()
            d.set_transforms(obj, vt[obj:obj + 1]).build(asynchronous=mode == "build_async")
            ts.append((time.perf_counter() - t0) * 1e3)
        d.build()                    # joins a pending asynchronous half
        out[mode] = statistics.median(ts[warmup:])
    d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--object", type=int, default=BALL1)
    ap.add_argument("--step", type=float, default=0.1, help="world units along x between the two poses")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("motion_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    s = T.Scene(a.scene)
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    cam = s.m_camera
    f3 = lambda: torch.zeros((H, W, 3), device=dev)
    f1 = lambda: torch.zeros((H, W), device=dev)
    i1 = lambda: torch.zeros((H, W), dtype=torch.int32, device=dev)
    poses = [np.asarray(s.vert_trans, np.float32).copy(), moved(s.vert_trans, a.object, (a.step, 0.0, 0.0))]
    frames = []
    for k, vt in enumerate(poses):                          # each pose's frame and feature buffers
        if k:
            d.set_transforms(a.object, vt[a.object:a.object + 1]).build()
        rad = f3()
        aov = {"albedo": f3(), "normal": f3(), "depth": f1(), "face": i1(), "material": i1()}
        pt.doTrace(d, cam, None, a.spp, seed=k + 1, radiance=rad)
        pt.renderAOV(d, cam, out=aov)
        frames.append((rad, aov))
    out, var, n, mv = f3(), f1(), f1(), torch.zeros((H, W, 2), device=dev)
    names = ("temporal", "motion_static", "motion_moving", "motion_moving_out")
    hist = {v: T.History(d, W, H) for v in names}
    times = {v: [] for v in names}
    found = {}
    one = lambda vt: vt[a.object:a.object + 1]
    for i in range(a.warmup + a.reps):
        # alternating: all see the same machine state.  The static variants run with the scene at
        # pose 0 before and now; the moving ones at the pose that swings.
        for v in names:
            k = 0 if v in ("temporal", "motion_static") else i % 2
            d.set_transforms(a.object, one(poses[k]))        # (the pass reads the matrices; no build is needed for it)
            rad, aov = frames[k]
            st = {}
            pt.temporal(hist[v], cam, rad, aov, out=out, variance=var, history_len=n, stats=st,
                        motion=v != "temporal", motion_out=mv if v == "motion_moving_out" else None)
            if i >= a.warmup:
                times[v].append(st["kernel_ms"])
                found[v] = st["reprojected"]
    for h in hist.values():
        h.close()
    lo, hi = int(s.lut[a.object][0]), int(s.lut[a.object + 1][0]) if a.object + 1 < len(s.lut) else s.n_faces
    face = frames[1][1]["face"]
    res = {"width": W, "height": H, "scene": os.path.basename(a.scene), "reps": a.reps, "pixels": W * H,
           "object": a.object, "object_pixels": int(((face >= lo) & (face < hi)).sum().item()),
           "reprojected": found, "build": T.build_identity()}
    base = statistics.median(times["temporal"])
    for v in names:
        med = statistics.median(times[v])
        res[v] = {"kernel_ms": med, "min": min(times[v]), "max": max(times[v]), "vs_temporal": med / base}
    d.close()
    res["rebuild_ms"] = {"box": rebuild_ms("box", BALL1, a.reps, a.warmup), "box2": rebuild_ms("box2", CUBE, a.reps, a.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
