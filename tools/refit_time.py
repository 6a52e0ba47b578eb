#!/usr/bin/env python3
"""What a BVH refit costs and what it does to the trees (DESIGN.md section 5 "BVH refit"), on one
MI355X, in one process with the variants alternating, medians of repeated calls after a warm-up:

  * set_vertices + refit against set_vertices + build and + build_async, the pose changing every
    time: host wall time of the two calls, and the refit's own device time (tpt_refit_stats.ms).
    box.gltf with ball1 under tpt_render --wave's displacement, and C5 (131,712 triangles) with
    every vertex displaced.  The yardstick is the rebuild in the same process.
  * the same displacement at amplitudes from one pixel of a 1920x1080 frame up to a large fraction
    of the object: the refitted main tree's cost against the built one (tpt_refit_stats.cost /
    cost_built, refitted from a build of the rest pose), and the trace rate of a 64-spp frame of
    the refitted scene against the same frame of the scene rebuilt from the same vertices.

Run it under a time limit of its own (timeout -k 10 600 python tools/refit_time.py).  Prints one
JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402
from tinypathtracer_amd import synth  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
BALL1 = 5                           # box's ball1: the scene's mesh nodes in node order


def object_ids(scene, obj):
    lut = np.asarray(scene.lut, np.int64).reshape(-1, 2)
    end = int(lut[obj + 1, 0]) if obj + 1 < len(lut) else scene.n_faces
    return np.unique(np.asarray(scene.indices, np.int64)[3 * int(lut[obj, 0]):3 * end])


def wave(scene, ids, amp, frame):
    """tpt_render --wave on the vertices `ids`: (first vertex, positions of the id range)."""
    lo, hi = int(ids.min()), int(ids.max())
    out = np.asarray(scene.vertices, np.float32)[lo:hi + 1].copy()
    s = (amp * np.sin(6.0 * out[ids - lo, 1].astype(np.float64) + float(frame))).astype(np.float32)
    out[ids - lo] += s[:, None] * np.asarray(scene.normals, np.float32)[ids]
    return lo, out


def timing(d, first, poses, reps, warmup):
    """Per variant the median host wall time of set_vertices + the call, the poses changing every
    time; every timed call starts from a complete build (an untimed one follows build_async, whose
    host half the next set_vertices would otherwise join, and supersede)."""
    wall = {"refit": [], "build": [], "build_async": []}
    dev_ms, launches, calls = [], 0, 0
    d.build()
    for i in range(warmup + reps):
        for v in wall:
            pose = poses[calls % len(poses)]
            calls += 1
            t0 = time.perf_counter()
            d.set_vertices(first, pose)
            if v == "refit":
                st = d.refit()
            else:
                d.build(asynchronous=v == "build_async")
            dt = (time.perf_counter() - t0) * 1e3
            if v == "refit":
                assert st["rebuilt"] == 0, "the refit fell back to a build"
                launches = st["launches"]
                if i >= warmup:
                    dev_ms.append(st["ms"])
            if v == "build_async":
                d.build()
            if i >= warmup:
                wall[v].append(dt)
    out = {v: {"wall_ms": statistics.median(ts), "min": min(ts), "max": max(ts)} for v, ts in wall.items()}
    out["refit"]["device_ms"] = statistics.median(dev_ms)
    out["refit"]["launches"] = launches
    out["refit"]["vs_build"] = out["refit"]["wall_ms"] / out["build"]["wall_ms"]
    return out


def mrays(pt, d, cam, rad, spp, seed):
    st = pt.doTrace(d, cam, None, spp, seed=seed, radiance=rad)
    return st["traversals"] / (st["trace_ms"] * 1e-3) / 1e6


def sweep(s, d, pt, cam, rad, ids, amps, spp, reps):
    """Per amplitude: cost / cost_built of the scene refitted from a build of the rest pose, and
    the trace rate of the same frame on the refitted and on the rebuilt scene (medians, alternating)."""
    first = int(ids.min())
    rest = np.asarray(s.vertices, np.float32)[first:int(ids.max()) + 1]
    rows = []
    for amp in amps:
        _, pose = wave(s, ids, amp, 1)
        rate = {"refit": [], "build": []}
        refused = None
        for i in range(1 + reps):
            d.set_vertices(first, rest).build()
            d.set_vertices(first, pose)
            st = d.refit()
            assert st["rebuilt"] == 0
            a = mrays(pt, d, cam, rad, spp, 7)
            try:
                # a pose that folds many vertices onto one point gives the LBVH duplicate Morton
                # keys, which a full build may refuse; the refit keeps the rest pose's topology
                d.set_vertices(first, pose).build()
            except T.TPTError as e:
                refused = str(e)
                break
            b = mrays(pt, d, cam, rad, spp, 7)
            if i:
                rate["refit"].append(a)
                rate["build"].append(b)
        row = {"amp": amp, "cost": st["cost"], "cost_built": st["cost_built"],
               "cost_ratio": st["cost"] / st["cost_built"], "refit_ms": st["ms"]}
        if refused is None:
            r, b = statistics.median(rate["refit"]), statistics.median(rate["build"])
            row.update({"mrays_refit": r, "mrays_rebuilt": b, "rate_ratio": r / b})
        else:
            row["rebuild_refused"] = refused[:80]
        rows.append(row)
    d.set_vertices(first, rest).build()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frame-reps", type=int, default=3, help="64-spp frames per amplitude and variant")
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("refit_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    res = {"width": W, "height": H, "spp": a.spp, "reps": a.reps, "build": T.build_identity()}

    def run(name, s, ids, amps, reps, frame_reps):
        d = s.copySceneToDevice(0).build()
        pt = T.PathTracer("", W, H, 0)
        rad = torch.zeros((H, W, 3), device=dev)
        first = int(ids.min())
        poses = [wave(s, ids, amps[1], k)[1] for k in range(8)]
        out = {"faces": s.n_faces, "vertices_set": int(ids.max()) - first + 1,
               "timing": timing(d, first, poses, reps, a.warmup),
               "sweep": sweep(s, d, pt, s.m_camera, rad, ids, amps, a.spp, frame_reps)}
        d.close()
        res[name] = out

    # box: ball1 waving.  One pixel at 1920x1080: ball1 sits 7 world units from the camera, where a
    # frame 1080 rows high over 2 tan(vfov / 2) has 380 pixels per world unit; its matrix has scale 1
    s = T.Scene(os.path.join(SCENES, "box.gltf"))
    ids = object_ids(s, BALL1)
    radius = 0.5 * float(np.ptp(np.asarray(s.vertices, np.float64)[ids], axis=0).max())
    px = 7.0 * 2.0 * np.tan(0.5 * float(s.m_camera.vfov)) / H
    res["box_ball1_radius"] = radius
    run("box_ball1", s, ids, [px, 0.055] + [f * radius for f in (0.25, 0.5, 0.75, 0.95)], a.reps, a.frame_reps)

    # C5: every vertex, the same displacement; amplitudes as fractions of its mean edge length
    path = os.path.join(tempfile.gettempdir(), f"tpt_scenes_{os.getuid()}", "c5.gltf")
    synth.write_c5(path, SCENES)
    s5 = T.Scene(path)
    v5 = np.asarray(s5.vertices, np.float64)
    tri = np.asarray(s5.indices, np.int64).reshape(-1, 3)
    edge = float(np.linalg.norm(v5[tri[:, 1]] - v5[tri[:, 0]], axis=-1).mean())
    res["c5_mean_edge"] = edge
    all_ids = np.arange(len(v5))
    run("c5_all_vertices", s5, all_ids, [f * edge for f in (0.1, 0.5, 1.0, 2.0, 5.0, 20.0)], max(5, a.reps // 4),
        max(2, a.frame_reps - 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
