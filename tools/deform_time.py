#!/usr/bin/env python3
"""What following deforming meshes costs (DESIGN.md section 5 "Deforming meshes"): at 1920x1080
on box.gltf with device tensors, the kernel time (HIP events inside the library) of tpt_temporal,
of tpt_temporal_motion and of tpt_temporal_deform with nothing deformed, alternating in one
process, and of tpt_temporal_deform beside tpt_temporal_motion while ball1 swings between two
poses of tpt_render --wave's displacement (each pose with its own 8-spp frame and feature buffers
rendered beforehand; the scene is rebuilt before every call, outside the timed kernel) -- medians
of repeated calls after a warm-up, tpt_temporal_motion being the yardstick.  The snapshot copy is
the difference of the calls' wall times less the difference of the kernels' (a call returns when
its stream has run), on box and, at a small frame, on C5, whose vertex count makes it visible.
Also the wall time of set_vertices + build / build_async for box's ball1 and for every vertex of
C5.  Prints one JSON line."""
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


def wave(scene, obj, amp, frame):
    """tpt_render --wave: (first vertex, positions) of the object's vertex range in `frame`."""
    lut = np.asarray(scene.lut, np.int64).reshape(-1, 2)
    end = int(lut[obj + 1, 0]) if obj + 1 < len(lut) else scene.n_faces
    ids = np.unique(np.asarray(scene.indices, np.int64)[3 * int(lut[obj, 0]):3 * end])
    lo, hi = int(ids.min()), int(ids.max())
    out = np.asarray(scene.vertices, np.float32)[lo:hi + 1].copy()
    s = (amp * np.sin(6.0 * out[ids - lo, 1].astype(np.float64) + float(frame))).astype(np.float32)
    out[ids - lo] += s[:, None] * np.asarray(scene.normals, np.float32)[ids]
    return lo, out


def median_ms(f, reps, warmup):
    ts = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        f(i)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[warmup:])


def rebuild_ms(s, d, first, poses, reps, warmup):
    """Median wall time of set_vertices + build (and + build_async, which returns before the
    host trees are done) over poses that change every time."""
    out = {}
    for mode in ("build", "build_async"):
        out[mode] = median_ms(lambda i: d.set_vertices(first, poses[i % len(poses)]).build(asynchronous=mode == "build_async"),
                              reps, warmup)
        d.build()                    # joins a pending asynchronous half
    return out


def buffers(torch, dev, W, H):
    f3 = lambda: torch.zeros((H, W, 3), device=dev)
    f1 = lambda: torch.zeros((H, W), device=dev)
    i1 = lambda: torch.zeros((H, W), dtype=torch.int32, device=dev)
    return f3, f1, i1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--amp", type=float, default=0.055, help="the wave's amplitude in world units")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("deform_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    s = T.Scene(os.path.join(SCENES, "box.gltf"))
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    cam = s.m_camera
    f3, f1, i1 = buffers(torch, dev, W, H)
    first, _ = wave(s, BALL1, a.amp, 0)
    poses = [wave(s, BALL1, a.amp, k)[1] for k in (0, 1)]
    frames = []
    for k in range(2):                                      # each pose's frame and feature buffers
        d.set_vertices(first, poses[k]).build()
        rad = f3()
        aov = {"albedo": f3(), "normal": f3(), "depth": f1(), "face": i1(), "material": i1()}
        pt.doTrace(d, cam, None, a.spp, seed=k + 1, radiance=rad)
        pt.renderAOV(d, cam, out=aov)
        frames.append((rad, aov))
    out, var, n, mv = f3(), f1(), f1(), torch.zeros((H, W, 2), device=dev)
    names = ("temporal", "motion_static", "deform_static", "motion_swing", "deform_swing", "deform_swing_out")
    hist = {v: T.History(d, W, H) for v in names}
    kernel = {v: [] for v in names}
    wall = {v: [] for v in names}
    found = {}

    def call(v, k, keep):
        rad, aov = frames[k]
        st = {}
        t0 = time.perf_counter()
        pt.temporal(hist[v], cam, rad, aov, out=out, variance=var, history_len=n, stats=st,
                    motion=v.startswith("motion"), deform=v.startswith("deform"),
                    motion_out=mv if v.endswith("_out") else None)
        dt = (time.perf_counter() - t0) * 1e3
        if keep:
            kernel[v].append(st["kernel_ms"])
            wall[v].append(dt)
            found[v] = st["reprojected"]

    d.set_vertices(first, poses[0]).build()
    for i in range(a.warmup + a.reps):                      # nothing deformed: the scene stays at pose 0
        for v in names[:3]:
            call(v, 0, i >= a.warmup)
    for i in range(a.warmup + a.reps):                      # ball1 swings; every variant sees the pose's frame
        d.set_vertices(first, poses[i % 2]).build()
        for v in names[3:]:
            call(v, i % 2, i >= a.warmup)
    for h in hist.values():
        h.close()
    lo, hi = int(s.lut[BALL1][0]), int(s.lut[BALL1 + 1][0])
    face = frames[1][1]["face"]
    res = {"width": W, "height": H, "scene": "box.gltf", "reps": a.reps, "pixels": W * H, "object": BALL1,
           "object_pixels": int(((face >= lo) & (face < hi)).sum().item()), "vertices": len(s.vertices),
           "reprojected": found, "build": T.build_identity()}
    med = {v: statistics.median(kernel[v]) for v in names}
    for v in names:
        base = med["motion_static" if v in names[:3] else "motion_swing"]
        res[v] = {"kernel_ms": med[v], "min": min(kernel[v]), "max": max(kernel[v]), "vs_motion": med[v] / base,
                  "call_ms": statistics.median(wall[v])}
    res["snapshot_ms_box"] = (res["deform_static"]["call_ms"] - res["motion_static"]["call_ms"]) - \
                             (med["deform_static"] - med["motion_static"])
    res["rebuild_ms"] = {"box_ball1": rebuild_ms(s, d, first, poses, a.reps, a.warmup)}
    d.close()

    # C5: the scene-side figures at its triangle count, the snapshot copy at a frame small enough not to hide it
    path = os.path.join(tempfile.gettempdir(), f"tpt_scenes_{os.getuid()}", "c5.gltf")
    synth.write_c5(path, SCENES)
    s5 = T.Scene(path)
    d5 = s5.copySceneToDevice(0).build()
    w5, h5 = 256, 144
    pt5 = T.PathTracer("", w5, h5, 0)
    g3, g1, j1 = buffers(torch, dev, w5, h5)
    rad5, out5 = g3(), g3()
    aov5 = {"albedo": g3(), "normal": g3(), "depth": g1(), "face": j1(), "material": j1()}
    pt5.renderAOV(d5, s5.m_camera, out=aov5)
    h5s = {v: T.History(d5, w5, h5) for v in ("motion", "deform")}
    c5 = {}
    for v in h5s:
        ks = []

        def one(i, v=v):
            st = {}
            pt5.temporal(h5s[v], s5.m_camera, rad5, aov5, out=out5, stats=st, motion=v == "motion", deform=v == "deform")
            ks.append(st["kernel_ms"])
        c5[v] = {"call_ms": median_ms(one, a.reps, a.warmup), "kernel_ms": statistics.median(ks[a.warmup:])}
    for h in h5s.values():
        h.close()
    nv = len(s5.vertices)
    res["c5"] = {"faces": s5.n_faces, "vertices": nv, "snapshot_bytes": 24 * nv, "frame": [w5, h5], **c5,
                 "snapshot_ms": (c5["deform"]["call_ms"] - c5["motion"]["call_ms"]) -
                                (c5["deform"]["kernel_ms"] - c5["motion"]["kernel_ms"])}
    v5 = np.asarray(s5.vertices, np.float32)
    all5 = [v5, v5 + np.float32(1e-3) * np.asarray(s5.normals, np.float32)]
    res["rebuild_ms"]["c5_all_vertices"] = rebuild_ms(s5, d5, 0, all5, max(3, a.reps // 4), 1)
    d5.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
