#!/usr/bin/env python3
"""What history clipping costs (DESIGN.md section 5 "History clipping"): at 1920x1080 on box.gltf
with device tensors, on tools/temporal_time.py's yaw sequence (the camera turns 1 degree per
frame, there and back, so every call reprojects), the box kernel's time for radius 1, 2 and 3
(tpt_clip_stats.box_ms: HIP events inside the library) and each clipped temporal kernel beside
its unclipped twin (tpt_temporal_stats.kernel_ms), the two alternating in one process on a history
each, fed the same frames -- medians of repeated calls after a warm-up.  tpt_temporal_motion and
tpt_temporal_deform run with nothing moved and nothing deformed (their test-and-skip paths);
tpt_temporal_path runs on the mirror-path buffers, its box comparing bounce counts too.  Prints
each kernel's compulsory traffic in bytes per pixel, the bandwidth that implies and its share of
the HBM peak.  The box kernel reads the frame's five input planes (44 B) and writes two float4
planes (32 B); a clipped temporal kernel reads those 32 B on top of its twin's traffic.  Prints one
JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402

HBM_PEAK_TBS = 8.0
BYTES_IN, BYTES_STATE, BYTES_OUT = 44, 48 + 48, 24          # tools/temporal_time.py's accounting
BYTES_PLANES = 32
EXTRA_IN = {"temporal": 0, "motion": 4, "deform": 4, "path": 4 + 12}   # face ids; bounce counts and points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--yaw", type=float, default=1.0)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("clip_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    npix = W * H
    s = T.Scene(a.scene)
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    med = statistics.median
    up = lambda g: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in g.items()}

    cams, rads, firsts, paths = [], [], [], []
    for k in range(a.frames):
        cam = s.m_camera.yawed(a.yaw * k)
        rad = torch.zeros((H, W, 3), device=dev)
        pt.doTrace(d, cam, None, a.spp, seed=k + 1, radiance=rad)
        cams.append(cam)
        rads.append(rad)
        firsts.append(up(pt.renderAOV(d, cam)))
        paths.append(up(pt.renderAOVPath(d, cam, T.AOV_PATH_DEFAULTS["max_bounces"], points=True)))
    order = list(range(a.frames)) + list(range(a.frames - 2, 0, -1))   # 0 1 2 3 2 1 | 0 1 ...

    out = torch.zeros((H, W, 3), device=dev)
    var = torch.zeros((H, W), device=dev)
    n = torch.zeros((H, W), device=dev)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    outputs = dict(out=out, variance=var, history_len=n, framebuffer=fb)

    def one(entry, hist, k, st):
        if entry == "path":
            pt.temporalPath(hist, cams[k], rads[k], paths[k], stats=st, **outputs)
        else:
            extra = {entry: True} if entry in ("motion", "deform") else {}
            pt.temporal(hist, cams[k], rads[k], firsts[k], stats=st, **outputs, **extra)

    def rate(bytes_per_pixel, ms):
        tbs = bytes_per_pixel * npix / (ms * 1e-3) / 1e12
        return {"ms": ms, "bytes_per_pixel": bytes_per_pixel, "tb_per_s": tbs, "hbm_peak_fraction": tbs / HBM_PEAK_TBS}

    res = {"width": W, "height": H, "scene": os.path.basename(a.scene), "reps": a.reps, "yaw_deg_per_frame": a.yaw,
           "build": T.build_identity(), "clip_defaults": T.CLIP_DEFAULTS}
    # every entry point: the clipped kernel beside its twin, alternating
    for entry in EXTRA_IN:
        hists = {False: T.History(d, W, H), True: T.History(d, W, H).set_clip()}
        times, box, clipped = {False: [], True: []}, [], []
        for i in range(a.warmup + a.reps):
            k = order[i % len(order)]
            for on in (False, True):
                st = {}
                one(entry, hists[on], k, st)
                if i >= a.warmup:
                    times[on].append(st["kernel_ms"])
                    if on:
                        cs = hists[on].clip_stats()
                        box.append(cs["box_ms"])
                        clipped.append(cs["clipped"] / npix)
        for h in hists.values():
            h.close()
        bpp = BYTES_IN + EXTRA_IN[entry] + BYTES_STATE + BYTES_OUT
        res[entry] = {"unclipped": dict(rate(bpp, med(times[False])), ms_min=min(times[False]), ms_max=max(times[False])),
                      "clipped": dict(rate(bpp + BYTES_PLANES, med(times[True])), ms_min=min(times[True]), ms_max=max(times[True])),
                      "clipped_over_unclipped": med(times[True]) / med(times[False]),
                      "box": dict(rate(BYTES_IN + (4 if entry == "path" else 0) + BYTES_PLANES, med(box)), ms_min=min(box), ms_max=max(box)),
                      "clipped_fraction": med(clipped)}
    # the box kernel per radius (tpt_temporal's inputs), the three alternating
    hists = {r: T.History(d, W, H).set_clip(radius=r) for r in (1, 2, 3)}
    box = {r: [] for r in hists}
    for i in range(a.warmup + a.reps):
        k = order[i % len(order)]
        for r, h in hists.items():
            one("temporal", h, k, {})
            if i >= a.warmup:
                box[r].append(h.clip_stats()["box_ms"])
    for h in hists.values():
        h.close()
    res["box_by_radius"] = {str(r): dict(rate(BYTES_IN + BYTES_PLANES, med(v)), ms_min=min(v), ms_max=max(v),
                                         lds_reads_per_pixel=(2 * r + 1) ** 2 * 2) for r, v in box.items()}
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
