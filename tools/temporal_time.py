#!/usr/bin/env python3
"""What the temporal pass costs (DESIGN.md section 5 "Post-pass"): at 1920x1080 on
box.gltf, tpt_temporal's kernel time (HIP events inside the library) on the frames of
a yaw sequence -- the camera turns 1 degree per frame, there and back, so every call
reprojects -- as the median of repeated calls after a warm-up, for the row-segment
and the 16x16-tile launches in alternation (a history each, fed the same frames).
Prints the pass's compulsory traffic in bytes per pixel (this frame's planes in, the
previous state in once, the new state and the outputs out), the bandwidth that
implies and its share of the HBM peak; beside it tpt_denoise's pack and resolve
kernels, pure streaming kernels over the same frame in the same process, by the same
arithmetic, and the wall time of a 64-spp tpt_render as the yardstick.  Prints one
JSON line."""
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

HBM_PEAK_TBS = 8.0
# bytes per pixel: radiance 12 + albedo 12 + normal 12 + depth 4 + material 4 in; three float4
# planes of the previous state in (each pixel once: overlapping taps are cache hits) and of
# the new state out; radiance 12 + variance 4 + history length 4 + framebuffer 4 out
BYTES_IN, BYTES_STATE, BYTES_OUT = 44, 48 + 48, 24
PACK_BYTES = 12 + 12 + 12 + 4 + 32          # k_dn_pack: radiance, albedo, normal, depth in; two float4 planes out
RESOLVE_BYTES = 16 + 12 + 12 + 4            # k_dn_resolve: colour plane, albedo in; radiance, framebuffer out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--yaw", type=float, default=1.0)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("temporal_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    npix = W * H
    s = T.Scene(a.scene)
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    med = statistics.median

    # the sequence's frames, rendered once: radiance and feature buffers in device memory
    cams, rads, aovs, render_wall = [], [], [], []
    for k in range(a.frames):
        cam = s.m_camera.yawed(a.yaw * k)
        rad = torch.zeros((H, W, 3), device=dev)
        aov = {"albedo": torch.zeros((H, W, 3), device=dev), "normal": torch.zeros((H, W, 3), device=dev),
               "depth": torch.zeros((H, W), device=dev), "material": torch.zeros((H, W), dtype=torch.int32, device=dev)}
        for _ in range(2):                                 # the second render of a frame is the timed one
            t0 = time.perf_counter()
            pt.doTrace(d, cam, None, a.spp, seed=k + 1, radiance=rad)
            wall = (time.perf_counter() - t0) * 1e3
        render_wall.append(wall)
        pt.renderAOV(d, cam, out=aov)
        cams.append(cam)
        rads.append(rad)
        aovs.append(aov)
    order = list(range(a.frames)) + list(range(a.frames - 2, 0, -1))   # 0 1 2 3 2 1 | 0 1 ...

    out = torch.zeros((H, W, 3), device=dev)
    var = torch.zeros((H, W), device=dev)
    n = torch.zeros((H, W), device=dev)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    variants = {"rows": 0, "tiles": _lib.TEMPORAL_TILES}
    outputs = {"all_outputs": dict(variance=var, history_len=n, framebuffer=fb), "radiance_only": {}}
    hists = {(v, o): T.History(d, W, H) for v in variants for o in outputs}
    times = {key: [] for key in hists}
    found = {key: [] for key in hists}
    for i in range(a.warmup + a.reps):
        k = order[i % len(order)]
        for o, extra in outputs.items():
            for v, fl in variants.items():                 # alternating: both see the same machine state
                st = {}
                pt.temporal(hists[v, o], cams[k], rads[k], aovs[k], out=out, flags=fl, stats=st, **extra)
                if i >= a.warmup:
                    times[v, o].append(st["kernel_ms"])
                    found[v, o].append(st["reprojected"] / npix)
    for h in hists.values():
        h.close()

    # two streaming kernels over the same frame, same process: tpt_denoise's pack and resolve
    pack, resolve = [], []
    for i in range(a.warmup + a.reps):
        st = {}
        pt.denoise(d, rads[0], aovs[0], iterations=1, out=out, framebuffer=fb, stats=st)
        if i >= a.warmup:
            pack.append(st["pack_ms"])
            resolve.append(st["resolve_ms"])

    def rate(bytes_per_pixel, ms):
        tbs = bytes_per_pixel * npix / (ms * 1e-3) / 1e12
        return {"ms": ms, "bytes_per_pixel": bytes_per_pixel, "tb_per_s": tbs, "hbm_peak_fraction": tbs / HBM_PEAK_TBS}

    res = {"width": W, "height": H, "scene": os.path.basename(a.scene), "reps": a.reps, "yaw_deg_per_frame": a.yaw,
           "render_spp": a.spp, "render_wall_ms": med(render_wall), "build": T.build_identity(),
           "k_dn_pack": rate(PACK_BYTES, med(pack)), "k_dn_resolve": rate(RESOLVE_BYTES, med(resolve))}
    for (v, o), ms in times.items():
        bpp = BYTES_IN + BYTES_STATE + (BYTES_OUT if o == "all_outputs" else 12)
        res[f"{v}_{o}"] = dict(rate(bpp, med(ms)), ms_min=min(ms), ms_max=max(ms),
                               reprojected_fraction=med(found[v, o]))
    best = min(variants, key=lambda v: res[f"{v}_all_outputs"]["ms"])
    res["best"] = best
    res["temporal_over_render"] = res[f"{best}_all_outputs"]["ms"] / res["render_wall_ms"]
    res["temporal_rate_over_pack_rate"] = res[f"{best}_all_outputs"]["tb_per_s"] / res["k_dn_pack"]["tb_per_s"]
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
