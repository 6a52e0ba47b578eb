#!/usr/bin/env python3
"""What guided upsampling costs (DESIGN.md section 5 "Guided upsampling"): at 1920x1080 on
box.gltf, k_upsample's time (HIP events inside the library: tpt_upsample_stats.kernel_ms) from
960x540 and from 640x360, without and with demodulation, as medians of repeated calls after a
warm-up on device buffers, and the compulsory bytes over that time; then the whole chain of a
scaled frame -- the low-size render at --spp, the feature buffers of both sizes, the upsample -- as
the wall time of the calls, beside full-size renders at --spp / 4 and --spp in the same process.
The compulsory bytes are counted here: each full-size pixel's guides read once and its outputs
written once, each low-size pixel's planes read once (the taps that lanes share come from cache).
k_temporal's 0.065 ms and 5.2 TB/s at this size is the project's yardstick for a streaming
post-pass kernel.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402


def compulsory_bytes(npix, npix_low, demodulate, framebuffer):
    """Full size: normal 12 + depth 4 + material 4 read, radiance 12 written (+ 3 framebuffer
    bytes; alpha is untouched), albedo 12 more read with demodulation.  Low size: radiance 12 +
    normal 12 + depth 4 + material 4, albedo 12 more with demodulation."""
    full = 12 + 4 + 4 + 12 + (3 if framebuffer else 0) + (12 if demodulate else 0)
    low = 12 + 12 + 4 + 4 + (12 if demodulate else 0)
    return npix * full + npix_low * low


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("upsample_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    s = T.Scene(a.scene)
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    med = statistics.median

    def planes(w, h):
        return {"albedo": torch.zeros((h, w, 3), device=dev), "normal": torch.zeros((h, w, 3), device=dev),
                "depth": torch.zeros((h, w), device=dev), "face": torch.zeros((h, w), dtype=torch.int32, device=dev),
                "material": torch.zeros((h, w), dtype=torch.int32, device=dev)}

    aov = planes(W, H)
    out = torch.zeros((H, W, 3), device=dev)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    res = {"width": W, "height": H, "scene": os.path.basename(a.scene), "reps": a.reps, "spp": a.spp,
           "build": T.build_identity(), "scales": {}}

    def timed_render(tracer, spp, rad, fbuf):
        wall, trace = [], []
        for i in range(a.warmup + max(a.reps // 4, 3)):
            t0 = time.perf_counter()
            st = tracer.doTrace(d, s.m_camera, fbuf, spp, seed=42, radiance=rad)   # complete when it returns
            if i >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                trace.append(st["trace_ms"])
        return {"wall_ms": med(wall), "trace_ms": med(trace)}

    res["full_render"] = {str(spp): timed_render(pt, spp, out, fb) for spp in (max(a.spp // 4, 1), a.spp)}
    pt.renderAOV(d, s.m_camera, out=aov)
    for scale in (2, 3):
        wl, hl = T.low_size(W, H, scale)
        low = T.PathTracer("", wl, hl, 0)
        rad = torch.zeros((hl, wl, 3), device=dev)
        lfb = torch.zeros((hl, wl, 4), dtype=torch.uint8, device=dev)
        aov_low = planes(wl, hl)
        entry = {"low_width": wl, "low_height": hl, "low_render": timed_render(low, a.spp, rad, lfb)}
        low.renderAOV(d, s.m_camera, out=aov_low)
        for demod in (False, True):
            ms, fallback = [], 0
            for i in range(a.warmup + a.reps):
                st = {}
                pt.upsample(d, rad, aov_low, aov, demodulate=demod, out=out, framebuffer=fb, stats=st)
                if i >= a.warmup:
                    ms.append(st["kernel_ms"])
                fallback = st["fallback"]
            nbytes = compulsory_bytes(W * H, wl * hl, demod, True)
            entry["demodulate" if demod else "plain"] = {
                "kernel_ms": med(ms), "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "fallback": fallback,
                "compulsory_bytes": nbytes, "tb_per_s": nbytes / (med(ms) * 1e-3) / 1e12}
        chain = {"wall_ms": [], "render_ms": [], "aov_low_ms": [], "aov_ms": [], "upsample_ms": []}
        for i in range(a.warmup + max(a.reps // 4, 3)):
            sa, sb, su = {}, {}, {}
            t0 = time.perf_counter()
            st = low.doTrace(d, s.m_camera, lfb, a.spp, seed=42, radiance=rad)
            low.renderAOV(d, s.m_camera, out=aov_low, stats=sa)
            pt.renderAOV(d, s.m_camera, out=aov, stats=sb)
            pt.upsample(d, rad, aov_low, aov, out=out, framebuffer=fb, stats=su)
            if i >= a.warmup:
                chain["wall_ms"].append((time.perf_counter() - t0) * 1e3)
                chain["render_ms"].append(st["trace_ms"])
                chain["aov_low_ms"].append(sa["trace_ms"])
                chain["aov_ms"].append(sb["trace_ms"])
                chain["upsample_ms"].append(su["kernel_ms"])
        entry["chain"] = {k: med(v) for k, v in chain.items()}
        entry["chain_over_full_render"] = entry["chain"]["wall_ms"] / res["full_render"][str(a.spp)]["wall_ms"]
        res["scales"][str(scale)] = entry
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
