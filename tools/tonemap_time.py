#!/usr/bin/env python3
"""What tone mapping costs (DESIGN.md section 5 "Tone mapping"): at 1920x1080, on a noise frame
(luminances log-uniform over 2^-10 .. 2^6) and on a constant frame (every lane of a wave in one
histogram bin), the times of tpt_tonemap's kernels by the library's own HIP events, as medians of
repeated calls after a warm-up on device buffers: fixed exposure to bytes, fixed exposure to bytes
and floats, and under auto-exposure the histogram, the measurement and the map kernel each.  In
the same run k_upsample (from 960x540, as tools/upsample_time.py times it) and k_temporal (row
segments, all outputs, as tools/temporal_time.py times it) on box.gltf, and every kernel's
bandwidth on its compulsory bytes: the map kernel reads 12 B per pixel and writes 3 B of a 4-B
pixel (12 B more with the float output), the histogram kernel reads 12 B.  The unchanged kernels'
bandwidth in this run is the yardstick.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402

MAP_BYTES, MAP_FLOAT_BYTES, HIST_BYTES = 12 + 4, 12 + 4 + 12, 12
UPSAMPLE_FULL, UPSAMPLE_LOW = 12 + 4 + 4 + 12 + 3, 12 + 12 + 4 + 4      # tools/upsample_time.py compulsory_bytes, plain
TEMPORAL_BYTES = 44 + 96 + 24                                           # tools/temporal_time.py, all outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--op", default=T.TONEMAP_DEFAULTS["op"])
    ap.add_argument("--transfer", default=T.TONEMAP_DEFAULTS["transfer"])
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("tonemap_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    npix = W * H
    s = T.Scene(a.scene)
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)

    def rate(nbytes, ms):
        m = statistics.median(ms)
        return {"ms": m, "ms_min": min(ms), "ms_max": max(ms), "compulsory_bytes": nbytes,
                "tb_per_s": nbytes / (m * 1e-3) / 1e12}

    def timed(call, keys):
        got = {k: [] for k in keys}
        for i in range(a.warmup + a.reps):
            st = call()
            if i >= a.warmup:
                for k in keys:
                    got[k].append(st[k])
        return got

    rng = np.random.default_rng(1)
    L = np.exp2(rng.uniform(-10.0, 6.0, (H, W, 1))).astype(np.float32)
    frames = {"noise": torch.from_numpy(L * rng.uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)).to(dev),
              "constant": torch.full((H, W, 3), 0.31, device=dev)}
    out = torch.zeros((H, W, 3), device=dev)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    res = {"width": W, "height": H, "reps": a.reps, "op": a.op, "transfer": a.transfer, "build": T.build_identity()}
    x = T.Exposure(d)
    kw = dict(op=a.op, transfer=a.transfer)
    for name, f in frames.items():
        def fixed(**extra):
            st = {}
            pt.tonemap(d, f, bgra=fb, stats=st, **kw, **extra)
            return st

        def auto():
            st = {}
            pt.tonemap(d, f, exposure=x, bgra=fb, stats=st, auto=True, **kw)
            st["measure_ms"] = x.measure_ms()
            return st

        entry = {"fixed_bytes": rate(npix * MAP_BYTES, timed(fixed, ["map_ms"])["map_ms"]),
                 "fixed_bytes_and_floats": rate(npix * MAP_FLOAT_BYTES, timed(lambda: fixed(out=out), ["map_ms"])["map_ms"])}
        t = timed(auto, ["hist_ms", "measure_ms", "map_ms"])
        entry["auto_histogram"] = rate(npix * HIST_BYTES, t["hist_ms"])
        entry["auto_measure"] = rate(0, t["measure_ms"])
        entry["auto_map"] = rate(npix * MAP_BYTES, t["map_ms"])
        res[name] = entry
    x.close()
    nm, cm = res["noise"]["auto_histogram"], res["constant"]["auto_histogram"]
    res["histogram_constant_over_noise"] = cm["ms"] / nm["ms"]
    res["histogram_noise_spread_ms"] = nm["ms_max"] - nm["ms_min"]

    # the unchanged kernels, in this run: k_upsample from half the size, k_temporal in row segments
    def planes(w, h):
        return {"albedo": torch.zeros((h, w, 3), device=dev), "normal": torch.zeros((h, w, 3), device=dev),
                "depth": torch.zeros((h, w), device=dev), "face": torch.zeros((h, w), dtype=torch.int32, device=dev),
                "material": torch.zeros((h, w), dtype=torch.int32, device=dev)}

    wl, hl = T.low_size(W, H, 2)
    low = T.PathTracer("", wl, hl, 0)
    aov, aov_low = planes(W, H), planes(wl, hl)
    pt.renderAOV(d, s.m_camera, out=aov)
    low.renderAOV(d, s.m_camera, out=aov_low)
    rad_low = torch.zeros((hl, wl, 3), device=dev)
    low.doTrace(d, s.m_camera, None, 4, seed=42, radiance=rad_low)

    def upsample():
        st = {}
        pt.upsample(d, rad_low, aov_low, aov, out=out, framebuffer=fb, stats=st)
        return st

    res["k_upsample"] = rate(npix * UPSAMPLE_FULL + wl * hl * UPSAMPLE_LOW, timed(upsample, ["kernel_ms"])["kernel_ms"])
    rad = torch.zeros((H, W, 3), device=dev)
    pt.doTrace(d, s.m_camera, None, 4, seed=42, radiance=rad)
    hist = T.History(d, W, H)
    var, n = torch.zeros((H, W), device=dev), torch.zeros((H, W), device=dev)
    acc = torch.zeros((H, W, 3), device=dev)

    def temporal():
        st = {}
        pt.temporal(hist, s.m_camera, rad, aov, out=acc, variance=var, history_len=n, framebuffer=fb, stats=st)
        return st

    res["k_temporal"] = rate(npix * TEMPORAL_BYTES, timed(temporal, ["kernel_ms"])["kernel_ms"])
    hist.close()
    for name in frames:
        for k, v in res[name].items():
            if v["compulsory_bytes"]:
                v["over_k_upsample"] = v["tb_per_s"] / res["k_upsample"]["tb_per_s"]
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
