#!/usr/bin/env python3
"""What the variance-guided filter costs (DESIGN.md section 5 "Post-pass"): at 1920x1080
on box.gltf with device tensors, tpt_denoise_svgf's pack / estimate / filter / resolve
times (HIP events inside the library) as medians of repeated calls after a warm-up,
for the LDS-staged and the direct kernels in alternation and for every iteration
count (the cost of iteration i is the increment), with tpt_denoise in the same
process as the yardstick.  The input is an 8-spp frame through tpt_temporal over
--frames yawing frames, so the steady state has that pass's share of short
histories; the estimate kernel is also timed on a first frame (no variance: every
pixel short) and with no short pixel at all.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402
from tinypathtracer_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "box.gltf"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--yaw", type=float, default=1.0)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if T.device_count() <= 0:
        sys.exit("svgf_time.py: no HIP device (a time measured elsewhere says nothing)")
    import torch
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    s = T.Scene(a.scene)
    d = s.copySceneToDevice(0).build()
    pt = T.PathTracer("", W, H, 0)
    f3 = lambda: torch.zeros((H, W, 3), device=dev)
    f1 = lambda: torch.zeros((H, W), device=dev)
    rad, acc, out, var, hist, vout = f3(), f3(), f3(), f1(), f1(), f1()
    aov = {"albedo": f3(), "normal": f3(), "depth": f1(), "face": torch.zeros((H, W), dtype=torch.int32, device=dev),
           "material": torch.zeros((H, W), dtype=torch.int32, device=dev)}
    history = T.History(d, W, H)
    for k in range(a.frames):
        cam = s.m_camera.yawed(a.yaw * k)
        pt.doTrace(d, cam, None, a.spp, seed=k + 1, radiance=rad)
        pt.renderAOV(d, cam, out=aov)
        pt.temporal(history, cam, rad, aov, out=acc, variance=var, history_len=hist)
    history.close()
    long_ = torch.full((H, W), 64.0, device=dev)
    med = statistics.median
    keys = ("pack_ms", "estimate_ms", "filter_ms", "resolve_ms")
    variants = {"lds": 0, "direct": _lib.SVGF_DIRECT}
    counts = range(1, a.iterations + 1)
    times = {v: {n: {k: [] for k in keys} for n in counts} for v in variants}
    plain = {v: {n: [] for n in counts} for v in variants}
    plain_all = {v: {k: [] for k in ("pack_ms", "filter_ms", "resolve_ms")} for v in variants}
    first, none_short, estimated = [], [], {}
    for i in range(a.warmup + a.reps):
        keep = i >= a.warmup
        for n in counts:
            for v, fl in variants.items():             # alternating: all see the same machine state
                st, sp = {}, {}
                pt.denoiseSVGF(d, acc, aov, var, hist, iterations=n, out=out, variance_out=vout, flags=fl, stats=st)
                pt.denoise(d, acc, aov, iterations=n, out=out, flags=fl, stats=sp)   # DENOISE_DIRECT == SVGF_DIRECT
                if keep:
                    for k in keys:
                        times[v][n][k].append(st[k])
                    plain[v][n].append(sp["filter_ms"])
                    if n == a.iterations:
                        for k in plain_all[v]:
                            plain_all[v][k].append(sp[k])
                    estimated["steady"] = st["estimated"]
        st = {}
        pt.denoiseSVGF(d, rad, aov, iterations=1, out=out, stats=st)               # a first frame: every pixel short
        if keep:
            first.append(st["estimate_ms"])
            estimated["first_frame"] = st["estimated"]
        st = {}
        pt.denoiseSVGF(d, acc, aov, var, long_, iterations=1, out=out, stats=st)   # every block takes the early exit
        if keep:
            none_short.append(st["estimate_ms"])
            estimated["none_short"] = st["estimated"]

    def by_iteration(series):
        filt = [med(series[n]) for n in counts]
        return [filt[0]] + [filt[k] - filt[k - 1] for k in range(1, len(filt))]

    res = {"width": W, "height": H, "scene": os.path.basename(a.scene), "reps": a.reps, "frames": a.frames,
           "pixels": W * H, "estimated": estimated, "estimate_ms_first_frame": med(first),
           "estimate_ms_none_short": med(none_short), "build": T.build_identity()}
    for v in variants:
        full = times[v][a.iterations]
        res[v] = {k: med(full[k]) for k in keys}
        res[v]["total_ms"] = sum(res[v][k] for k in keys)
        res[v]["filter_ms_min"], res[v]["filter_ms_max"] = min(full["filter_ms"]), max(full["filter_ms"])
        res[v]["filter_ms_by_iteration"] = by_iteration({n: times[v][n]["filter_ms"] for n in counts})
        res["tpt_denoise_" + v] = {k: med(x) for k, x in plain_all[v].items()}
        res["tpt_denoise_" + v]["filter_ms_by_iteration"] = by_iteration(plain[v])
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
