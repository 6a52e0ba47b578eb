"""The child process of tests/test_gpu_threads.py: one phase of concurrent calls on different
scenes (include/tpt.h: "calls on different scenes may run concurrently from different host
threads"), and the same calls made serially on twin handles, all written to one .npz.  The
parent asserts; this file only records.

    python tests/threads_child.py --phase first|steady|env|churn --out FILE.npz

The library is loaded on the main thread; the workers start behind one barrier (ctypes
releases the GIL in every call), catch their exceptions and keep the name of the call they
are in.  The main thread joins each with a limit of JOIN_SECONDS; a worker still alive after
that ends the process with status 3 and the name of its call, and nothing more is started.
A worker that raised ends the phase too: the .npz is written with what there is and the serial
twins are not run (the parent fails on `errors`).

Keys of the .npz: <run>__<thread>_<scene>__<step>__<field>, run = conc | serial; `errors`
holds one line per worker that raised.  A thread's frame is (40 + 8 i) x (24 + 4 i) pixels at
4 spp, seed 42 + i, depth 8 (16 for tir): no two threads share a buffer size, and every scene
builds its trees with two threads."""
import argparse
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tinypathtracer_amd as T  # noqa: E402
from tinypathtracer_amd import _lib  # noqa: E402

SCENE_DIR = os.path.join(ROOT, "tests", "golden", "scenes")
JOIN_SECONDS = 120
SPP = 4
FIRST_SCENES = ["tir", "box1", "square", "box2", "light", "ball", "box", "tir"]   # the second tir: its own handle
STEADY_SCENES = ["box", "ball", "tir", "box2"]
RNG_FIRSTS = (0, 65535)
RNG_COUNT = 256
# square and ball hold delta lights: four lanes per pixel are refused there (launch_plan.cpp), so the
# scripts ask for pair mode (two lanes) on them and for four lanes on the others
LIT = ("square", "ball")


def frame_size(i):
    return 40 + 8 * i, 24 + 4 * i


def depth_of(name):
    return 16 if name == "tir" else 8


def sky_of(name, width=64, height=32):
    """ball renders against a sky; the other scenes against none."""
    return T.EnvLight(T.procedural_sky(width, height)) if name == "ball" else None


class Rec:
    """One thread's (or the serial twin's) record: the call it is in, its outputs."""

    def __init__(self, out, run, who):
        self.out, self.prefix, self.who, self.call = out, f"{run}__{who}", who, "start"

    def step(self, name, fn):
        self.call = name
        return fn()

    def put(self, step, field, value):
        self.out[f"{self.prefix}__{step}__{field}"] = np.array(value)

    def stats(self, step, d):
        for k, v in d.items():
            self.put(step, k, np.float64(v) if isinstance(v, float) else np.int64(v))


class WorkersFailed(Exception):
    """A worker raised: nothing more is started on the device."""


class Worker(threading.Thread):
    def __init__(self, barrier, rec, fn):
        super().__init__(daemon=True)
        self.barrier, self.rec, self.fn, self.error = barrier, rec, fn, None

    def run(self):
        try:
            self.barrier.wait()
            self.fn(self.rec)
            self.rec.call = "done"
        except BaseException as e:   # recorded: the parent names thread, scene and call
            self.error = f"{self.rec.who} in {self.rec.call}: {type(e).__name__}: {e}\n{traceback.format_exc()}"


def run_workers(out, jobs):
    """jobs: (who, fn(rec)); all start together.  Returns once every worker has ended well."""
    barrier = threading.Barrier(len(jobs))
    workers = [Worker(barrier, Rec(out, "conc", who), fn) for who, fn in jobs]
    for w in workers:
        w.start()
    for w in workers:
        w.join(JOIN_SECONDS)
        if w.is_alive():
            print(f"HUNG: {w.rec.who} in {w.rec.call}; the others: " +
                  ", ".join(f"{x.rec.who} in {x.rec.call}" for x in workers if x is not w), flush=True)
            os._exit(3)
    out["errors"] = np.array([w.error for w in workers if w.error] or [], dtype=str)
    if len(out["errors"]):
        raise WorkersFailed()


def device_scene(name):
    s = T.Scene(os.path.join(SCENE_DIR, f"{name}.gltf"))
    return s, s.copySceneToDevice(0).set_build_threads(2)


def render(rec, step, pt, d, cam, seed, depth, spp=SPP, **kw):
    """One doTrace into fresh buffers: radiance, framebuffer and the statistics recorded."""
    W, H = pt.m_width, pt.m_height
    rad, fb = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 4), np.uint8)
    st = rec.step(step, lambda: pt.doTrace(d, cam, fb, spp, seed=seed, max_depth=depth, radiance=rad, **kw))
    rec.put(step, "radiance", rad)
    rec.put(step, "bgra", fb)
    rec.stats(step, st)
    return rad


def rng_states(rec, i):
    for first in RNG_FIRSTS:
        st = np.zeros((RNG_COUNT, 6), np.uint32)
        rec.step(f"rng{first}", lambda: _lib.check(T.lib().tpt_debug_rng_init(0, 42 + i, first, RNG_COUNT, st.ctypes.data)))
        rec.put("rng", f"first{first}", st)


# ---- first: the first library use of the process, from eight threads ----

def first_frame(rec, i, name):
    W, H = frame_size(i)
    s, d = rec.step("create", lambda: device_scene(name))
    rec.step("build", d.build)
    pt = T.PathTracer("", W, H, 0)
    pt.envLight = rec.step("env_create", lambda: sky_of(name))
    render(rec, "frame", pt, d, s.m_camera, 42 + i, depth_of(name))
    rec.step("close", d.close)
    if pt.envLight is not None:
        rec.step("env_close", pt.envLight.close)


def phase_first(out):
    def job(i, name):
        def fn(rec):
            if i % 2 == 0:
                first_frame(rec, i, name)
                rng_states(rec, i)
            else:
                rng_states(rec, i)
                first_frame(rec, i, name)
        return f"t{i}_{name}", fn
    jobs = [job(i, name) for i, name in enumerate(FIRST_SCENES)]
    run_workers(out, jobs)
    for i, name in enumerate(FIRST_SCENES):        # fresh handles, one after the other
        first_frame(Rec(out, "serial", f"t{i}_{name}"), i, name)


# ---- steady: every entry-point family on handles made beforehand ----

class Handles:
    def __init__(self, i, name):
        self.i, self.name = i, name
        self.W, self.H = frame_size(i)
        self.s, self.d = device_scene(name)
        self.d.build()
        self.env = sky_of(name)
        self.pt = T.PathTracer("", self.W, self.H, 0)
        self.wl, self.hl = T.low_size(self.W, self.H, 2)
        self.low = T.PathTracer("", self.wl, self.hl, 0)
        self.pt.envLight = self.low.envLight = self.env
        self.hist = T.History(self.d, self.W, self.H)

    def close(self):
        self.hist.close()
        self.d.close()
        if self.env is not None:
            self.env.close()


def steady_script(rec, h, rounds=2):
    s, d, pt, W, H = h.s, h.d, h.pt, h.W, h.H
    cam, cam2 = s.m_camera, s.m_camera.yawed(2.0)
    seed, depth = 42 + h.i, depth_of(h.name)
    for r in range(rounds):
        n = lambda step: f"r{r}_{step}"
        rad = render(rec, n("trace"), pt, d, cam, seed, depth)
        render(rec, n("one_lane"), pt, d, cam, seed, depth, lanes_per_pixel=1)
        if h.name in LIT:
            render(rec, n("pair"), pt, d, cam, seed, depth, lanes_per_pixel=2)
        else:
            render(rec, n("four_lanes"), pt, d, cam, seed, depth, lanes_per_pixel=4)
        render(rec, n("ref_order"), pt, d, cam, seed, depth, flags=_lib.FLAG_REF_ORDER)
        render(rec, n("wavefront"), pt, d, cam, seed, depth, flags=_lib.FLAG_WAVEFRONT)
        render(rec, n("accumulate_a"), pt, d, cam, seed, depth, spp=2)
        render(rec, n("accumulate_b"), pt, d, cam, None, depth, spp=2, accumulate=True)
        # two frames in one launch
        rads = [np.zeros((H, W, 3), np.float32) for _ in range(2)]
        fbs = [np.zeros((H, W, 4), np.uint8) for _ in range(2)]
        st = rec.step(n("frames"), lambda: pt.doTraceFrames(d, cam, [seed, seed + 100], fbs, SPP, max_depth=depth,
                                                            radiances=rads))
        rec.put(n("frames"), "radiance", np.stack(rads))
        rec.put(n("frames"), "bgra", np.stack(fbs))
        rec.stats(n("frames"), st)
        # feature buffers
        aov = rec.step(n("aov"), lambda: pt.renderAOV(d, cam))
        for k, v in aov.items():
            rec.put(n("aov"), k, v)
        if h.name == "tir":
            st = {}
            path = rec.step(n("aov_path"), lambda: pt.renderAOVPath(d, cam, points=True, stats=st))
            for k, v in path.items():
                rec.put(n("aov_path"), k, v)
            rec.stats(n("aov_path"), st)
        # the a-trous filter
        st, fb = {}, np.zeros((H, W, 4), np.uint8)
        den = rec.step(n("denoise"), lambda: pt.denoise(d, rad, aov, iterations=3, framebuffer=fb, stats=st))
        rec.put(n("denoise"), "radiance", den)
        rec.put(n("denoise"), "bgra", fb)
        rec.stats(n("denoise"), st)
        # two frames of temporal accumulation on the thread's own history, the second one clipped
        rec.step(n("history_reset"), lambda: h.hist.set_clip(None).reset())
        var = nlen = acc = aov_t = None
        for f, c in enumerate((cam, cam2)):
            step = n(f"temporal{f}")
            if f == 1:
                rec.step(n("set_clip"), h.hist.set_clip)
            rad_f = render(rec, step + "_render", pt, d, c, seed + f, depth)
            aov_t = rec.step(step + "_aov", lambda: pt.renderAOV(d, c))
            var, nlen, st = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), {}
            acc = rec.step(step, lambda: pt.temporal(h.hist, c, rad_f, aov_t, variance=var, history_len=nlen, stats=st))
            rec.put(step, "radiance", acc)
            rec.put(step, "variance", var)
            rec.put(step, "history_len", nlen)
            rec.stats(step, st)
            rec.stats(step + "_clip", rec.step(step + "_clip_stats", h.hist.clip_stats))
        st, vout = {}, np.zeros((H, W), np.float32)
        sv = rec.step(n("svgf"), lambda: pt.denoiseSVGF(d, acc, aov_t, var, nlen, variance_out=vout, stats=st))
        rec.put(n("svgf"), "radiance", sv)
        rec.put(n("svgf"), "variance", vout)
        rec.stats(n("svgf"), st)
        # guided upsampling from the half-size render
        rad_low = render(rec, n("low_render"), h.low, d, cam, seed, depth)
        aov_low = rec.step(n("low_aov"), lambda: h.low.renderAOV(d, cam))
        st, fb = {}, np.zeros((H, W, 4), np.uint8)
        up = rec.step(n("upsample"), lambda: pt.upsample(d, rad_low, aov_low, aov, framebuffer=fb, stats=st))
        rec.put(n("upsample"), "radiance", up)
        rec.put(n("upsample"), "bgra", fb)
        rec.stats(n("upsample"), st)
        # adaptive sampling
        rad_a, fb = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 4), np.uint8)
        tiles = ((H + 15) // 16, (W + 15) // 16)
        tspp, terr = np.zeros(tiles, np.int32), np.zeros(tiles, np.float32)
        st = rec.step(n("adaptive"), lambda: pt.doTraceAdaptive(d, cam, fb, min_spp=4, max_spp=16, seed=seed,
                                                                max_depth=depth, radiance=rad_a, tile_spp=tspp,
                                                                tile_error=terr))
        rec.put(n("adaptive"), "radiance", rad_a)
        rec.put(n("adaptive"), "bgra", fb)
        rec.put(n("adaptive"), "tile_spp", tspp)
        rec.put(n("adaptive"), "tile_error", terr)
        rec.stats(n("adaptive"), st)
        # one object moved, the trees refitted
        moved = s.vert_trans[:1].copy()
        moved[0, 12:15] += np.float32(0.0625)
        rec.step(n("set_transforms"), lambda: d.set_transforms(0, moved))
        rec.stats(n("refit"), rec.step(n("refit"), d.refit))
        render(rec, n("refit_render"), pt, d, cam, seed, depth)
        # back where it was, by a build whose host half runs beside the render's first launches
        rec.step(n("set_transforms_back"), lambda: d.set_transforms(0, s.vert_trans[:1]))
        rec.step(n("build_async"), lambda: d.build(asynchronous=True))
        render(rec, n("async_render"), pt, d, cam, seed, depth)


def phase_steady(out):
    conc = [Handles(i, name) for i, name in enumerate(STEADY_SCENES)]
    twin = [Handles(i, name) for i, name in enumerate(STEADY_SCENES)]
    # the workers first: the serial run would fill the process's caches (the trace variants' LDS fits,
    # the kernels' code objects) before any two threads could meet in them
    run_workers(out, [(f"t{h.i}_{h.name}", (lambda rec, h=h: steady_script(rec, h))) for h in conc])
    for h in twin:
        steady_script(Rec(out, "serial", f"t{h.i}_{h.name}"), h)
    for h in conc + twin:
        h.close()


# ---- env: two scenes render against one env handle ----

ENV_SCENES = ["ball", "box1"]


def env_script(rec, i, s, d, env):
    W, H = frame_size(i)
    pt = T.PathTracer("", W, H, 0)
    pt.envLight = env
    seed, depth = 42 + i, 8
    render(rec, "env", pt, d, s.m_camera, seed, depth)
    render(rec, "env_is", pt, d, s.m_camera, seed, depth, flags=_lib.FLAG_ENV_IS)
    render(rec, "env_is_wavefront", pt, d, s.m_camera, seed, depth, flags=_lib.FLAG_ENV_IS | _lib.FLAG_WAVEFRONT)


def phase_env(out):
    def handles():
        made = [device_scene(name) for name in ENV_SCENES]
        for _, d in made:
            d.build()
        return T.EnvLight(T.procedural_sky(256, 128)), made
    env, made = handles()
    twin_env, twin = handles()
    run_workers(out, [(f"t{i}_{name}", (lambda rec, i=i: env_script(rec, i, *made[i], env)))
                      for i, name in enumerate(ENV_SCENES)])
    for i, name in enumerate(ENV_SCENES):
        env_script(Rec(out, "serial", f"t{i}_{name}"), i, *twin[i], twin_env)
    for _, d in made + twin:
        d.close()
    env.close()
    twin_env.close()


# ---- churn: handles come and go on one thread while two others render ----

CHURN_ROUNDS, CHURN_FRAMES = 5, 6


def churn_script(rec):
    W, H = frame_size(0)
    for k in range(CHURN_ROUNDS):
        s, d = rec.step(f"create{k}", lambda: device_scene("box"))
        rec.step(f"build{k}", lambda: d.build(asynchronous=k % 2 == 1))
        hist = rec.step(f"history_create{k}", lambda: T.History(d, W, H))
        pt = T.PathTracer("", W, H, 0)
        pt.envLight = rec.step(f"env_create{k}", lambda: T.EnvLight(T.procedural_sky(64, 32)))
        render(rec, f"frame{k}", pt, d, s.m_camera, 42 + k, 8)
        rec.step(f"history_close{k}", hist.close)     # each frees device memory: the device synchronises
        rec.step(f"env_close{k}", pt.envLight.close)
        rec.step(f"close{k}", d.close)


def frames_script(rec, i, name, s, d):
    W, H = frame_size(i)
    pt = T.PathTracer("", W, H, 0)
    for k in range(CHURN_FRAMES):
        render(rec, f"frame{k}", pt, d, s.m_camera, 42 + i + 10 * k, depth_of(name))


def phase_churn(out):
    steady = [(1, "tir"), (2, "box2")]
    made = {i: device_scene(name) for i, name in steady}
    twin = {i: device_scene(name) for i, name in steady}
    for _, d in list(made.values()) + list(twin.values()):
        d.build()
    run_workers(out, [("t0_box", churn_script)] +
                [(f"t{i}_{name}", (lambda rec, i=i, name=name: frames_script(rec, i, name, *made[i])))
                 for i, name in steady])
    churn_script(Rec(out, "serial", "t0_box"))
    for i, name in steady:
        frames_script(Rec(out, "serial", f"t{i}_{name}"), i, name, *twin[i])
    for _, d in list(made.values()) + list(twin.values()):
        d.close()


PHASES = {"first": phase_first, "steady": phase_steady, "env": phase_env, "churn": phase_churn}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", required=True, choices=sorted(PHASES))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    forced = os.environ.get("TPT_TEST_FORCE_FLAGS")      # as tests/conftest.py: a whole suite through a variant
    if forced:
        T.test_force_flags = int(forced, 0)
    T.lib()
    out = {}
    try:
        PHASES[args.phase](out)
    except WorkersFailed:
        pass
    np.savez(args.out, **out)
    print(f"{args.phase}: {len(out)} arrays, {len(out['errors'])} worker errors", flush=True)


if __name__ == "__main__":
    main()
