"""include/tpt.h: "calls on different scenes may run concurrently from different host threads".
Every other GPU test drives the library from one thread; here up to eight threads call it at
once, each on scenes of its own, and a call made beside the others must give the bits it
gives alone: every output array and every counter equals the same call's on twin handles made
and used serially.  (The serial twins come from the code under test: that one thread's results
are right is what the rest of the suite establishes against the oracle.  The first phase also
holds the RNG states against the oracle, since a wrong jump table -- what the first scene of a
process found when another thread was still building it -- gives wrong frames whose serial
twins, rendered later, are right.)

What the threads share: the RNG's jump table (host/rng_host.cpp), the trace variants' LDS-fit
cache (trace.hip launch_one), the calling thread's current device and last error, an env
handle (phase env), the device itself when handles are destroyed (phase churn).

Each phase runs in a fresh child process (tests/threads_child.py): a hung thread cannot be
ended from inside pytest, and the first phase needs a process that has not used the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import threads_child as child
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

# what no two runs of a call share: the statistics' wall and event times
TIMING_FIELDS = ["rng_init_ms", "trace_ms", "resolve_ms", "total_ms", "trace_kernel_ms", "tree_wait_ms", "ms",
                 "error_ms", "pack_ms", "filter_ms", "estimate_ms", "kernel_ms", "box_ms"]


def run_phase(phase, tmp_path):
    out = str(tmp_path / f"{phase}.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "threads_child.py"), "--phase", phase,
                        "--out", out], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with np.load(out) as z:
        got = {k: z[k] for k in z.files}
    assert list(got.pop("errors")) == []          # each names its thread, scene and call
    return got


def same_as_serial(got, whos, steps):
    """Every thread's every array and counter equals its serial twin's, bit for bit; `steps`
    (per thread) are there: nothing was left out at run time."""
    conc = {k[len("conc__"):]: v for k, v in got.items() if k.startswith("conc__") and "__rng__" not in k}
    serial = {k[len("serial__"):]: v for k, v in got.items() if k.startswith("serial__")}
    assert sorted(conc) == sorted(serial)
    assert sorted({k.split("__")[0] for k in conc}) == sorted(whos)
    compared = 0
    for key, a in sorted(conc.items()):
        who, step, field = key.split("__")
        if field in TIMING_FIELDS:
            continue
        b = serial[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), \
            f"thread and scene {who}, call {step}, output {field}: differs from the serial twin" + \
            (f" in {int((a != b).sum())} of {a.size} values" if a.shape == b.shape else "")
        compared += 1
    for who in whos:
        have = {k.split("__")[1] for k in conc if k.startswith(who + "__")}
        missing = [s for s in steps(who) if s not in have]
        assert not missing, f"{who}: no record of {missing}"
        for s in steps(who):                       # a render that shaded nothing would compare equal too
            n = conc.get(f"{who}__{s}__traversals")
            assert n is None or int(n) > 0, (who, s)
    return compared


def test_first_use_from_eight_threads(gpu_available, tmp_path):
    """Eight threads make the process's first calls together: even threads create, build and
    render first and read RNG states after, odd threads the other way round."""
    got = run_phase("first", tmp_path)
    whos = [f"t{i}_{name}" for i, name in enumerate(child.FIRST_SCENES)]
    one = (O.C.c_uint32 * 6)()
    for i, who in enumerate(whos):
        for first in child.RNG_FIRSTS:
            want = np.zeros((child.RNG_COUNT, 6), np.uint32)
            for k in range(child.RNG_COUNT):
                O.lib().orc_xorwow_init(42 + i, first + k, one)
                want[k] = one[:]
            st = got[f"conc__{who}__rng__first{first}"]
            assert np.array_equal(st, want), f"{who}: RNG states from pixel {first} differ from the oracle's"
    same_as_serial(got, whos, lambda who: ["frame"])
    for i, who in enumerate(whos):
        W, H = child.frame_size(i)
        assert got[f"conc__{who}__frame__radiance"].shape == (H, W, 3)
        assert int(got[f"conc__{who}__frame__samples"]) == W * H * child.SPP


def steady_steps(who):
    name = who.split("_", 1)[1]
    steps = ["trace", "one_lane", "pair" if name in child.LIT else "four_lanes", "ref_order", "wavefront",
             "accumulate_a", "accumulate_b", "frames", "aov", "denoise", "temporal0", "temporal1", "temporal1_clip",
             "svgf", "upsample", "adaptive", "refit", "refit_render", "async_render"]
    if name == "tir":
        steps.append("aov_path")
    return [f"r{r}_{s}" for r in range(2) for s in steps]


def test_steady_state_every_entry_point(gpu_available, tmp_path):
    """Four threads, handles made beforehand, two rounds of a script through every entry-point
    family and trace family."""
    got = run_phase("steady", tmp_path)
    whos = [f"t{i}_{name}" for i, name in enumerate(child.STEADY_SCENES)]
    same_as_serial(got, whos, steady_steps)
    for who in whos:
        name = who.split("_", 1)[1]
        for step, n in (("one_lane", 1), ("pair", 2) if name in child.LIT else ("four_lanes", 4)):
            assert int(got[f"conc__{who}__r0_{step}__lanes_per_pixel"]) == n, (who, step)   # the mode asked for ran
        assert int(got[f"conc__{who}__r0_accumulate_b__accumulated_spp"]) == 4


def test_two_scenes_share_one_env(gpu_available, tmp_path):
    got = run_phase("env", tmp_path)
    whos = [f"t{i}_{name}" for i, name in enumerate(child.ENV_SCENES)]
    same_as_serial(got, whos, lambda who: ["env", "env_is", "env_is_wavefront"])
    for who in whos:   # the env is seen: importance sampling changes the frame
        assert not np.array_equal(got[f"conc__{who}__env__radiance"], got[f"conc__{who}__env_is__radiance"])


def test_handles_come_and_go_beside_renders(gpu_available, tmp_path):
    got = run_phase("churn", tmp_path)
    frames = [f"frame{k}" for k in range(child.CHURN_FRAMES)]
    same_as_serial(got, ["t0_box", "t1_tir", "t2_box2"],
                   lambda who: frames[:child.CHURN_ROUNDS] if who == "t0_box" else frames)
