"""bench.py's plain run, --full and --dump-outputs.

* CPU: the dump writer keeps a frame within the budget whole, and writes a
  larger one as a fixed sample of its pixels, the same on every call.
* GPU: a plain run times exactly --steps steps, reports ms_per_step, runs none
  of the --full measurements, and dumps the frame its last timed step returned:
  the same frame bit for bit as one doTrace of the same arguments; --full
  reports the tolerance mode beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, scene_path

W, H, SPP, DEPTH, SEED = 256, 144, 8, 8, 42
SMALL = ["--gpus", "1", "--width", str(W), "--height", str(H), "--spp", str(SPP), "--depth", str(DEPTH),
         "--seed", str(SEED)]


def test_dump_writer_whole_and_sampled(tmp_path, monkeypatch):
    import torch

    import bench
    n_pix = 36 * 64
    frame = torch.arange(n_pix, dtype=torch.float32).repeat_interleave(3).reshape(36, 64, 3)   # pixel p = (p, p, p)
    bench.dump_outputs(str(tmp_path), frame, 0, 1)
    a = np.load(tmp_path / "radiance.npy")
    assert a.dtype == np.float32 and a.shape == (36, 64, 3) and np.array_equal(a, frame.numpy())
    bench.dump_outputs(str(tmp_path), None, 1, 1)            # a rank that holds no frame writes nothing
    assert sorted(os.listdir(tmp_path)) == ["radiance.npy"]
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * (4096 + 600 * 12))
    bench.dump_outputs(str(tmp_path), frame, 1, 2)           # 2 writers: 600 pixels each
    s = np.load(tmp_path / "radiance_rank1.npy")
    assert s.dtype == np.float32 and s.shape == (600, 3)
    ids = s[:, 0].astype(int)
    assert (np.diff(ids) > 0).all() and ids.min() >= 0 and ids.max() < n_pix   # distinct pixels, ascending
    assert np.array_equal(s, frame.numpy().reshape(-1, 3)[ids])
    bench.dump_outputs(str(tmp_path / "again"), frame, 1, 2)
    assert np.array_equal(np.load(tmp_path / "again" / "radiance_rank1.npy"), s)
    assert 2 * os.path.getsize(tmp_path / "radiance_rank1.npy") <= bench.DUMP_BUDGET_BYTES


def _bench(extra, timeout=240):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_frame(tmp_path, gpu_available):
    import tinypathtracer_amd as T
    out = tmp_path / "dump"
    d = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    # value = rays of the 3 timed steps / their time (ms_per_step and value are rounded in the line)
    rays = d["gpu_traversals"] + d["local_rays"]            # of the 3 timed steps together
    assert d["value"] == pytest.approx(rays / (3 * d["ms_per_step"] * 1e3), rel=1e-2)
    for key in ("cpu_baseline", "tolerance_mode", "weak"):
        assert key not in d
    assert sorted(os.listdir(out)) == ["radiance.npy"]
    got = np.load(out / "radiance.npy")
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    scene = T.Scene(scene_path("box"))
    dev = scene.copySceneToDevice(0).build()
    rad = np.zeros((H, W, 3), np.float32)
    st = T.PathTracer("", W, H, 0).doTrace(dev, scene.m_camera, None, SPP, seed=SEED, max_depth=DEPTH, radiance=rad)
    dev.close()
    assert st["traversals"] * 3 == rays                      # every timed step rendered this frame
    assert np.array_equal(got.view(np.uint32), rad.view(np.uint32))


@pytest.mark.gpu
def test_full_run_adds_the_tolerance_mode(gpu_available):
    d = _bench(["--steps", "1", "--warmup", "0", "--full", "--cpu-baseline", "0"])
    assert d["steps"] == 1 and d["ms_per_step"] > 0
    t = d["tolerance_mode"]
    assert t["unit"] == "Mrays/s" and t["value"] > 0 and t["flags"] == "TPT_FLAG_FAST"
    assert "cpu_baseline" not in d
