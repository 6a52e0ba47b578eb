"""Occupancy timeline of one k_trace launch from a per-wave dump.

The dump (TPT_DEBUG_WAVES=<file> with a TPT_PROFILE_PHASES build) holds 8 u64 per
wave: start tick, life, traversal steps, shading passes, rays, 4-wide visits,
the heaviest lane's rays, shading-pass ticks (s_memrealtime, 100 MHz).  A wave's
record sits at index tile * 4 + sub-tile of its launch's region, whatever the
workgroup shape, so the waves of one workgroup are `wg` consecutive records.

Prints how long the launch ran with the chip full (live waves >= the resident
capacity) and the tail: the time from the last wave start to the launch end,
and the wave-time the chip could have held but did not (idle slot fraction).

Grouped by workgroup (a workgroup's LDS and its waves' slots are only handed on
as a unit once its last wave ends):
  hole       sum over waves (workgroup end - wave end) /
             sum over waves (workgroup end - wave start): the share of the
             slot time workgroups hold that their finished waves leave empty;
  tail hole  the same ratio over the time after the launch's last wave start
             (launches=K: the file's K equal regions are K launches, each with
             its own last start; the sums run over all of them);
  held       slot utilisation with a wave's slot counted until its workgroup
             ends (slots held, not only live).
Usage: python tools/wave_timeline.py dump.bin [capacity=5120] [wg=4] [launches=1]
"""
import sys

import numpy as np


def utilisation(start, end, cap, span):
    """Integral of min(live, cap) over the launch, as a fraction of cap * span,
    the live counts and the event times."""
    ev = np.concatenate([np.stack([start, np.ones_like(start)], 1), np.stack([end, -np.ones_like(end)], 1)])
    ev = ev[np.argsort(ev[:, 0], kind="stable")]
    live = np.cumsum(ev[:, 1])
    dt = np.diff(np.append(ev[:, 0], span))
    util = float((np.minimum(live, cap) * dt).sum() / (cap * span))
    return util, live, dt, ev


def hole_sums(start, end, wg_end, after=None):
    """(empty, held) slot time of waves in their workgroups, optionally only after time `after`."""
    if after is not None:
        start = np.maximum(start, after)
        end = np.maximum(end, after)
        wg_end = np.maximum(wg_end, after)
    return float((wg_end - end).sum()), float((wg_end - start).sum())


def main():
    raw = np.fromfile(sys.argv[1], dtype=np.uint64).reshape(-1, 8).astype(np.float64)
    cap = int(sys.argv[2]) if len(sys.argv) > 2 else 5120
    wg = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    launches = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    if wg not in (1, 2, 4) or launches < 1 or len(raw) % launches != 0:
        sys.exit("wave_timeline: wg is 1, 2 or 4 and the dump holds `launches` equal regions")
    ran = raw[:, 1] > 0
    ids = np.nonzero(ran)[0]
    d = raw[ran]
    t0 = d[:, 0].min()
    start = (d[:, 0] - t0) / 100.0   # us
    end = start + d[:, 1] / 100.0
    span = end.max()
    util, live, dt, ev = utilisation(start, end, cap, span)
    full = float(dt[live >= cap * 0.98].sum())
    last_start = start.max()
    life = d[:, 1] / 100.0
    order = np.argsort(-life)
    print(f"waves {len(d)}  launch {span / 1000:.2f} ms  slot utilisation {util:.3f}  "
          f"chip-full {full / 1000:.2f} ms  last start {last_start / 1000:.2f} ms  "
          f"tail after last start {(span - last_start) / 1000:.2f} ms")
    print(f"wave life ms: mean {life.mean() / 1000:.2f}  median {np.median(life) / 1000:.2f}  "
          f"p99 {np.percentile(life, 99) / 1000:.2f}  max {life.max() / 1000:.2f}")
    for q in (0.5, 0.75, 0.9, 0.95, 0.99):
        # time at which the live count first drops below q*cap for good
        above = np.nonzero(live >= q * cap)[0]
        t = ev[above[-1] + 1, 0] if len(above) and above[-1] + 1 < len(ev) else span
        print(f"  live < {q:.2f}*cap from {t / 1000:.2f} ms ({(span - t) / span * 100:.1f} % of the launch)")
    # by workgroup: records of one workgroup are wg consecutive ids (regions are multiples of 4 records)
    group = ids // wg
    _, inv = np.unique(group, return_inverse=True)
    g_end = np.zeros(inv.max() + 1)
    np.maximum.at(g_end, inv, end)
    wg_end = g_end[inv]
    empty, held = hole_sums(start, end, wg_end)
    per = len(raw) // launches
    region = ids // per
    t_empty = t_held = 0.0
    for k in range(launches):
        m = region == k
        if m.any():
            e, h = hole_sums(start[m], end[m], wg_end[m], after=start[m].max())
            t_empty += e
            t_held += h
    util_held = utilisation(start, wg_end, cap, span)[0]
    sizes = np.bincount(inv)
    partly = float((np.bincount(inv, weights=(wg_end - end > 0).astype(np.float64)) > 0).mean())
    print(f"workgroups {len(g_end)} of {wg} waves (mean {sizes.mean():.2f} ran)  "
          f"hole {empty / max(held, 1e-9):.4f}  tail hole {t_empty / max(t_held, 1e-9):.4f} "
          f"({launches} launch{'es' if launches > 1 else ''}; tail slot time {t_held / max(held, 1e-9) * 100:.1f} % of all held)  "
          f"slot utilisation held {util_held:.3f} (live {util:.3f})")
    print(f"  empty slot time {empty / 1e6:.3f} wave-s of {held / 1e6:.3f} held; "
          f"{empty / (cap * span) * 100:.2f} % of the chip's slot time over the launch; "
          f"workgroups with a wave ending early {partly * 100:.1f} %")
    print("heaviest waves (start ms, life ms, rays, wide, max lane rays):")
    for i in order[:5]:
        print(f"  {start[i] / 1000:8.2f} {life[i] / 1000:8.2f} {int(d[i, 4]):10d} {int(d[i, 5]):10d} {int(d[i, 6]):8d}")


if __name__ == "__main__":
    main()
