"""What --ring-entry costs and what it buys (csrc/gcode_order.hip: orip_gcode_order_rings alone, explicit form, so the call's uploads, its read-backs and
its two synchronisations are in the host time), beside its yardstick on the same strokes: orip_gcode_order_pens on their ends plus orip_gcode_seam -- the
walk now buckets L candidates per ring instead of one.  Three inputs: a 20 x 20 grid of circles of 64 vertices (the sheet of the README's prototype figure);
--rings circles of 64 vertices on a grid; --open open strokes and no ring: what the candidate grid costs when it buys nothing.  Per input: the host time of
each call (median of --reps after a warm-up call), the device time of the chains (k_ro_chain, k_op_chain; HIP events), and the pen-up steps under four
settings: the plain order, plain + --loop-start, --ring-entry, --ring-entry + --loop-start (the seam pass on the rotated strokes).
usage: python tools/time_ring_entry.py [--rings N] [--open N] [--reps K] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def circles(count, vertices=64, radius=150, pitch=400, seed=3):
    """(off, pts): `count` circles on a square grid in row order, each stored from a seeded angle"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(count)))
    i = np.arange(count)
    c = np.stack([radius + 50 + pitch * (i % side), radius + 50 + pitch * (i // side)], 1)
    a = 2.0 * np.pi * np.arange(vertices)[None, :] / vertices + rng.uniform(0, 6.28, count)[:, None]
    ring = np.stack([np.rint(c[:, None, 0] + radius * np.cos(a)), np.rint(c[:, None, 1] + radius * np.sin(a))], 2).astype(np.int32)
    return np.arange(count + 1, dtype=np.int64) * (vertices + 1), np.concatenate([ring, ring[:, :1]], 1).reshape(-1, 2)


def open_strokes(count, seed=4):
    rng = np.random.default_rng(seed)
    side = 400 * int(np.ceil(np.sqrt(count)))
    a = rng.integers(0, side, (count, 2)); b = np.clip(a + rng.integers(-300, 301, (count, 2)), 0, side)
    return np.arange(count + 1, dtype=np.int64) * 2, np.stack([a, b + (a == b).all(1)[:, None]], 1).reshape(-1, 2).astype(np.int32)


def median_ms(dev, call, scope, reps):
    host, device, out = [], [], None
    for rep in range(reps + 1):
        dev.prof_reset()
        t0 = time.perf_counter(); out = call(); t1 = time.perf_counter()
        if rep:                                                               # the first call loads code objects and grows buffers
            host.append(t1 - t0); device.append(dev.prof_get(scope)[0])
    return out, 1e3 * float(np.median(host)), float(np.median(device))


def timed(dev, off, pts, reps):
    from orip import gcode as GC
    n = len(off) - 1
    ends, grp = GC.path_ends(off, pts), np.zeros(n, np.int32)
    (order, rev), pens_ms, pens_chain = median_ms(dev, lambda: dev.gcode_order_pens(ends, grp, 1), "k_op_chain", reps)
    (seam, sst), seam_ms, _ = median_ms(dev, lambda: dev.gcode_seam(off, pts, order, rev), "k_sm_back", reps)
    (r_order, r_rev, r_seam, rst), ring_ms, ring_chain = median_ms(dev, lambda: dev.gcode_order_rings(off, pts, grp, 1), "k_ro_chain", reps)
    by_stroke = np.zeros(n, np.int64); by_stroke[r_order] = r_seam
    rotated = GC.gather_paths(off, pts, np.arange(n), None, by_stroke)[1]
    _, sst2 = dev.gcode_seam(off, rotated, r_order, r_rev)
    assert sst["travel_before"] == GC.travel_steps(*GC.gather_paths(off, pts, order, rev)) and sst2["travel_before"] == rst["travel"]
    return {"strokes": n, "points": len(pts), "candidates": rst["candidates"], "reps": reps,
            "order_pens_host_ms": pens_ms, "order_pens_chain_ms": pens_chain, "seam_host_ms": seam_ms, "order_rings_host_ms": ring_ms, "order_rings_chain_ms": ring_chain,
            "travel": {"plain": sst["travel_before"], "plain_loop_start": sst["travel_after"], "ring_entry": rst["travel"], "ring_entry_loop_start": sst2["travel_after"]},
            "moved": rst["moved"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=10000)
    ap.add_argument("--open", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    res = {}
    dev = Device(0)
    try:
        dev.prof_enable(True)
        res["grid_400"] = timed(dev, *circles(400), a.reps)
        res["circles"] = timed(dev, *circles(a.rings), a.reps)
        res["open_only"] = timed(dev, *open_strokes(a.open), a.reps)
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
