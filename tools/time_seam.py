"""What --loop-start costs (csrc/gcode_seam.hip: orip_gcode_seam alone, explicit form, so the call's upload and its two synchronisations are in the host
time), on three inputs: --rings circles of 64 vertices on a grid, all in one run (the chain of short layers: one block walks them); the same circles with
an open stroke after each, so that every run has one ring (no layer at all: the prepare kernels, the scan and the forward pass); and two rings of --large
vertices in a row (one large layer over many blocks).  Per input: the pairs sum of L_k * L_{k+1}, the host time of the call (median of --reps after a
warm-up call) and the device time of the three profiled scopes (k_sm_prepare, k_sm_back, k_sm_forward; HIP events), the travel before and after.
--hand-over: pairs of rings R x R' on both sides of SM_HAND_OVER, between two small rings: just under it the layer is walked by the run's one block, from
it on it gets blocks of its own.  A build with another constant (make EXTRA=-DSM_HAND_OVER_PAIRS=...) is timed by running this tool on it.
usage: python tools/time_seam.py [--rings N] [--large N] [--reps K] [--hand-over] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SCOPES = ("k_sm_prepare", "k_sm_back", "k_sm_forward")


def circles(count, vertices=64, radius=150, pitch=400, gap=False, seed=3):
    """(off, pts): `count` circles on a square grid in row order, each started at a seeded angle; gap: a short open stroke after every circle"""
    import seam_cases as SC
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(count)))
    strokes = []
    for i in range(count):
        cx, cy = radius + 50 + pitch * (i % side), radius + 50 + pitch * (i // side)
        strokes.append(SC.ring(cx, cy, radius, vertices, float(rng.uniform(0, 6.28))))
        if gap:
            strokes.append(SC.line(cx - 20, cy, cx + 20, cy + 10))
    off, pts, _, _, _ = SC.pack(strokes)
    return off, pts


def pairs_of(off, pts):
    L = np.diff(off)
    closed = (L >= 4) & (pts[off[:-1]] == pts[off[1:] - 1]).all(1)
    R = np.where(closed, L - 1, 0).astype(np.int64)
    return int((R[:-1] * R[1:]).sum())


def timed(dev, off, pts, reps):
    host, scopes, st = [], [], None
    for rep in range(reps + 1):
        dev.prof_reset()
        t0 = time.perf_counter(); seam, st = dev.gcode_seam(off, pts, None, None); t1 = time.perf_counter()
        if rep:                                                               # the first call loads code objects and grows buffers
            host.append(t1 - t0); scopes.append({k: dev.prof_get(k)[0] for k in SCOPES})
    return {"strokes": len(off) - 1, "points": len(pts), "pairs": pairs_of(off, pts), "host_ms_median": 1e3 * float(np.median(host)),
            "device_ms_median": {k: float(np.median([s[k] for s in scopes])) for k in SCOPES}, "reps": reps, "stats": st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=10000)
    ap.add_argument("--large", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hand-over", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    import seam_cases as SC
    res = {"hand_over_pairs": SC.HAND_OVER}
    dev = Device(0)
    try:
        dev.prof_enable(True)
        res["one_run"] = timed(dev, *circles(a.rings), a.reps)
        res["runs_of_one"] = timed(dev, *circles(a.rings, gap=True), a.reps)
        big = SC.pack([SC.ring(2 * a.large, 2 * a.large, a.large, a.large, 0.3), SC.ring(5 * a.large, 3 * a.large, a.large, a.large, 1.1)])
        res["two_large"] = timed(dev, big[0], big[1], a.reps)
        if a.hand_over:
            res["hand_over"] = {}
            for r, rn in ((512, 512), (724, 724), (1024, 1023), (1024, 1024), (1024, 1025), (1448, 1448), (2048, 2048), (4096, 4096)):
                case = SC.rings_in_a_row([64, r, rn, 64], 7, spread=20000)
                t = timed(dev, case[0], case[1], a.reps)
                res["hand_over"]["%dx%d" % (r, rn)] = dict(t, own_blocks=r * rn >= SC.HAND_OVER)
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
