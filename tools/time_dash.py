"""What the dash pass costs (csrc/gcode_dash.hip), on three drawings in steps: "lines", --strokes two-point lines of 4000 steps, dashed 2 mm on and 1 mm off at
40 steps per mm (one segment with 67 cut points, 34 dashes: the wave's case); "curves", --strokes flattened curves of about 400 points with the same pattern
(thousands of vertices per stroke, a dash over many of them: the scans' case); "solid", the lines with no pattern (the price of the pass when it has nothing
to do, to set beside the dedup's no-op case).  Per drawing: the orip_gcode_dash call on the uploaded step polylines by the host clock (the call ends in a
stream synchronisation; the upload is inside it, the fetches are not), median of --reps after one warm-up call; its phases (orip_prof_get, in runs of their
own: every timed scope ends in an event wait); the stats; the same clock around orip_gcode_to_steps on the same drawing in mm and around orip_gcode_dedup;
the bytes the pass must read and write (the input points and offsets, the output points, offsets and origins) and the time a device-to-device copy of as many
bytes takes at the copy bandwidth measured here (ten copies in a row of a 256 MiB buffer between two device buffers, by the host clock, ending in a device synchronise); and the comparison with
the sequential definition (tests/dash_double.py) on the first --check strokes.  --lib FILE loads another build of the library, such as one with another
DS_THREAD_CUTS, the cut points a thread writes before a wave takes the segment.  --hand-over NEVER ALWAYS takes two such builds (csrc/gcode_dash.hip compiled
with -DDS_THREAD_CUTS=1073741824, where a thread never hands over, and with -DDS_THREAD_CUTS=0, where every segment with a cut point goes to a wave) and times
the lines at HAND_OVER_STEPS lengths, L / 60 cut points per line, with each of them, one child process per run (a process loads one build): "hand_over" in the
result, the ds_emit phase and the call on both sides of every count, which is what the committed threshold rests on.
usage: python tools/time_dash.py [--strokes N] [--reps K] [--check N] [--line-steps L] [--only NAME] [--lib FILE] [--hand-over NEVER ALWAYS] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SPM, U = 40.0, 256
PATTERN = [int(round(2 * SPM * U)), int(round(1 * SPM * U))]                     # 2 mm on, 1 mm off
PHASES = ("ds_len", "ds_count", "ds_emit", "ds_compact")
HAND_OVER_STEPS = (120, 240, 480, 960, 1200, 1440, 1680, 1920, 3840)             # 2, 4, 8, 16, 20, 24, 28, 32, 64 cut points per line


def lines(n, steps=4000):
    """n two-point lines of about `steps` steps, oblique, one above the other"""
    y = 10 * np.arange(n, dtype=np.int64)
    pts = np.stack([np.stack([np.full(n, 100), y], 1), np.stack([np.full(n, 100 + steps - steps // 200), y + steps // 10], 1)], 1).reshape(-1, 2)
    return 2 * np.arange(n + 1, dtype=np.int64), pts.astype(np.int32)


def curves(n, k=400, seed=7):
    """n flattened curves of k points: chords of 2 .. 5 steps along a slow sine"""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.integers(2, 6, (n, k)), 1) + 50
    ph = rng.random((n, 1)) * 6.28
    y = np.rint(300 + 250 * np.sin(x / 180.0 + ph)).astype(np.int64) + 700 * np.arange(n)[:, None] % (1 << 29)
    return k * np.arange(n + 1, dtype=np.int64), np.stack([x, y], 2).reshape(-1, 2).astype(np.int32)


def clock(fn, reps):
    t = []
    for rep in range(reps + 1):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        if rep:
            t.append(t1 - t0)
    return {"s_median": float(np.median(t)), "s_min_max": [float(min(t)), float(max(t))]}


def copy_bandwidth(reps):
    """bytes read plus bytes written per second of a device-to-device copy of 256 MiB: ten copies in a row between two device buffers by the host clock,
    ending in a device synchronise, median of reps after a warm-up; through the HIP runtime the library itself has loaded"""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    size, a, b = 1 << 28, C.c_void_p(), C.c_void_p()

    def ck(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    ck(hip.hipMalloc(C.byref(a), C.c_size_t(size))); ck(hip.hipMalloc(C.byref(b), C.c_size_t(size)))
    try:
        ck(hip.hipMemset(a, 1, C.c_size_t(size)))
        t = []
        for rep in range(reps + 1):
            ck(hip.hipDeviceSynchronize())
            t0 = time.perf_counter()
            for _ in range(10):
                ck(hip.hipMemcpyAsync(b, a, C.c_size_t(size), 3, None))          # hipMemcpyDeviceToDevice, the null stream
            ck(hip.hipDeviceSynchronize())
            if rep:
                t.append((time.perf_counter() - t0) / 10)
    finally:
        hip.hipFree(a); hip.hipFree(b)
    return 2.0 * size / float(np.median(t))


def hand_over(never, always, strokes, reps):
    """the lines at every length of HAND_OVER_STEPS with both builds, each run a child process of this tool: {cut points: {build: times}}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for L in HAND_OVER_STEPS:
            row = {}
            for name, path in (("thread_only", never), ("always_a_wave", always)):
                f = os.path.join(tmp, f"{L}_{name}.json")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "lines", "--line-steps", str(L), "--lib", path, "--strokes", str(strokes), "--reps", str(reps),
                                "--out", f], check=True, stdout=subprocess.DEVNULL, timeout=300)
                with open(f) as fh:
                    r = json.load(fh)["inputs"]["lines"]
                row[name] = {"call_s_median": r["dash"]["s_median"], "ds_emit_s_median": r["phases_s_median"]["ds_emit"], "dashes": r["stats"]["dashes"],
                             "equals_sequential_definition": r["equals_sequential_definition"]}
            out[str(L // 60)] = dict(row, line_steps=L)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strokes", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=200)
    ap.add_argument("--line-steps", type=int, default=4000, help="the length of the two-point lines: 120 steps to the period, two cut points each")
    ap.add_argument("--only", default=None, help="one of lines, curves, solid")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--hand-over", nargs=2, metavar=("NEVER", "ALWAYS"), default=None, help="two builds of the library: a thread never hands over / always does")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip import lib
    if a.lib:
        lib.LIB_PATH = os.path.abspath(a.lib)
    from orip.device import Device
    import dash_double as DD
    n = a.strokes
    inputs = {"lines": (lines(n, a.line_steps), 0), "curves": (curves(n), 0), "solid": (lines(n, a.line_steps), -1)}
    if a.only:
        inputs = {a.only: inputs[a.only]}
    sweep = hand_over(a.hand_over[0], a.hand_over[1], n, a.reps) if a.hand_over else None      # before this process opens the device
    res = {"strokes": n, "line_steps": a.line_steps, "pattern_u": PATTERN, "steps_per_mm": SPM, "reps": a.reps, "lib": a.lib, "inputs": {}}
    dev = Device(0)
    try:
        res["copy_bytes_per_s"] = bw = copy_bandwidth(max(a.reps, 3))
        po, pv = np.array([0, 2], np.int32), np.array(PATTERN, np.int64)
        m = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=SPM, W=1 << 30, H=1 << 30, invert_y=0)
        for name, ((off, pts), q) in inputs.items():
            o = np.ascontiguousarray(off, np.int64); p = np.ascontiguousarray(pts, np.int32)
            pa, ph = np.full(n, q, np.int32), np.zeros(n, np.int64)
            st8, st9 = np.zeros(8, np.int64), np.zeros(9, np.int64)
            call = lambda: dev._ck(dev.L.orip_gcode_dash(dev.h, o.ctypes.data, p.ctypes.data, pa.ctypes.data, ph.ctypes.data, n, po.ctypes.data, pv.ctypes.data, 1, st8.ctypes.data))
            r = {"strokes": n, "points": len(p)}
            r["dash"] = clock(call, a.reps)
            r["stats"] = st = {k: int(v) for k, v in zip(lib.DASH_STATS, st8)}
            kern = {k: [] for k in PHASES}
            for rep in range(a.reps):
                dev.prof_reset(); dev.prof_enable(True)
                call()
                dev.prof_enable(False)
                for k in kern:
                    kern[k].append(dev.prof_get(k)[0] * 1e-3)
            r["phases_s_median"] = {k: float(np.median(v)) for k, v in kern.items()}
            mm = p.astype(np.float64) / SPM
            r["to_steps"] = clock(lambda: dev.gcode_to_steps(o, mm, m), a.reps)
            r["dedup"] = clock(lambda: dev._ck(dev.L.orip_gcode_dedup(dev.h, o.ctypes.data, p.ctypes.data, None, n, 1, st9.ctypes.data)), a.reps)
            r["bytes_in_out"] = b = 8 * len(p) + 8 * (n + 1) + 8 * st["points_out"] + 8 * (st["paths_out"] + 1) + 4 * st["paths_out"]
            r["copy_bound_s"] = b / bw
            r["dash_over_copy_bound"] = r["dash"]["s_median"] / r["copy_bound_s"]
            k = min(a.check, n)
            sub = (o[:k + 1], p[:int(o[k])], pa[:k], ph[:k], po, pv)
            got, want = dev.gcode_dash(*sub), DD.dash_numpy(*sub)
            r["equals_sequential_definition"] = bool(all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == want[3])
            res["inputs"][name] = r
    finally:
        dev.close()
    if sweep is not None:
        res["hand_over"] = sweep
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
