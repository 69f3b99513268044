"""Where the time of gcode2stream goes (orip/gcode.py, csrc/gcode.hip, csrc/gcode_order.hip, csrc/stream.hip), on seeded synthetic plots.
  whole   : parse / to-steps / order / plan / codes / pack + fetch of a hatch-like plot of --paths paths on A4 at 40 steps per mm, through
            build_stream_from_gcode, and the whole script on the same file as a child process
  order   : the order kernel alone at several sizes of uniformly spread paths (call time, k_gc_chain time, time per step) and for a star
            (every path starts on one point); at --check-size the result is compared with the numpy definition (tests/gcode_double.py)
  pack    : orip_stream_pack + the fetch of the bytes on one piece table of about --pack-steps steps, next to orip_stream_codes with and without
            the fetch of the codes
usage: python tools/time_gcode.py [--paths N] [--order-sizes 25000,50000,...] [--star N] [--pack-steps N] [--skip whole,order,pack] [--out FILE.json]"""
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


def synth_gcode(n_paths, seed=1, w_mm=200.0, h_mm=287.0):
    """a hatch-filled page: n short strokes of 1-3 segments, uniformly spread, in file order unrelated to position"""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform([5, 5], [w_mm, h_mm], (n_paths, 2))
    k = rng.integers(1, 4, n_paths)
    lines = ["G21", "G90", "M5"]
    for i in range(n_paths):
        p = p0[i]
        lines.append(f"G0 X{p[0]:.3f} Y{p[1]:.3f}"); lines.append("M3")
        for _ in range(k[i]):
            p = p + rng.normal(0, 1.5, 2)
            lines.append(f"G1 X{p[0]:.3f} Y{p[1]:.3f}")
        lines.append("M5")
    return "\n".join(lines) + "\n"


def uniform_ends(n, seed=2, W=8400, H=11880):
    rng = np.random.default_rng(seed)
    s = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    return np.concatenate([s, np.clip(s + rng.integers(-120, 121, (n, 2)), 0, [W - 1, H - 1])], 1).astype(np.int32)


def time_order(dev, ends, reps):
    dev.gcode_order(ends[:64])                                       # code objects
    call, kern = [], []
    for _ in range(reps):
        dev.prof_reset(); dev.prof_enable(True)
        t0 = time.perf_counter(); order = dev.gcode_order(ends); call.append(time.perf_counter() - t0)
        dev.prof_enable(False)
        kern.append(dev.prof_get("k_gc_chain")[0] * 1e-3)
    n = len(ends)
    return {"paths": n, "call_s_median": float(np.median(call)), "chain_s_median": float(np.median(kern)), "chain_us_per_step": 1e6 * float(np.median(kern)) / n,
            "reps": reps, "call_s": call, "chain_s": kern}, order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--order-sizes", default="25000,50000,100000,200000")
    ap.add_argument("--star", type=int, default=20000)
    ap.add_argument("--check-size", type=int, default=20000)
    ap.add_argument("--pack-steps", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    from orip.device import Device
    from orip import gcode as GC, stream as ST
    import gcode_double as D
    res = {}
    dev = Device(0)
    try:
        if "order" not in skip:
            res["order"] = []
            for n in [int(v) for v in a.order_sizes.split(",") if v]:
                e = uniform_ends(n)
                r, order = time_order(dev, e, a.reps)
                if n <= a.check_size:
                    t0 = time.perf_counter(); r["equals_numpy_definition"] = bool(np.array_equal(order, D.order_numpy(e))); r["numpy_definition_s"] = time.perf_counter() - t0
                res["order"].append(r); print("order", json.dumps(r), flush=True)
            rng = np.random.default_rng(3)
            star = np.concatenate([np.full((a.star, 2), 4000), rng.integers(0, 8000, (a.star, 2))], 1).astype(np.int32)
            r, order = time_order(dev, star, a.reps); r["case"] = "star"; r["equals_index_order"] = bool(np.array_equal(order, np.arange(a.star)))
            res["order"].append(r); print("order", json.dumps(r), flush=True)
        if "pack" not in skip:
            sc = ST.StreamConfig()
            rng = np.random.default_rng(4)
            nm = max(1, a.pack_steps // 5000)
            p = np.stack([rng.integers(0, 8400, nm + 1), rng.integers(0, 11880, nm + 1)], 1)
            moves = np.concatenate([p[:-1], p[1:]], 1).astype(np.int32)
            P = ST.fixed_plan(np.r_[[ST.PEN_UP], np.full(nm, -1)], moves)
            tm = {}; clk = [time.perf_counter()]

            def lap(name):
                t1 = time.perf_counter(); tm[name] = t1 - clk[0]; clk[0] = t1
            _, table, off = ST.compile_plan(P, sc, dev, lap=lap)       # its pack is the warm-up: buffers, code objects
            t_codes, t_plan = tm["codes"], tm["plan"]
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); data = dev.stream_pack(table); t.append(time.perf_counter() - t0)
            dev.prof_reset(); dev.prof_enable(True); dev.stream_pack(table); dev.prof_enable(False)
            r = {"steps": int(off[-1]), "pieces": len(table.pos), "bytes": len(data), "codes_s": t_codes, "plan_s": t_plan, "pack_and_fetch_s_median": float(np.median(t)),
                 "k_pk_bytes_ms": dev.prof_get("k_pk_bytes")[0]}
            t0 = time.perf_counter(); dev.stream_codes(moves); r["codes_with_fetch_s"] = time.perf_counter() - t0
            res["pack"] = r; print("pack", json.dumps(r), flush=True)
        if "whole" not in skip:
            t0 = time.perf_counter(); text = synth_gcode(a.paths); t_gen = time.perf_counter() - t0
            opts = GC.GcodeOptions()
            GC.build_stream_from_gcode(synth_gcode(500), opts, dev)  # code objects, first buffers
            tm = {}
            t0 = time.perf_counter(); data, info = GC.build_stream_from_gcode(text, opts, dev, timings=tm); t_all = time.perf_counter() - t0
            dev.prof_reset(); dev.prof_enable(True); GC.build_stream_from_gcode(text, opts, dev); dev.prof_enable(False)
            res["whole"] = {"paths_in_file": a.paths, "file_bytes": len(text), "generate_s": t_gen, "in_process_s": t_all, "stages_s": tm, "info": {k: v for k, v in info.items()},
                            "kernel_ms": {k: dev.prof_get(k)[0] for k in ("k_gc_points", "k_gc_emit", "k_gc_chain", "k_seg_codes", "k_pk_bytes")}}
            print("whole", json.dumps(res["whole"]), flush=True)
    finally:
        dev.close()
    if "whole" not in skip:
        with tempfile.TemporaryDirectory() as td:
            src = os.path.join(td, "in.gcode"); open(src, "w").write(text)
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream", "gcode2stream.py"), src, "-o", os.path.join(td, "out.bin")],
                               capture_output=True, text=True, timeout=900)
            res["whole"]["script_s"] = time.perf_counter() - t0; res["whole"]["script_rc"] = r.returncode
            res["whole"]["script_equal"] = r.returncode == 0 and open(os.path.join(td, "out.bin"), "rb").read() == data
        print("script", res["whole"]["script_s"], res["whole"]["script_rc"], res["whole"]["script_equal"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
