"""Device time and launch count of the stream preview (include/orip.h: orip_stream_preview), and the numpy double's time on the same inputs.
Two streams: the stage-13 stream of the bench configuration (synthetic 4096 x 4096 image, 8 layers, default canvas 8400 x 11880 steps) and a
seeded 64 MB synthetic stream with heavy overdraw; both drawn with the stage-14 parameters (1200 x 900, RGBK, taps, clip, white).
usage: python tools/time_stream_preview.py [--reps N] [--no-double] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

KERNELS = ("k_sp_reduce", "k_sp_scan", "k_sp_draw", "k_sp_resolve")


def bench_stream(size=4096, K=8):
    from orip.config import Config, canvas_size_px
    from orip.device import Device
    from orip import stages as S, stream as ST
    from orip.synth import synth_image, layer_names
    img = synth_image(size, size, K)
    cfg = Config(); cfg.color_names = layer_names(K)
    dev = Device(0)
    try:
        ops = S.run_path(img, cfg, dev)
        W, H = canvas_size_px(cfg)
        layers = [(n, i, ops[n]) for i, n in enumerate(cfg.color_names)]
        data, _ = ST.build_stream(layers, W, H, ST.stream_config_from_pipeline(cfg), color_maps=ST.load_color_maps(cfg), device=dev)
    finally:
        dev.close()
    return data, cfg


def synth_stream(nbytes, seed=64):
    """random walk with heavy overdraw: 90 % step bytes (half of them double), pen / colour / tap / speed / unknown service bytes, no EOF"""
    rng = np.random.default_rng(seed)
    b = (0x80 | rng.integers(0, 128, nbytes)).astype(np.uint8)
    u = rng.random(nbytes)
    b[u < 0.10] = 0x02
    b[(u >= 0.10) & (u < 0.12)] = 0x01
    b[(u >= 0.12) & (u < 0.13)] = (0x08 + rng.integers(0, 8, int(((u >= 0.12) & (u < 0.13)).sum()))).astype(np.uint8)
    b[(u >= 0.13) & (u < 0.1302)] = 0x03
    b[(u >= 0.1302) & (u < 0.135)] = 0x45
    b[(u >= 0.135) & (u < 0.136)] = 0x20
    return b.tobytes()


def time_one(dev, data, W, H, reps):
    from orip import stream_preview as SP
    SP.preview(dev, data, W, H)                                    # warm-up: code objects, buffer growth
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); rgb, st = SP.preview(dev, data, W, H); t.append(time.perf_counter() - t0)
    dev.prof_reset(); dev.prof_enable(True)
    for _ in range(reps):
        SP.preview(dev, data, W, H)
    dev.prof_enable(False)
    per = {k: dev.prof_get(k) for k in KERNELS}
    dev_ms = sum(ms for ms, _ in per.values()) / reps
    launches = sum(n for _, n in per.values()) // reps
    return {"bytes": len(data), "commands": st["commands"], "call_ms_median": 1e3 * float(np.median(t)), "call_ms_min": 1e3 * min(t),
            "kernel_ms": dev_ms, "kernels_per_call": launches, "memsets_per_call": 1, "copies_per_call": 3,
            "per_kernel_ms": {k: ms / reps for k, (ms, _) in per.items()}}, rgb, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-double", action="store_true")
    ap.add_argument("--synth-mb", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    from orip import stream_preview as SP
    import stream_preview_double as D
    t0 = time.perf_counter(); bench_data, cfg = bench_stream(); t_build = time.perf_counter() - t0
    W, H, inv = SP.canvas_for_output("/nonexistent", cfg)
    streams = {"bench_stage13": bench_data, f"synth_{a.synth_mb}MB": synth_stream(a.synth_mb << 20)}
    res = {"canvas": [W, H], "render": [1200, 900], "bench_stream_build_s": t_build}
    dev = Device(0)
    try:
        for name, data in streams.items():
            r, rgb, st = time_one(dev, data, W, H, a.reps)
            if not a.no_double:
                t0 = time.perf_counter(); rgb2, st2 = D.preview(data, W, H, 1200, 900); r["double_s"] = time.perf_counter() - t0
                r["double_equal"] = bool(np.array_equal(rgb, rgb2) and st == st2)
            res[name] = r
            print(name, json.dumps(r), flush=True)
    finally:
        dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
