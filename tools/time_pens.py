"""What the grouped, reversible order costs next to the order it grew from (csrc/gcode_order.hip: k_gc_chain, k_op_chain), on --paths uniformly spread paths on an
A4 step canvas (8400 x 11880), the input of tools/time_gcode.py's order section:
  parent          : orip_gcode_order
  one_group       : orip_gcode_order_pens, one group, no flag (the same work: the result must be equal)
  one_group_rev   : one group, ORIP_ORDER_REVERSE (twice the entries, one more removal per step)
  four_groups_rev : four groups, ORIP_ORDER_REVERSE
Per case the call time (host clock around a call that ends in a stream synchronisation) and the chain kernel's time, medians of --reps.  At --check-size
the grouped results are compared with the numpy definition (tests/pens_double.py).
usage: python tools/time_pens.py [--paths N] [--reps K] [--check-size N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from time_gcode import uniform_ends


def timed(dev, call, kernel, reps):
    call()                                                            # code objects, buffers
    t, k = [], []
    for _ in range(reps):
        dev.prof_reset(); dev.prof_enable(True)
        t0 = time.perf_counter(); out = call(); t.append(time.perf_counter() - t0)
        dev.prof_enable(False)
        k.append(dev.prof_get(kernel)[0] * 1e-3)
    return {"call_s_median": float(np.median(t)), "chain_s_median": float(np.median(k)), "reps": reps, "call_s": t, "chain_s": k}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check-size", type=int, default=8000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    import pens_double as PD
    n = a.paths
    ends = uniform_ends(n)
    grp4 = np.random.default_rng(5).integers(0, 4, n).astype(np.int32)
    one = np.zeros(n, np.int32)
    res = {"paths": n}
    dev = Device(0)
    try:
        res["parent"], base = timed(dev, lambda: dev.gcode_order(ends), "k_gc_chain", a.reps)
        res["one_group"], (o, r) = timed(dev, lambda: dev.gcode_order_pens(ends, one, 1), "k_op_chain", a.reps)
        res["one_group"]["equals_parent"] = bool(np.array_equal(o, base) and not r.any())
        res["one_group_rev"], (o, r) = timed(dev, lambda: dev.gcode_order_pens(ends, one, 1, True), "k_op_chain", a.reps)
        res["one_group_rev"]["reversed"] = int(r.sum())
        res["four_groups_rev"], (o, r) = timed(dev, lambda: dev.gcode_order_pens(ends, grp4, 4, True), "k_op_chain", a.reps)
        res["four_groups_rev"]["reversed"] = int(r.sum())
        for name in ("one_group", "one_group_rev", "four_groups_rev"):
            res[name]["chain_over_parent"] = res[name]["chain_s_median"] / res["parent"]["chain_s_median"]
        if a.check_size:
            m = min(n, a.check_size)
            got = dev.gcode_order_pens(ends[:m], grp4[:m], 4, True)
            want = PD.order_pens_numpy(ends[:m], grp4[:m], 4, True)
            res["equals_numpy_definition"] = {"paths": m, "equal": bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))}
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
