"""Stage 04's memo planes and walk logs are kept from step to step and never cleared as a whole; the launch of a layer's trace zeroes the eight memo
words of that layer's skeleton pixels only (walker.h: WalkArgs::memo).  Here the product's serial walker runs on the CPU (tests/host/memo_reuse_harness.cpp,
a stand-alone program built with g++) over every pair of consecutive maps a memo plane sees in the sequence of tests/memo_reuse_cases.py -- the sequence
tests/test_gpu_memo_reuse.py runs on the device -- with ONE memo and ONE log across the pair:
  * with the second map's words cleared, the second run equals the oracle on every pair;
  * with nothing cleared it does not, on at least one pair: the sequence bites (CPU only: on the device a stale word would index the log of an
    earlier step);
  * once more under AddressSanitizer and UBSan, with the clear."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from util import same_polys
from memo_reuse_cases import sequence

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "memo_reuse_harness.cpp")

_cases = {}


def cases():
    """(skeleton maps, pairs, oracle contours of each pair's second map).  Memo plane l sees layer l of every step that has one: its consecutive maps
    are the pairs.  Skeletons and contours are the oracle's, computed once and left unchanged."""
    if not _cases:
        sk_of, maps, want_of, pairs = {}, [], [], []
        seq = sequence()
        for l in range(max(st.shape[0] for _, st in seq)):
            prev = None
            for tag, st in seq:
                if l >= st.shape[0]:
                    continue
                key = (tag, l)
                if key not in sk_of:
                    sk = O.thin_rot(st[l])
                    sk_of[key] = len(maps); maps.append(sk); want_of.append([p for p in O.trace(sk) if len(p) >= 5])
                if prev is not None:
                    pairs.append((sk_of[prev], sk_of[key]))
                prev = key
        _cases.update(maps=maps, pairs=pairs, want=[want_of[b] for _, b in pairs])
    return _cases["maps"], _cases["pairs"], _cases["want"]


def build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-sign-compare", *flags, "-o", exe, SRC])
    return exe


def run(tmp_path, exe, mode):
    """[(rc, contours of the second run)] per pair"""
    maps, pairs, _ = cases()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / f"out_{mode}.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(maps)))
        for m in maps:
            f.write(struct.pack("<ii", *m.shape)); f.write(np.ascontiguousarray(m, np.uint8).tobytes())
        f.write(struct.pack("<i", len(pairs)))
        f.write(np.asarray(pairs, np.int32).tobytes())
    r = subprocess.run([exe, fin, fout, mode], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stdout, r.stderr)
    buf = open(fout, "rb").read(); pos = 0; out = []
    for _ in pairs:
        rc, n, t = struct.unpack_from("<iqq", buf, pos); pos += 20
        off = np.frombuffer(buf, np.int64, n + 1, pos); pos += 8 * (n + 1)
        pts = np.frombuffer(buf, np.int32, 2 * t, pos).reshape(-1, 2); pos += 8 * t
        out.append((rc, [pts[off[i]:off[i + 1]].reshape(-1, 1, 2) for i in range(n)]))
    assert pos == len(buf)
    return out


def test_the_pairs_are_the_sequence():
    maps, pairs, want = cases()
    seq = sequence()
    assert [t for t, _ in seq] == ["A", "A_shift", "A_T", "A", "A_k2", "A", "B", "A"]
    assert len(pairs) == 2 * (len(seq) - 1) + 2 * (len(seq) - 2)           # planes 0, 1 see every step, planes 2, 3 all but the K = 2 one
    assert all(len(w) >= 1 for w in want) and all(m.any() for m in maps)
    assert any(maps[a].shape != maps[b].shape for a, b in pairs)           # H and W swapped: the old words land at other pixels
    A, S = seq[0][1], seq[1][1]
    near = [(O.thin_rot(A[l]) > 0, O.thin_rot(S[l]) > 0) for l in range(A.shape[0])]
    assert all((a & s).any() and (s & ~a).any() for a, s in near)          # the shifted skeleton lies partly on the old one and partly beside it


def test_second_run_equals_oracle_when_its_words_are_cleared(tmp_path):
    _, pairs, want = cases()
    got = run(tmp_path, build(tmp_path, "memo_reuse", ["-O2"]), "clear")
    for (a, b), (rc, polys), w in zip(pairs, got, want):
        assert rc == 0 and same_polys(polys, w), (a, b, rc, len(polys), len(w))


def test_without_the_clear_the_sequence_bites(tmp_path):
    _, pairs, want = cases()
    got = run(tmp_path, build(tmp_path, "memo_reuse", ["-O2"]), "noclear")
    bad = [(a, b) for (a, b), (rc, polys), w in zip(pairs, got, want) if rc != 0 or not same_polys(polys, w)]
    print(f"{len(bad)} of {len(pairs)} pairs differ from the oracle with nothing cleared: {bad}")
    assert bad


def test_second_run_under_sanitizers(tmp_path):
    _, pairs, want = cases()
    exe = build(tmp_path, "memo_reuse_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    got = run(tmp_path, exe, "clear")
    for (a, b), (rc, polys), w in zip(pairs, got, want):
        assert rc == 0 and same_polys(polys, w), (a, b, rc)
