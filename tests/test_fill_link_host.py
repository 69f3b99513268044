"""fill connect on the host, no GPU: the sequential double of tests/fill_link_double.py against what the rule implies (include/orip.h: orip_fill_link), the
counts the pass was proposed with, the named cases against what they are named for, the numpy form against the sequential one, orip.stages.fill_options
with the two new keys, and the stage script with the doubles injected for the device.  Every comparison is equality."""
import json
import pickle
import sys

import numpy as np
import pytest

import fill_cases as FC
import fill_double as FD
import fill_link_cases as LC
import fill_link_double as LD
import pens_double as PD
from fill_cases import STAGES, make_output, snapshot

CASES = LC.cases()
WANT = {}


def want(name):
    """(off, pts, stats, detail) of the sequential double, computed once"""
    if name not in WANT:
        d = {}
        WANT[name] = LD.fill_link(*LC.args(CASES[name]), detail=d) + (d,)
    return WANT[name]


# ------------------------------------------------------------------ the consequences of the rule
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_consequences_on_the_double(name):
    c = CASES[name]
    off, pts, st, d = want(name)
    seg, fk = d["seg"], d["fk"]
    assert np.array_equal(seg, FD.fill_mask(*FC.args(c))[0])                          # the families one by one are the fill's list
    assert st["segments"] == len(seg) and st["paths_out"] == st["segments"] - st["links"] == len(off) - 1 and st["points_out"] == 2 * st["segments"] == len(pts)
    assert st["links"] <= st["eligible"] <= st["in_reach"] and off[0] == 0 and off[-1] == len(pts) and pts.dtype == np.int32 and off.dtype == np.int64
    assert sorted(j for m in d["members"] for j in m) == list(range(len(seg)))          # every segment once
    assert [m[0] for m in d["members"]] == sorted(m[0] for m in d["members"])           # strokes in ascending order of their first member
    links = set(d["links"])
    steps = 0
    for i, m in enumerate(d["members"]):
        p = pts[off[i]:off[i + 1]].tolist()
        assert len(p) == 2 * len(m)
        for r, j in enumerate(m):                                                     # every output segment is an input segment, as it was, or a link, in order
            assert p[2 * r] + p[2 * r + 1] == seg[j].tolist()
            if r:
                a = m[r - 1]
                assert (a, j) in links and a < j and fk[a][0] == fk[j][0] and fk[j][1] == fk[a][1] + 1      # one family, consecutive k
                E, S = tuple(seg[a][2:4].tolist()), tuple(seg[j][0:2].tolist())
                dx, dy = S[0] - E[0], S[1] - E[1]
                assert max(abs(dx), abs(dy)) <= c["reach"] and dx * dx + dy * dy <= c["reach"] ** 2
                px = LD.link_pixels(E, S)
                assert px[0] == E and px[-1] == S and all(FD.ink(c["mask"], c["place"], X, Y) for X, Y in px)      # every link's pixels are ink
                steps += max(abs(dx), abs(dy))
    assert steps == st["link_steps"] and sum(len(m) - 1 for m in d["members"]) == st["links"]


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_with_a_reach_too_small_for_any_pair_the_list_comes_back(name):
    c = FC.cases()[name]
    seg = FD.fill_mask(*FC.args(c))[0]
    off, pts, st = LD.fill_link(*FC.args(c), 1)
    assert st["in_reach"] == st["links"] == 0 and np.array_equal(off, 2 * np.arange(len(seg) + 1)) and np.array_equal(pts.reshape(-1, 4), seg)


def test_the_counts_the_pass_was_proposed_with():
    for d, n in ((0, 17), (1, 25), (2, 34), (4, 48)):
        for mult in (2, 3):
            st = want(f"full_u{d}@{mult}")[2]
            assert (st["segments"], st["paths_out"]) == (n, 1)
    for d, n in ((0, 19), (1, 24), (2, 29), (3, 26)):
        assert (want(f"rect_hole_p0_u{d}@2")[2]["segments"], want(f"rect_hole_p0_u{d}@2")[2]["paths_out"]) == (n, 2)
    assert (want("family_cross_serpentine@2")[2]["segments"], want("family_cross_serpentine@2")[2]["paths_out"]) == (55, 5)
    assert (want("off_canvas_y@2")[2]["segments"], want("off_canvas_y@2")[2]["paths_out"]) == (92, 5)
    assert (want("random_60@2")[2]["segments"], want("random_60@2")[2]["paths_out"]) == (750, 460)
    for name in ("family_along@2", "family_across@2", "family_cross@2", "negative_k_plain@2"):      # without serpentine almost nothing links
        assert want(name)[2]["links"] <= 2 and want(name)[2]["segments"] > 20


def test_the_pass_is_not_idempotent_and_nothing_is_reversed():
    off, pts, st, d = want("rect_hole_p0_u3@2")
    assert st["links"] > 0 and len(off) - 1 < len(d["seg"])                            # its output is no list of 2-point segments: it cannot be its own input
    assert np.array_equal(np.sort(pts.reshape(-1, 4), 0), np.sort(d["seg"], 0))        # each segment START -> END as it came


# ------------------------------------------------------------------ the named cases
def link_of(d, a):
    return dict(d["links"]).get(a)


def test_the_cases_exercise_what_they_are_named_for():
    off, pts, st, d = want("long_link")
    assert st == dict(segments=5, in_reach=4, eligible=4, links=4, paths_out=1, points_out=10, link_steps=280)
    assert all(len(LD.link_pixels(tuple(d["seg"][a][2:4].tolist()), tuple(d["seg"][b][0:2].tolist()))) == 71 for a, b in d["links"])      # a second block of 64
    off, pts, st, d = want("hole_in_second_block")
    px = LD.link_pixels((39, 0), (39, 70))
    c = CASES["hole_in_second_block"]
    assert d["seg"][0].tolist() == [0, 0, 39, 0] and d["seg"][1].tolist() == [39, 70, 0, 70]
    assert [t for t, p in enumerate(px) if not FD.ink(c["mask"], c["place"], *p)] == [65, 66, 67, 68, 69]      # none of the first 64
    assert d["links"] == [(1, 2), (2, 3), (3, 4)] and st["in_reach"] == 4 and st["eligible"] == 3      # that link is refused and the others hold
    off, pts, st, d = want("slit")
    assert [s.tolist() for s in d["seg"]] == [[3, 0, 26, 0], [26, 4, 3, 4], [3, 8, 26, 8], [26, 12, 3, 12]]
    c = CASES["slit"]
    assert FD.ink(c["mask"], c["place"], 3, 4) and FD.ink(c["mask"], c["place"], 3, 8) and not FD.ink(c["mask"], c["place"], 3, 6)      # both ends ink, the row between empty
    assert d["links"] == [(0, 1), (2, 3)] and st["in_reach"] == 3 and st["eligible"] == 2
    off, pts, st, d = want("comb")
    assert [s.tolist() for s in d["seg"]] == [[0, 0, 20, 0], [2, 4, 5, 4], [9, 4, 12, 4], [17, 4, 19, 4], [23, 4, 26, 4]]
    c = CASES["comb"]
    for S in ((17, 4), (23, 4)):                                                      # an exact tie in d^2, both over ink: the lower index wins
        assert (S[0] - 20) ** 2 + 16 == 25 and all(FD.ink(c["mask"], c["place"], *p) for p in LD.link_pixels((20, 0), S))
    assert st["in_reach"] == 3 and st["eligible"] == 3 and d["links"] == [(0, 3)] and st["paths_out"] == 4
    off, pts, st, d = want("family_boundary")
    fam = [f for f, k in d["fk"]]
    last_along = [j for j in range(len(fam)) if d["fk"][j] == max(x for x in d["fk"] if x[0] == 0)]
    first_across = [j for j in range(len(fam)) if d["fk"][j] == min(x for x in d["fk"] if x[0] == 1)]
    near = [(a, b) for a in last_along for b in first_across if ((d["seg"][b][0:2] - d["seg"][a][2:4]).astype(np.int64) ** 2).sum() <= 45 ** 2]
    assert near and all(fam[a] == fam[b] for a, b in d["links"]) and st["paths_out"] == 2 and link_of(d, last_along[-1]) is None
    off, pts, st, d = want("chain_150")
    assert st["segments"] == 150 and st["paths_out"] == 1 and len(d["members"][0]) == 150 > 2 ** 7
    off, pts, st, d = want("negative_k_serpentine")
    ks = [k for f, k in d["fk"]]
    assert min(ks) < 0 < max(ks) and any(k & 1 for k in ks if k < 0) and st["paths_out"] == 1
    back = [j for j, k in enumerate(ks) if k & 1]                                     # the parity of a negative k in two's complement: -1, -3 are drawn backwards
    fw = FD.fill_mask(*FC.args(dict(CASES["negative_k_serpentine"], flags=FC.ALONG)))[0]
    assert all(d["seg"][j].tolist() == fw[j][[2, 3, 0, 1]].tolist() for j in back) and any(ks[j] < 0 for j in back)
    off, pts, st, d = want("plain_far")
    assert st["links"] == 3 and st["paths_out"] == 1 and st["link_steps"] == 3 * 199 and all(d["seg"][b][0] == 0 and d["seg"][a][2] == 199 for a, b in d["links"])
    for name in ("empty@2", "all_short@3", "tiny_canvas@2"):
        assert want(name)[2] == dict.fromkeys(LD.STATS, 0) and want(name)[0].tolist() == [0] and want(name)[1].shape == (0, 2)
    assert want("reach_1")[2]["links"] == 0 and want("reach_1")[2]["segments"] == 19


# ------------------------------------------------------------------ the numpy form
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_numpy_form_equals_the_sequential_one(name):
    off, pts, st = LD.fill_link_numpy(*LC.args(CASES[name]))
    assert st == want(name)[2] and off.dtype == np.int64 and pts.dtype == np.int32 and np.array_equal(off, want(name)[0]) and np.array_equal(pts, want(name)[1])


def test_the_cap_case_exceeds_the_cap():
    off, pts, st = LD.fill_link_numpy(*LC.args(LC.cap_pairs()))
    assert st["in_reach"] > LC.ELIG_WAVES_CAP and 0 < st["eligible"] < st["in_reach"] and st["links"] == st["eligible"] and st["paths_out"] == 150


# ------------------------------------------------------------------ the config
def cfg_with(fill, **kw):
    from orip.config import Config
    cfg = Config()
    for k, v in kw.items():
        setattr(cfg, k, v)
    cfg._raw = {} if fill is None else {"fill": fill}
    return cfg


def test_fill_options_with_and_without_connect():
    from orip import lib, stages as S
    plain = S.fill_options(cfg_with({"layers": {"layer_dark": {"spacing_mm": 0.6, "direction": "cross"}, "layer_mid": {}}}))
    assert plain["layer_dark"] == dict(spacing=24, inset=12, min_len=20, u=(2896, 2896), flags=lib.FILL_ALONG | lib.FILL_ACROSS | lib.FILL_SERPENTINE, order="serpentine",
                                       angle_deg=45.0)                               # the dict it was: no key is added without connect
    off = S.fill_options(cfg_with({"connect": False, "connect_mm": "never read", "layers": {"layer_dark": {"spacing_mm": 0.6, "direction": "cross"}, "layer_mid": {"connect_mm": -3}}}))
    assert off == plain
    on = S.fill_options(cfg_with({"connect": True, "layers": {"layer_dark": {"spacing_mm": 0.6, "direction": "cross"}, "layer_mid": {"connect_mm": 1.25}, "layer_light": {"connect": False}}}))
    assert on["layer_dark"] == dict(plain["layer_dark"], reach=48) and on["layer_mid"] == dict(plain["layer_mid"], reach=50)      # twice the layer's spacing; its own length
    assert "reach" not in on["layer_light"] and list(on) == ["layer_dark", "layer_mid", "layer_light"]
    per = S.fill_options(cfg_with({"layers": {"layer_mid": {"connect": True}}}, pixels_per_mm=10))
    assert per["layer_mid"]["reach"] == 20 and lib.FILL_LINK_REACH_MAX == 1 << 15 and len(lib.FILL_LINK_STATS) == 7


@pytest.mark.parametrize("fill, word", [
    ({"connect": 1, "layers": {"layer_dark": {}}}, "connect"), ({"layers": {"layer_dark": {"connect": "yes"}}}, "connect"),
    ({"connect": True, "connect_mm": 0, "layers": {"layer_dark": {}}}, "connect_mm"), ({"connect": True, "connect_mm": 900, "layers": {"layer_dark": {}}}, "connect_mm"),
    ({"connect": True, "layers": {"layer_dark": {"connect_mm": "2"}}}, "connect_mm"), ({"connect": True, "layers": {"layer_dark": {"connect_mm": float("nan")}}}, "connect_mm"),
    ({"connect": True, "layers": {"layer_dark": {"connect_mm": True}}}, "connect_mm"), ({"connected": True, "layers": {"layer_dark": {}}}, "connected"),
    ({"layers": {"layer_dark": {"connect_px": 3}}}, "connect_px")])
def test_fill_options_refuses_and_names_the_key(fill, word):
    from orip import stages as S
    with pytest.raises(ValueError, match=word):
        S.fill_options(cfg_with(fill))


# ------------------------------------------------------------------ the stage script
def stage_module():
    if STAGES not in sys.path:
        sys.path.insert(0, STAGES)
    import fill_layers
    return fill_layers


CONNECT = {"spacing_mm": 1.0, "angle_deg": 30, "connect": True, "layers": {"layer_dark": {"direction": "cross"}, "layer_light": {"order": "nearest", "spacing_mm": 0.7, "connect_mm": 2.0}}}


def test_the_stage_script_writes_the_chains_as_polylines(tmp_path, capsys):
    from orip import stages as S
    from orip.config import load_config
    from orip.stream import to_steps
    FL = stage_module()
    out, masks = make_output(tmp_path, CONNECT)
    before = snapshot(out)
    cfg = load_config(str(out / "config.json"))
    D = LD.Doubles()
    assert FL.run(cfg, fill_fn=D.fill, order_fn=PD.order_pens_numpy, link_fn=D.link) == 0 and D.fills == D.links == 2
    printed = capsys.readouterr().out.splitlines()
    report = [l for l in printed if l.startswith("[fill] layer_")]
    linked = [l for l in printed if l.startswith("[fill-link] layer_")]
    assert [printed.index(l) for l in linked] == [printed.index(l) + 1 for l in report]      # the second line, behind the first
    after = snapshot(out)
    assert sorted(set(after) - set(before)) == ["layer_dark/ops_filled.pkl", "layer_light/ops_filled.pkl"]
    assert all(after[k] == before[k] for k in before if k != "vector_manifest.json")
    man = json.loads(after["vector_manifest.json"])
    opts = S.fill_options(cfg)
    assert opts["layer_dark"]["reach"] == 20 and opts["layer_light"]["reach"] == 20
    for i, name in enumerate(cfg.color_names):
        o = opts[name]
        ops, filled = pickle.loads(before[f"{name}/ops.pkl"]), pickle.loads(after[f"{name}/ops_filled.pkl"])
        fargs = (masks[i], 200, 150, (200, 40, 0, 0), o["u"], o["spacing"], o["inset"], o["min_len"], o["flags"])
        fst = FD.fill_mask(*fargs)[1]
        off, pts, st = LD.fill_link(*fargs, o["reach"])
        strokes = [pts[off[k]:off[k + 1]] for k in range(len(off) - 1)]
        assert st["links"] > 3 and st["paths_out"] < st["segments"]
        if o["order"] == "nearest":                                                   # each stroke's first and last point, from the end of the outline: its tap
            ends = np.concatenate([to_steps(pts[off[:-1]], 200, 150), to_steps(pts[off[1:] - 1], 200, 150)], 1)
            order, rev = PD.order_pens_numpy(ends, np.zeros(len(strokes), np.int32), 1, reverse=True, start=tuple(to_steps(np.array([[150, 20 + i]]), 200, 150)[0]))
            strokes = [strokes[k][::-1] if r else strokes[k] for k, r in zip(order, rev)]
        tail = filled[len(ops):]
        assert man["layers"][i]["file"] == f"{name}/ops_filled.pkl" and man["layers"][i]["count_ops"] == len(filled) == len(ops) + st["paths_out"]
        assert all(t["type"] == "line" and t["points"].dtype == np.float32 and np.array_equal(t["points"], s.astype(np.float32)) for t, s in zip(tail, strokes))
        assert f"angle={o['angle_deg']:.3f}" in report[i] and all(f"{k}={fst[k]}" in report[i] for k in FD.STATS)
        assert linked[i] == f"[fill-link] {name}: reach=20 " + " ".join(f"{k}={st[k]}" for k in LD.STATS)
    D2 = LD.Doubles()
    assert FL.run(load_config(str(out / "config.json")), fill_fn=D2.fill, order_fn=PD.order_pens_numpy, link_fn=D2.link) == 0      # a second run: identical files
    assert snapshot(out) == after


def test_without_connect_no_link_call_is_made_and_nothing_changes(tmp_path, capsys):
    from orip.config import load_config
    FL = stage_module()
    plain = {k: v for k, v in CONNECT.items() if k != "connect"}                       # connect_mm alone switches nothing on
    a, _ = make_output(tmp_path / "a", FC.FILL)
    b, _ = make_output(tmp_path / "b", dict(plain, connect=False))
    c, _ = make_output(tmp_path / "c", {k: v for k, v in plain.items() if k != "layers"} | {"layers": {"layer_dark": {"direction": "cross"}, "layer_light": {"order": "nearest", "spacing_mm": 0.7}}})

    def never(*a, **k):
        raise AssertionError("no link call without connect")
    lines = []
    for out in (a, b, c):
        assert FL.run(load_config(str(out / "config.json")), fill_fn=FD.fill_mask, order_fn=PD.order_pens_numpy, link_fn=never) == 0
        lines.append([l.replace(str(out), "") for l in capsys.readouterr().out.splitlines()])
    assert lines[0] == lines[1] == lines[2] and not any("fill-link" in l for l in lines[0])
    sa, sb, sc = (snapshot(o) for o in (a, b, c))
    same = lambda x, y: all(x[k] == y[k] for k in x if k != "config.json") and set(x) == set(y)
    assert same(sa, sb) and same(sa, sc)


def test_one_layer_connected_and_one_not(tmp_path, capsys):
    from orip.config import load_config
    FL = stage_module()
    out, masks = make_output(tmp_path, {"angle_deg": 30, "layers": {"layer_dark": {}, "layer_light": {"connect": True, "spacing_mm": 0.7}}})
    D = LD.Doubles()
    assert FL.run(load_config(str(out / "config.json")), fill_fn=D.fill, order_fn=PD.order_pens_numpy, link_fn=D.link) == 0 and (D.fills, D.links) == (2, 1)
    printed = capsys.readouterr().out
    assert "[fill-link] layer_light: reach=14 " in printed and "[fill-link] layer_dark" not in printed
    dark = pickle.loads((out / "layer_dark" / "ops_filled.pkl").read_bytes())[2:]
    light = pickle.loads((out / "layer_light" / "ops_filled.pkl").read_bytes())[2:]
    assert all(o["points"].shape == (2, 2) for o in dark) and any(len(o["points"]) > 2 for o in light) and all(len(o["points"]) % 2 == 0 for o in light)
