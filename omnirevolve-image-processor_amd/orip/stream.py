"""Plotter byte stream from the ordered ops of every layer -- the step after the path (13_build_stream.py + the wire protocol of
shared/omnirevolve_plotter_stream_creator_helper.py).

Wire format (helper :7-15): step bytes 11 FFF SSS (two steps) / 10 SSS 000 (one); service bytes 0x40|div (speed), 0x01 pen up,
0x02 pen down, 0x03 tap, 0x08..0x0F colour, 0x3F end of stream; padded with zeros to a multiple of 1024 bytes (:170-175).

The reference emits the stream one segment at a time through a byte-appending writer.  Here a plot is compiled in three passes, the same for
stage 13 and for gcode2stream / svg2stream (orip/gcode.py, orip/svg.py):
  1. every MOVE of the plot (pen-up travel, polyline segment) and every service byte is laid out in order, in plotter step space, as flat numpy
     arrays over all ops (plan_ops: no Python call per segment);
  2. the direction codes of all moves come from ONE launch of the HIP kernel behind orip_stream_codes (closed-form Bresenham, one thread
     per step) and stay on the device;
  3. the speed plan cuts every move into pieces (divider, step range) exactly as the helper's ramps do (plan_pieces), layout() gives every piece
     its byte position (prefix sums of the byte counts), and orip_stream_pack writes the bytes on the device (steps are paired per piece, as
     StreamWriter.add_steps pairs them); only the finished stream comes back.
Everything that decides a byte follows the reference line by line in meaning: rounding (Python round = half-to-even), clamping, the
Y flip, the "approach before colour select" rule, corner thresholds, ramp tables, the per-piece step pairing, the pen / tap sequence."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

SPI_CHUNK_SIZE = 1024                      # helper :22
PEN_UP, PEN_DOWN, TAP, EOF_BYTE = 0x01, 0x02, 0x03, 0x3F


@dataclass
class StreamConfig:                        # helper Config (:100-128): same fields, same defaults
    steps_per_mm: float = 40.0
    invert_y: bool = True
    div_start: int = 28
    div_fast: int = 15
    profile: str = "triangle"
    corner_deg: float = 85.0
    corner_div: int = 28
    corner_window_steps: int = 300
    short_len_steps: int = 120
    short_div: int = 16
    travel_div_fast: int = 10
    travel_start_div: int = 28
    travel_window_steps: int = 240
    travel_quant_step: int = 4
    soft_tail_steps: int = 0
    soft_tail_div: int = 20


def stream_config_from_pipeline(cfg) -> StreamConfig:
    """13:55-68.  The draw_* / corner_* / travel_* keys are not Config fields, so load_config drops them and the getattr defaults rule."""
    return StreamConfig(steps_per_mm=float(getattr(cfg, "pixels_per_mm", 40.0)), invert_y=True,
                        div_start=int(getattr(cfg, "draw_div_start", 25)), div_fast=int(getattr(cfg, "draw_div_fast", 15)),
                        profile=str(getattr(cfg, "draw_profile", "triangle")), corner_deg=float(getattr(cfg, "corner_deg", 85.0)),
                        corner_div=int(getattr(cfg, "corner_div", 30)), corner_window_steps=int(getattr(cfg, "corner_window_steps", 800)),
                        travel_div_fast=int(getattr(cfg, "travel_div_fast", 10)))


# ------------------------------------------------------------------ speed plans: a move of N steps -> [(divider, count), ...]
def _even_parts(total: int, levels: int) -> List[int]:               # helper :70-74
    base, rem = divmod(total, levels)
    return [base + (1 if i < rem else 0) for i in range(levels)]


def _ramp_counts(profile: str, length: int, div_fast: int, div_slow: int) -> Dict[int, int]:     # helper :76-98, :211-216
    if length <= 0:
        return {}
    if div_slow < div_fast:
        raise ValueError("div_slow must be >= div_fast")
    out: Dict[int, int] = {}
    if profile == "triangle":
        for i, cnt in enumerate(_even_parts(length, div_slow - div_fast + 1)):
            if cnt > 0:
                out[div_slow - i] = out.get(div_slow - i, 0) + cnt
    elif profile == "scurve":
        span = div_slow - div_fast
        for i in range(length):
            t = (i + 0.5) / length
            div = max(div_fast, min(div_slow, round(div_slow - ((3 * t * t) - (2 * t * t * t)) * span)))
            out[div] = out.get(div, 0) + 1
    else:
        raise ValueError("profile must be 'triangle' or 'scurve'")
    return out


def _accel(n: int, profile: str, div_fast: int, start_div: int) -> List[Tuple[int, int]]:        # emit_steps_accel, helper :218-227
    if n <= 0:
        return []
    if start_div <= div_fast:
        return [(div_fast, n)]
    counts = _ramp_counts(profile, n, div_fast, start_div)
    return [(d, counts[d]) for d in range(start_div, div_fast - 1, -1) if counts.get(d, 0) > 0]


def _decel(n: int, profile: str, div_fast: int, end_div: int) -> List[Tuple[int, int]]:          # emit_steps_decel, helper :229-238
    if n <= 0:
        return []
    if end_div <= div_fast:
        return [(div_fast, n)]
    counts = _ramp_counts(profile, n, div_fast, end_div)
    return [(d, counts[d]) for d in range(div_fast, end_div + 1) if counts.get(d, 0) > 0]


def plan_segment(n: int, sc: StreamConfig, slow_in: bool, slow_out: bool) -> List[Tuple[int, int]]:
    """emit_segment_with_corner_profile (helper :251-292) as a list of (divider, count) pieces covering the n steps in order."""
    if n == 0:
        return []
    if not slow_in and not slow_out:
        return [(sc.short_div if n <= sc.short_len_steps else sc.div_fast, n)]
    entry = min(sc.corner_window_steps if slow_in else 0, n)
    exit_ = min(sc.corner_window_steps if slow_out else 0, max(0, n - entry))
    mid = max(0, n - entry - exit_)
    if entry + exit_ >= n:
        half = n // 2
        out = _accel(half, sc.profile, sc.div_fast, sc.corner_div if slow_in else sc.div_start) if half > 0 else []
        if n % 2 == 1:
            out.append((sc.div_fast, 1)); half += 1
        return out + _decel(n - half, sc.profile, sc.div_fast, sc.corner_div if slow_out else sc.div_start)
    out = _accel(entry, sc.profile, sc.div_fast, sc.corner_div)
    if mid > 0:
        out.append((sc.div_fast, mid))
    return out + _decel(exit_, sc.profile, sc.div_fast, sc.corner_div)


def _quantized_levels(div_slow: int, div_fast: int, step: int) -> List[int]:                      # helper :100-107 (:88-95 in the file)
    if div_slow < div_fast:
        div_slow, div_fast = div_fast, div_slow
    levels = list(range(div_slow, div_fast - 1, -step))
    if levels[-1] != div_fast:
        levels.append(div_fast)
    return levels


def plan_travel(n: int, sc: StreamConfig) -> List[Tuple[int, int]]:
    """travel_ramped (helper :340-380)."""
    if n == 0:
        return []
    win, div_fast, div_start = int(sc.travel_window_steps), int(sc.travel_div_fast), int(sc.travel_start_div)
    if div_start < div_fast:
        div_start = div_fast
    if n <= 2 * win:
        half = max(1, n // 2)
        out = _accel(half, sc.profile, div_fast, div_start)
        if n % 2 == 1:
            out.append((div_fast, 1 if half < n else 0)); half += 1     # n == 1: the helper still sets the speed, for a slice without steps
        return out + _decel(max(0, n - half), sc.profile, div_fast, div_start)
    down = _quantized_levels(div_start, div_fast, max(1, int(sc.travel_quant_step)))
    out = [(d, c) for d, c in zip(down, _even_parts(win, len(down))) if c > 0]
    if n - 2 * win > 0:
        out.append((div_fast, n - 2 * win))
    return out + [(d, c) for d, c in zip(reversed(down), _even_parts(win, len(down))) if c > 0]


# ------------------------------------------------------------------ geometry in step space
def to_steps(xy: np.ndarray, W: int, H: int) -> np.ndarray:
    """_to_steps (13:84-88) on an array of (x, y): round half-to-even, clamp to the sheet, Y flip."""
    p = np.rint(np.asarray(xy, np.float64).reshape(-1, 2))
    x = np.clip(p[:, 0], 0, W - 1).astype(np.int64)
    y = (H - 1) - np.clip(p[:, 1], 0, H - 1).astype(np.int64)
    return np.stack([x, y], 1)


def _angle(a, b, c) -> float:                                          # angle_degrees, helper :242-249 (Python floats, libm)
    v1x, v1y, v2x, v2y = a[0] - b[0], a[1] - b[1], c[0] - b[0], c[1] - b[1]
    n1, n2 = math.hypot(v1x, v1y), math.hypot(v2x, v2y)
    if n1 == 0 or n2 == 0:
        return 180.0
    return math.degrees(math.acos(max(-1.0, min(1.0, (v1x * v2x + v1y * v2y) / (n1 * n2)))))


# ------------------------------------------------------------------ colour remap (13:92-160)
def _color_idx(x) -> int:
    try:
        return int(x) & 7
    except Exception:
        return 0


def load_color_maps(cfg):
    force = getattr(cfg, "stream_force_color_index", None)
    if force is not None:
        force = _color_idx(force)
    by_name = getattr(cfg, "stream_color_by_name", None)
    by_name = {str(k): _color_idx(v) for k, v in by_name.items()} if isinstance(by_name, dict) else None
    by_order = getattr(cfg, "stream_color_by_order", None)
    by_order = [_color_idx(v) for v in by_order] if isinstance(by_order, (list, tuple)) and len(by_order) > 0 else None
    env_force = os.environ.get("STREAM_FORCE_COLOR_INDEX")
    if env_force is not None:
        force = _color_idx(env_force)
    env_order = os.environ.get("STREAM_COLOR_ORDER")
    if env_order:
        by_order = [_color_idx(v) for v in env_order.split(",")]
    return force, by_name, by_order


def resolve_color_index(name: str, orig: int, ordinal: int, force, by_name, by_order) -> int:
    if force is not None:
        return force
    if by_name and name in by_name:
        return by_name[name]
    if by_order:
        return by_order[ordinal % len(by_order)]
    return _color_idx(orig)


def corner_flags_flat(pts: np.ndarray, off: np.ndarray, corner_deg: float) -> Tuple[np.ndarray, np.ndarray]:
    """slow_in / slow_out of every segment of the polylines of a flat list (emit_polyline, helper :300-312): pts int [total, 2], off [n + 1] (a polyline
    of one point has no segment and is no corner of its neighbours) -> flags per SEGMENT in list order (polyline p owns segments off[p] - p ..
    off[p + 1] - p - 2).  The interior angle at every vertex is computed vectorised; a vertex whose angle comes out within 1e-6 degrees of the
    threshold is decided again with the helper's scalar formula (math.hypot / acos / degrees), so the comparison is the reference's own arithmetic
    wherever it could matter."""
    pts = np.asarray(pts).reshape(-1, 2); off = np.asarray(off, np.int64)
    total = len(pts)
    sharp = np.zeros(total, bool)
    if total >= 3:
        p = pts.astype(np.float64)
        v1, v2 = p[:-2] - p[1:-1], p[2:] - p[1:-1]
        n1, n2 = np.hypot(v1[:, 0], v1[:, 1]), np.hypot(v2[:, 0], v2[:, 1])
        ok = (n1 > 0) & (n2 > 0)
        cosv = np.clip((v1[:, 0] * v2[:, 0] + v1[:, 1] * v2[:, 1]) / np.where(ok, n1 * n2, 1.0), -1.0, 1.0)
        ang = np.where(ok, np.degrees(np.arccos(cosv)), 180.0)
        sharp[1:-1] = ang < corner_deg
        for j in np.nonzero(np.abs(ang - corner_deg) < 1e-6)[0]:
            sharp[j + 1] = _angle(pts[j], pts[j + 1], pts[j + 2]) < corner_deg
    sharp[off[:-1]] = False; sharp[off[1:] - 1] = False                   # a polyline's end points are no corners (and their angles span two polylines)
    is_last = np.zeros(total, bool); is_last[off[1:] - 1] = True
    a = np.nonzero(~is_last)[0]                                           # first vertex of every segment
    return sharp[a], sharp[a + 1]


# ------------------------------------------------------------------ the plan of a plot, flat over all ops
@dataclass
class Plan:
    """The moves of a plot and what the byte layout needs once their step counts are known."""
    moves: np.ndarray           # int32 [M, 4]
    kind: np.ndarray            # per item: service byte, or -1 for the next move
    is_travel: np.ndarray       # per move
    slow_in: np.ndarray
    slow_out: np.ndarray


def fixed_plan(kind, travels=()) -> Plan:
    """service bytes and pen-up travels (x0, y0, x1, y1) in a given order: kind per item, -1 for the next travel"""
    t = np.asarray(travels, np.int32).reshape(-1, 4)
    return Plan(t, np.asarray(kind, np.int64), np.ones(len(t), bool), np.zeros(len(t), bool), np.zeros(len(t), bool))


def concat_plans(plans: Sequence[Plan]) -> Plan:
    return Plan(*(np.concatenate([getattr(p, f) for p in plans]) for f in ("moves", "kind", "is_travel", "slow_in", "slow_out")))


def plan_ops(off: np.ndarray, pts: np.ndarray, is_tap: np.ndarray, cur, head: Sequence[int], lift: bool, sc: StreamConfig) -> Plan:
    """The ops of a plot in step space (op i is pts[off[i]:off[i + 1]]; a tap is one point, a line two or more), drawn in order from the cursor `cur`
    with the pen up: the service bytes `head`; then per op a travel when the cursor is elsewhere (after a pen-up byte of its own when `lift`), and
    the tap byte, or pen down, the segments, pen up.  The cursor stays on a tap and goes to a line's last point."""
    off = np.asarray(off, np.int64); pts = np.asarray(pts, np.int64).reshape(-1, 2); is_tap = np.asarray(is_tap, bool)
    n = len(off) - 1
    nseg = np.diff(off) - 1
    first, last = pts[off[:-1]], pts[off[1:] - 1]
    before = np.concatenate([np.asarray(cur, np.int64).reshape(1, 2), last[:-1]])[:n]      # the cursor in front of every op
    trav = (before != first).any(1)
    per_op = trav + nseg                                                  # moves of an op
    mbase = np.cumsum(per_op) - per_op
    M = int(per_op.sum())
    moves = np.zeros((M, 4), np.int32)
    is_travel = np.zeros(M, bool); slow_in = np.zeros(M, bool); slow_out = np.zeros(M, bool)
    t = mbase[trav]
    moves[t, :2] = before[trav]; moves[t, 2:] = first[trav]; is_travel[t] = True
    is_last = np.zeros(len(pts), bool); is_last[off[1:] - 1] = True
    a = np.nonzero(~is_last)[0]                                           # first vertex of every segment
    sp = np.repeat(np.arange(n), nseg)
    s = mbase[sp] + trav[sp] + (a - off[sp])
    moves[s, :2] = pts[a]; moves[s, 2:] = pts[a + 1]
    slow_in[s], slow_out[s] = corner_flags_flat(pts, off, sc.corner_deg)
    lead = trav * (1 + bool(lift))                                        # items in front of the op's own: [pen up,] travel
    items = lead + np.where(is_tap, 1, nseg + 2)
    ibase = len(head) + np.cumsum(items) - items
    kind = np.full(len(head) + int(items.sum()), -1, np.int64)
    kind[:len(head)] = head
    if lift:
        kind[ibase[trav]] = PEN_UP
    own = ibase + lead
    kind[own[is_tap]] = TAP
    kind[own[~is_tap]] = PEN_DOWN
    kind[(own + nseg + 1)[~is_tap]] = PEN_UP
    return Plan(moves, kind, is_travel, slow_in, slow_out)


def plan_pieces(P: Plan, counts: np.ndarray, sc: StreamConfig) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(move, divider, count) of every piece in move order.  A segment without corners is one piece; every other move takes the plan of its
    (kind, step count), computed once per distinct pair with plan_travel / plan_segment and expanded with numpy."""
    counts = np.asarray(counts, np.int64)
    simple = ~P.is_travel & ~P.slow_in & ~P.slow_out
    i0 = np.nonzero(simple & (counts > 0))[0]
    pm = [i0]; pc = [counts[i0]]; pd = [np.where(counts[i0] <= sc.short_len_steps, sc.short_div, sc.div_fast).astype(np.int64)]
    i1 = np.nonzero(~simple & (counts > 0))[0]
    if len(i1):
        cls = np.where(P.is_travel[i1], 0, 1 + P.slow_in[i1] + 2 * P.slow_out[i1]).astype(np.int64)
        uniq, inv = np.unique(cls * (int(counts.max()) + 1) + counts[i1], return_inverse=True)
        plan_off = [0]; plan_div: List[int] = []; plan_cnt: List[int] = []
        for key in uniq:
            c, k = divmod(int(key), int(counts.max()) + 1)
            pcs = plan_travel(k, sc) if c == 0 else plan_segment(k, sc, bool((c - 1) & 1), bool((c - 1) & 2))
            plan_div += [d for d, _ in pcs]; plan_cnt += [q for _, q in pcs]; plan_off.append(len(plan_div))
        plan_off = np.asarray(plan_off, np.int64); plan_div = np.asarray(plan_div, np.int64); plan_cnt = np.asarray(plan_cnt, np.int64)
        lens = np.diff(plan_off)[inv]
        src = np.repeat(plan_off[inv], lens) + np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
        pm.append(np.repeat(i1, lens)); pd.append(plan_div[src]); pc.append(plan_cnt[src])
    pm, pd, pc = np.concatenate(pm), np.concatenate(pd), np.concatenate(pc)
    order = np.argsort(pm, kind="stable")
    return pm[order], pd[order], pc[order]


# ------------------------------------------------------------------ byte layout
@dataclass
class PieceTable:
    """Where every byte of a plot comes from.  Piece i (a run of steps at one divider) reads cnt[i] direction codes from code0[i] on and owns the bytes
    from pos[i]: its speed byte when speed[i] >= 0, then (cnt[i] + 1) // 2 step bytes, the steps paired inside the piece.  Pieces without bytes are not
    listed.  Service bytes (the end byte among them) are svc_val at svc_pos; nbytes is the padded length, every other byte is zero."""
    code0: np.ndarray
    cnt: np.ndarray
    pos: np.ndarray
    speed: np.ndarray
    svc_pos: np.ndarray
    svc_val: np.ndarray
    nbytes: int


def layout(kind: np.ndarray, pm: np.ndarray, pd: np.ndarray, pc: np.ndarray, off: np.ndarray, initial_div: Optional[int] = None) -> PieceTable:
    """Byte positions of a plot.  kind: per item a service byte (>= 0) or -1 for the next move; (pm, pd, pc): move index, divider and step count of every
    piece, in move order and plan order inside a move; off: first code of every move.  initial_div: the divider already set when the first piece starts
    (StreamWriter.set_speed writes nothing for the divider it holds, helper :139-143); None: nothing set yet, the first piece writes its speed byte."""
    kind = np.asarray(kind, np.int64)
    is_move = kind < 0
    nmov = int(is_move.sum())
    first_of_move = np.r_[True, pm[1:] != pm[:-1]] if len(pm) else np.zeros(0, bool)
    csum = np.cumsum(pc) - pc
    within = csum - np.maximum.accumulate(np.where(first_of_move, csum, 0)) if len(pm) else np.zeros(0, np.int64)
    pstart = off[pm] + within if len(pm) else np.zeros(0, np.int64)
    spd = np.ones(len(pm), bool)
    if len(pm) > 1:
        spd[1:] = pd[1:] != pd[:-1]
    if len(pm) and initial_div is not None:
        spd[0] = pd[0] != initial_div
    pbytes = spd.astype(np.int64) + (pc + 1) // 2
    move_bytes = np.zeros(nmov, np.int64)
    np.add.at(move_bytes, pm, pbytes)
    item_bytes = np.ones(len(kind), np.int64)
    item_bytes[is_move] = move_bytes
    item_pos = np.cumsum(item_bytes) - item_bytes
    total = int(item_bytes.sum())
    bsum = np.cumsum(pbytes) - pbytes
    ppos = item_pos[is_move][pm] + bsum - np.maximum.accumulate(np.where(first_of_move, bsum, 0)) if len(pm) else np.zeros(0, np.int64)
    sp = np.clip(pd, 0, 63)                                               # make_speed_byte (helper :46-51)
    speed = np.where(spd, 0x40 | (sp & 0x3F), -1)
    live = pbytes > 0
    svc_pos = np.r_[item_pos[~is_move], total].astype(np.int64)
    svc_val = np.r_[kind[~is_move], EOF_BYTE].astype(np.uint8)
    nbytes = total + 1 + (-(total + 1)) % SPI_CHUNK_SIZE
    return PieceTable(pstart[live].astype(np.int64), pc[live].astype(np.int32), ppos[live].astype(np.int64), speed[live].astype(np.int32), svc_pos, svc_val, nbytes)




# ------------------------------------------------------------------ the compiler
def compile_plan(P: Plan, sc: StreamConfig, device=None, codes_fn: Optional[Callable] = None, pack_fn: Optional[Callable] = None, initial_div: Optional[int] = None,
                 lap: Callable[[str], None] = lambda name: None) -> Tuple[bytes, PieceTable, np.ndarray]:
    """The bytes of a plan: direction codes of all moves, speed pieces, byte positions, packing (StreamWriter semantics, helper :130-175: a speed
    byte only when the divider changes, the steps of every piece paired on their own, end byte, padding).  The two device steps, each None = the
    GPU (orip.device.Device: the codes stay resident, the bytes are written there) -- there is no CPU path in the product:
      codes_fn(moves int32 [M, 4]) -> (off int64 [M + 1], codes or None)         orip_stream_codes
      pack_fn(table: PieceTable, codes) -> bytes                                 orip_stream_pack
    initial_div: layout().  lap(name) is called after each of "codes", "plan", "pack".  Returns (bytes, piece table, first code of every move)."""
    if codes_fn is None or pack_fn is None:
        if device is None:
            from .stages import device as _default_device
            device = _default_device()
        codes_fn = codes_fn or (lambda moves: device.stream_codes(moves, fetch_codes=False))
        pack_fn = pack_fn or device.stream_pack
    off, codes = codes_fn(P.moves)
    off = np.asarray(off, np.int64)
    lap("codes")
    pm, pd, pc = plan_pieces(P, np.diff(off), sc)
    table = layout(P.kind, pm, pd, pc, off, initial_div)
    lap("plan")
    data = pack_fn(table, codes)
    lap("pack")
    return data, table, off


def _layer_ops(ops: Sequence[dict], W: int, H: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """ops of a layer as flat arrays in step space, lines of fewer than two points dropped: (off, pts, is_tap, first point of ops[0] as given)"""
    raw = [np.array([[op["x"], op["y"]]], np.float64) if op["type"] == "tap" else np.asarray(op["points"], np.float64).reshape(-1, 2) for op in ops]
    tap = np.array([op["type"] == "tap" for op in ops], bool)
    npts = np.array([len(q) for q in raw], np.int64)
    steps = to_steps(np.concatenate(raw), W, H)                           # one call for the whole layer
    first = steps[:npts[0]][0]
    keep = tap | (npts >= 2)
    return np.concatenate([[0], np.cumsum(npts[keep])]).astype(np.int64), steps[np.repeat(keep, npts)], tap[keep], first


def plan_layers(layers: Sequence[Tuple[str, int, Sequence[dict]]], W: int, H: int, sc: StreamConfig, color_maps=(None, None, None)) -> Tuple[Plan, Dict[str, int]]:
    """The plan of 13:231-281 for layers given as (colour name, manifest colour index, ops), and the ops counted by type; per layer 13:179-227: the
    approach to the first op (a travel without a pen-up byte), the colour byte, the ops."""
    force, by_name, by_order = color_maps
    plans = [fixed_plan([PEN_UP])]
    cur = np.zeros(2, np.int64)
    n_lines = n_taps = 0
    for ordinal, (name, orig_idx, ops) in enumerate(layers):
        cidx = resolve_color_index(name, orig_idx, ordinal, force, by_name, by_order)
        n_lines += sum(1 for o in ops if o["type"] == "line"); n_taps += sum(1 for o in ops if o["type"] == "tap")
        off, pts, is_tap = np.zeros(1, np.int64), np.zeros((0, 2), np.int64), np.zeros(0, bool)
        if ops:
            off, pts, is_tap, first = _layer_ops(ops, W, H)
            if (cur != first).any():
                plans.append(fixed_plan([-1], [[*cur, *first]])); cur = first
        if not (0 <= cidx <= 7):
            raise ValueError("color index 0..7")
        plans.append(plan_ops(off, pts, is_tap, cur, [0x08 | (cidx & 7)], True, sc))
        if len(pts):
            cur = pts[-1]
    return concat_plans(plans), {"lines": n_lines, "taps": n_taps}


def build_stream(layers: Sequence[Tuple[str, int, Sequence[dict]]], W: int, H: int, sc: StreamConfig, codes_fn: Optional[Callable] = None,
                 color_maps=(None, None, None), device=None, pack_fn: Optional[Callable] = None) -> Tuple[bytes, Dict[str, int]]:
    """plot_stream.bin of stage 13 and its counts: plan_layers() through compile_plan() (device / codes_fn / pack_fn: there)."""
    P, meta = plan_layers(layers, W, H, sc, color_maps)
    data, _, _ = compile_plan(P, sc, device, codes_fn, pack_fn)
    return data, dict(meta, bytes=len(data))
