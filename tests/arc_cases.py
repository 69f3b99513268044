"""Small named inputs of orip_gcode_flatten (include/orip.h), each a handful of segments: (kind int32 [n_seg], seg float64 [n_seg, 6] = Ax Ay Bx By Cx Cy,
sub_off int64 [n_sub + 1], tol).  sin and cos appear here only to make inputs; the rule itself uses neither.  Every case keeps its centre within 2^8
radii of the origin, which the rounding bound of tests/test_arc_host.py relies on."""
import math

import numpy as np

LINE, CW, CCW = 1, 2, 3


def table(subpaths, tol):
    """subpaths: lists of (kind, A, B, C) -> a case"""
    kind = [s[0] for sp in subpaths for s in sp]
    seg = [[*s[1], *s[2], *(s[3] if s[3] is not None else (0.0, 0.0))] for sp in subpaths for s in sp]
    off = np.concatenate([[0], np.cumsum([len(sp) for sp in subpaths])]).astype(np.int64)
    return np.asarray(kind, np.int32), np.asarray(seg, np.float64).reshape(-1, 6), off, float(tol)


def on_circle(C, r, deg):
    a = math.radians(deg)
    return (C[0] + r * math.cos(a), C[1] + r * math.sin(a))


def sweep(kind, C, r, deg0, deg, hair=0.0):
    """an arc of `deg` degrees (plus `hair` radians) from the angle deg0, in the direction of kind"""
    d = 1.0 if kind == CCW else -1.0
    a1 = math.radians(deg0) + d * (math.radians(deg) + hair)
    return (kind, on_circle(C, r, deg0), (C[0] + r * math.cos(a1), C[1] + r * math.sin(a1)), C)


HAIR = 1e-7


def small_cases():
    c = {}
    O = (10.0, 10.0)
    c["quarter_ccw"] = table([[(CCW, (15.0, 10.0), (10.0, 15.0), O)]], 0.01)                   # axis-parallel ends: uB falls on q1, the last span is left out
    c["quarter_cw"] = table([[(CW, (10.0, 15.0), (15.0, 10.0), O)]], 0.01)
    c["three_quarters_ccw"] = table([[(CCW, (15.0, 10.0), (10.0, 5.0), O)]], 0.01)
    c["three_quarters_cw"] = table([[(CW, (15.0, 10.0), (10.0, 15.0), O)]], 0.01)
    c["half_ccw"] = table([[(CCW, (0.0, 0.0), (10.0, 0.0), (5.0, 0.0))]], 0.0125)
    c["half_cw"] = table([[(CW, (0.0, 0.0), (10.0, 0.0), (5.0, 0.0))]], 0.0125)
    c["full_cw"] = table([[(CW, (10.0, 0.0), (10.0, 0.0), (5.0, 0.0))]], 0.0125)               # the issue's G2 X10 Y0 I-5 J0 from (10, 0)
    c["full_ccw_oblique"] = table([[(CCW, on_circle((3.0, -4.0), 2.5, 33.0), on_circle((3.0, -4.0), 2.5, 33.0), (3.0, -4.0))]], 0.003)
    for kd, nm in ((CCW, "ccw"), (CW, "cw")):
        for deg in (90, 180, 270):
            c[f"hair_over_{deg}_{nm}"] = table([[sweep(kd, (1.0, 2.0), 7.0, 20.0, deg, HAIR)]], 0.01)
            c[f"hair_under_{deg}_{nm}"] = table([[sweep(kd, (1.0, 2.0), 7.0, 20.0, deg, -HAIR)]], 0.01)
        c[f"hair_under_360_{nm}"] = table([[sweep(kd, (1.0, 2.0), 7.0, 20.0, 360, -HAIR)]], 0.01)
        c[f"hair_over_0_{nm}"] = table([[sweep(kd, (1.0, 2.0), 7.0, 20.0, 0, HAIR)]], 0.01)
    c["short_m0"] = table([[sweep(CCW, (0.0, 0.0), 1.0, 10.0, math.degrees(0.1))]], 0.01)      # 1 - cos 0.05 = 0.00125: one piece
    c["short_m1"] = table([[sweep(CW, (0.0, 0.0), 1.0, 10.0, math.degrees(0.5))]], 0.01)       # 1 - cos 0.25 = 0.031, 1 - cos 0.125 = 0.0078: two pieces
    c["radii_differ"] = table([[(CCW, (10.0, 0.0), (0.0, 10.004), (0.0, 0.0))], [(CW, (3.0, 0.0), (-3.4, 0.0), (0.0, 0.0))]], 0.005)
    c["same_ray"] = table([[(CCW, (10.0, 0.0), (10.004, 0.0), (0.0, 0.0))], [(CW, (0.0, -3.0), (0.0, -3.001), (0.0, 0.0))]], 0.005)      # uB is uA though B is not A: one piece
    c["line_arc_line"] = table([[(LINE, (0.0, 0.0), (10.0, 0.0), None), (CCW, (10.0, 0.0), (12.0, 2.0), (10.0, 2.0)), (LINE, (12.0, 2.0), (12.0, 9.0), None)],
                                [(CW, (20.0, 5.0), (25.0, 0.0), (20.0, 0.0)), (LINE, (25.0, 0.0), (25.0, -3.0), None), (CW, (25.0, -3.0), (25.0, -3.0), (24.0, -3.0))]], 0.02)
    c["lines_only"] = table([[(LINE, (0.0, 0.0), (1.0, 1.0), None)], [(LINE, (2.0, 2.0), (3.0, 2.0), None), (LINE, (3.0, 2.0), (3.0, 2.0), None)]], 0.5)
    c["r_form_short"] = gcode_case("G0 X0 Y0\nM3\nG2 X10 Y0 R6\nM5\nG0 X20 Y0\nM3\nG3 X30 Y0 R6\n", 0.01)
    c["r_form_long"] = gcode_case("G0 X0 Y0\nM3\nG2 X10 Y0 R-6\nM5\nG0 X20 Y0\nM3\nG3 X30 Y0 R-6\n", 0.01)
    c["block_of_segments"] = table([[sweep(CCW if p % 3 else CW, (float(p % 17), float(p // 17)), 0.5 + 0.01 * p, 7.0 * p, 30.0 + p)] for p in range(300)], 0.02)
    c["block_inside_a_span"] = table([[(CCW, (1000.0, 0.0), (-1000.0, 0.0), (0.0, 0.0))]], 1e-4)      # m = 11: 2048 pieces in each of two spans
    return c


def gcode_case(text, tol):
    from orip import gcode as GC
    t, _ = GC.parse_gcode_arcs(text)
    return np.asarray(t.kind, np.int32), np.asarray(t.seg, np.float64), np.asarray(t.sub_off, np.int64), float(tol)


def random_case(seed, n_sub=40, tol=0.02):
    """chains of lines and arcs: any centre within +-100, radii from 1 to 30, any sweep, both directions, some full circles"""
    rng = np.random.default_rng(seed)
    subs = []
    for _ in range(n_sub):
        P = (float(rng.uniform(-100, 100)), float(rng.uniform(-100, 100)))
        sp = []
        for _ in range(int(rng.integers(1, 6))):
            what = int(rng.integers(0, 8))
            if what < 2:
                Q = (P[0] + float(rng.uniform(-20, 20)), P[1] + float(rng.uniform(-20, 20)))
                sp.append((LINE, P, Q, None))
            else:
                kd = CCW if what & 1 else CW
                r, a0 = float(rng.uniform(1, 30)), float(rng.uniform(0, 2 * math.pi))
                C = (P[0] - r * math.cos(a0), P[1] - r * math.sin(a0))
                if what == 7:
                    Q = P
                else:
                    a1 = a0 + (1.0 if kd == CCW else -1.0) * float(rng.uniform(0.01, 2 * math.pi - 0.01))
                    Q = (C[0] + r * math.cos(a1), C[1] + r * math.sin(a1))
                sp.append((kd, P, Q, C))
            P = Q
        subs.append(sp)
    return table(subs, tol)


RANDOM_SEEDS = (11, 12, 13)

# the whole tool: a circle made of two G2 halves, and a rounded rectangle (lines and four G3 fillets), closed, in mm on an A4 sheet
TOOL_GCODE = """G21 G90 G17
G0 X60 Y50
M3
G2 X40 Y50 I-10 J0
X60 Y50 I10 J0
M5
G0 X85 Y40
M3
G1 X115 Y40
G3 X120 Y45 I0 J5
G1 Y75
G3 X115 Y80 I-5 J0
G1 X85
G3 X80 Y75 J-5
G1 Y45
G3 X85 Y40 I5
M5
"""
