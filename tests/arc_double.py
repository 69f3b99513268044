"""The sequential double of orip_gcode_flatten (include/orip.h states the rule; csrc/gcode_arc.hip is the device side): one arc at a time, in plain Python
floats and math.sqrt.  Every operation below is one IEEE double operation rounded to nearest, as on the device, and CPython fuses nothing, so the points
repeat the device's bit for bit.  No sin, cos or atan2 anywhere.

flatten(table, tol) is also the flatten_fn of orip.gcode.build_stream_from_gcode; the parser needs no double of its own (orip.gcode.parse_gcode_arcs runs on
the host and is tested as it is)."""
import math

import numpy as np

MAX_M = 16                      # include/orip.h: ORIP_ARC_MAX_DEPTH
MAX_POINTS = (1 << 30) - 1
LINE, CW, CCW = 1, 2, 3


class FlattenError(ValueError):
    """what the device refuses: .what is one of "tol", "kind", "finite", "radius", "depth", "points", "chain" """
    def __init__(self, what, text):
        super().__init__(text); self.what = what


def turn(u, d):
    """a quarter turn of u in direction d (+1 counter-clockwise, -1 clockwise): exact"""
    return (-u[1], u[0]) if d > 0 else (u[1], -u[0])


def _unit_mid(uL, uR):
    sx = uL[0] + uR[0]; sy = uL[1] + uR[1]
    n = math.sqrt(sx * sx + sy * sy)
    return (sx / n, sy / n)


class Arc:
    """steps 1 to 3 of the rule for one arc: rA, rB, the joints J[0 .. S] of its S spans, the depth m, the pieces N"""
    def __init__(self, kind, A, B, C, tol, force_m=None):
        d = 1 if kind == CCW else -1
        if not all(math.isfinite(v) for v in (*A, *B, *C)):
            raise FlattenError("finite", "a coordinate is not finite")
        ax = A[0] - C[0]; ay = A[1] - C[1]; bx = B[0] - C[0]; by = B[1] - C[1]
        rA = math.sqrt(ax * ax + ay * ay); rB = math.sqrt(bx * bx + by * by)
        if not (math.isfinite(rA) and math.isfinite(rB)):
            raise FlattenError("finite", "a radius is not finite")
        if rA == 0.0 or rB == 0.0:
            raise FlattenError("radius", "a radius is 0")
        uA = (ax / rA, ay / rA); uB = (bx / rB, by / rB)
        r = max(rA, rB)
        self.full = A[0] == B[0] and A[1] == B[1]
        if self.full:
            q1 = turn(uA, d); q2 = turn(q1, d); q3 = turn(q2, d)
            J = [uA, q1, q2, q3, turn(q3, d)]
            quarter = True
        else:
            k = ax * by - ay * bx
            k = k if d > 0 else -k
            dot = ax * bx + ay * by
            if k > 0.0:
                j = 0 if dot > 0.0 else 1
            elif k < 0.0:
                j = 3 if dot >= 0.0 else 2
            else:
                j = 0 if dot >= 0.0 else 2
            J = [uA]
            for _ in range(j):
                J.append(turn(J[-1], d))
            if not (uB[0] == J[-1][0] and uB[1] == J[-1][1]):
                J.append(uB)
            quarter = j >= 1
        S = len(J) - 1
        m = 0
        if S > 0:
            c = math.sqrt(0.5) if quarter else math.sqrt((1.0 + (uA[0] * uB[0] + uA[1] * uB[1])) / 2.0)
            while not (r * (1.0 - c) <= tol):
                m += 1
                if m > MAX_M:
                    raise FlattenError("depth", "an arc needs more than 2^18 pieces at this tolerance")
                c = math.sqrt((1.0 + c) / 2.0)
            if force_m is not None:
                m = force_m
        self.kind = kind
        self.A, self.B, self.C, self.rA, self.rB, self.J, self.S, self.m = A, B, C, rA, rB, J, S, m
        self.N = (S << m) if S > 0 else 1              # no span is left (uB is uA, yet B is not A): one piece, to B

    def direction(self, g):
        """step 4: the unit vector of piece joint g, 0 < g < N"""
        s, i = g >> self.m, g & ((1 << self.m) - 1)
        uL, uR = self.J[s], self.J[s + 1]
        lo, hi = 0, 1 << self.m
        u = uL
        while i != lo:
            mid = (lo + hi) >> 1
            u = _unit_mid(uL, uR)
            if i == mid:
                break
            if i < mid:
                uR, hi = u, mid
            else:
                uL, lo = u, mid
        return u

    def point(self, g):
        """step 5: point g of the arc, 0 < g <= N (g == N: B as given)"""
        if g == self.N:
            return self.B
        u = self.direction(g)
        t = g / self.N
        rho = self.rA + (self.rB - self.rA) * t
        return (self.C[0] + rho * u[0], self.C[1] + rho * u[1])

    def points(self):
        return [self.point(g) for g in range(1, self.N + 1)]


def check_table(kind, seg, sub_off, tol):
    kind = np.asarray(kind, np.int64).reshape(-1); seg = np.asarray(seg, np.float64).reshape(-1, 6); sub_off = np.asarray(sub_off, np.int64).reshape(-1)
    if not (tol > 0.0) or not math.isfinite(tol):
        raise FlattenError("tol", "the tolerance must be a positive finite number")
    if ((kind < 1) | (kind > 3)).any():
        raise FlattenError("kind", "a kind outside 1..3")
    n = len(sub_off) - 1
    if n < 0 or (n == 0) != (len(kind) == 0) or (n and (sub_off[0] != 0 or sub_off[-1] != len(kind) or (np.diff(sub_off) < 1).any())):
        raise FlattenError("chain", "the subpaths' segment ranges")
    for p in range(n):
        for s in range(int(sub_off[p]) + 1, int(sub_off[p + 1])):
            if not (seg[s, 0] == seg[s - 1, 2] and seg[s, 1] == seg[s - 1, 3]):
                raise FlattenError("chain", f"segment {s} does not start where its predecessor ends")
    return kind, seg, sub_off


def flatten(table, tol, force_m=None):
    """(kind, seg, sub_off) or an orip.gcode.ArcTable -> (off int64 [n_sub + 1], pts float64 [total, 2], {"arcs", "pieces", "full_circles"})"""
    kind, seg, sub_off = check_table(table[0], table[1], table[2], tol)
    pts, off = [], [0]
    arcs = pieces = full = 0
    for p in range(len(sub_off) - 1):
        a, b = int(sub_off[p]), int(sub_off[p + 1])
        pts.append((float(seg[a, 0]), float(seg[a, 1])))
        for s in range(a, b):
            A, B, C = (float(seg[s, 0]), float(seg[s, 1])), (float(seg[s, 2]), float(seg[s, 3])), (float(seg[s, 4]), float(seg[s, 5]))
            if kind[s] == LINE:
                if not all(math.isfinite(v) for v in (*A, *B)):
                    raise FlattenError("finite", "a coordinate is not finite")
                pts.append(B)
            else:
                arc = Arc(int(kind[s]), A, B, C, tol, force_m)
                pts.extend(arc.points())
                arcs += 1; pieces += arc.N; full += bool(arc.full)
        off.append(len(pts))
        if len(pts) > MAX_POINTS:
            raise FlattenError("points", "2^30 points or more")
    return np.asarray(off, np.int64), np.asarray(pts, np.float64).reshape(-1, 2), {"arcs": arcs, "pieces": pieces, "full_circles": full}


def flatten_fn(table, tol):
    """the flatten_fn of orip.gcode.build_stream_from_gcode"""
    return flatten(table, tol)
