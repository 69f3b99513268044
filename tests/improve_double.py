"""TEST INFRASTRUCTURE: --improve-order as include/orip.h states it (orip_gcode_improve), brute force: every round looks at every move R(i, j) and
M(i, L, p) of the group, takes the one with the largest gain (among equals the lowest (code, i, second index)) and applies it alone.  Written from the
header's text, not from csrc/gcode_improve.hip: no tiles, no records, no position maps -- the sequence is a Python list that is cut and spliced."""
import numpy as np

MAX_PATHS = 65536                    # ORIP_IMPROVE_MAX_PATHS
STAT_NAMES = ("travel_before", "travel_after", "rounds", "converged_groups", "skipped_groups")


def _d(p, q):
    """steps of a travel: max(|dx|, |dy|), broadcasting over leading axes"""
    return np.abs(p - q).max(-1)


def entries(ends, order, rev):
    """-> (a, b) int64 [m, 2]: where the stroke at every position is entered and where it is left"""
    e = np.asarray(ends, np.int64).reshape(-1, 4)[np.asarray(order, np.int64)]
    r = np.asarray(rev, bool)[:, None]
    return np.where(r, e[:, 2:], e[:, :2]), np.where(r, e[:, :2], e[:, 2:])


def travel(ends, order, rev, start=(0, 0)):
    """pen-up steps of the whole sequence from `start`: every link of every group, the approaches between groups included"""
    a, b = entries(ends, order, rev)
    if len(a) == 0:
        return 0
    prev = np.concatenate([np.asarray(start, np.int64).reshape(1, 2), b[:-1]])
    return int(_d(prev, a).sum())


def best_move(a, b, cursor, reverse):
    """the move one round takes for a group given by its entry / exit points in position order -> (gain, code, i, second) with second = j for R (code 0)
    and p for M (code L), or (0, -1, -1, -1) when the group has no move at all.  A gain <= 0 means the group is done."""
    a = np.asarray(a, np.int64).reshape(-1, 2); b = np.asarray(b, np.int64).reshape(-1, 2)
    m = len(a)
    if m == 0:
        return (0, -1, -1, -1)
    bp = np.concatenate([np.asarray(cursor, np.int64).reshape(1, 2), b])          # bp[k] = b_{k-1}, k = 0 .. m
    an = np.concatenate([a, np.zeros((1, 2), np.int64)])                          # an[k] = a_k; an[m] does not exist
    has = np.arange(m + 1) < m                                                     # a term that mentions a_m is 0
    link = np.where(has, _d(bp, an), 0)                                            # link[k], k = 0 .. m; link[m] = 0

    def to_a(p, k):                                                                # d(p, a_k), 0 where k == m
        return np.where(has[k], _d(p, an[k]), 0)
    best = None
    if reverse:
        i = np.arange(m)[:, None]; j = np.arange(m)[None, :]
        g = link[i] + link[j + 1] - _d(bp[i], b[j]) - to_a(a[i], j + 1)
        g = np.where(j >= i, g, np.iinfo(np.int64).min)
        f = int(np.argmax(g))                                                      # the first maximum in (i, j) order
        best = (int(g.flat[f]), 0, f // m, f % m)
    for L in (1, 2, 3):
        if m - L + 1 <= 0:
            continue
        i = np.arange(m - L + 1)[:, None]; p = np.arange(-1, m)[None, :]
        j = i + L - 1
        g = link[i] + link[j + 1] - to_a(bp[i], j + 1) + link[p + 1] - _d(bp[p + 1], a[i]) - to_a(b[j], p + 1)
        ok = (p < i - 1) | (p > j)
        if not ok.any():
            continue
        g = np.where(ok, g, np.iinfo(np.int64).min)
        f = int(np.argmax(g))
        cand = (int(g.flat[f]), L, f // (m + 1), f % (m + 1) - 1)
        if best is None or cand[0] > best[0]:                                      # codes ascend, so an equal gain keeps the lower code
            best = cand
    return best if best is not None else (0, -1, -1, -1)


def apply_move(seq, code, i, second):
    """seq: list of (stroke, reversed) in position order -> the list after the move"""
    if code == 0:
        j = second
        return seq[:i] + [(s, not r) for s, r in reversed(seq[i:j + 1])] + seq[j + 1:]
    L, p = code, second
    block, rest = seq[i:i + L], seq[:i] + seq[i + L:]
    at = p + 1 if p < i else p + 1 - L                                            # behind old position p, counted in the list without the block
    return rest[:at] + block + rest[at:]


def improve(ends, group, n_groups, order, rev, reverse=False, start=(0, 0), max_rounds=None, trace=None):
    """-> (order int32 [n], rev bool [n], stats dict).  max_rounds None: 2 m + 64 rounds for a group of m strokes.  trace: a list that receives
    (group, gain, code, i, second) of every applied move."""
    e = np.asarray(ends, np.int64).reshape(-1, 4)
    grp = np.asarray(group, np.int64).reshape(-1)
    order = np.asarray(order, np.int64).reshape(-1).copy(); rev = np.asarray(rev, bool).reshape(-1).copy()
    n = len(order)
    st = dict.fromkeys(STAT_NAMES, 0)
    st["travel_before"] = travel(e, order, rev, start)
    cursor = np.asarray(start, np.int64)
    og = grp[order]
    for g in range(int(n_groups)):
        pos = np.nonzero(og == g)[0]
        m = len(pos)
        if m == 0:
            continue
        lo = int(pos[0])
        assert np.array_equal(pos, np.arange(lo, lo + m)), "the groups of the order must not decrease"
        if m > MAX_PATHS:
            st["skipped_groups"] += 1
        else:
            seq = [(int(s), bool(r)) for s, r in zip(order[lo:lo + m], rev[lo:lo + m])]
            cap = 2 * m + 64 if max_rounds is None else int(max_rounds)
            for _ in range(cap):
                so = np.array([s for s, _ in seq]); sr = np.array([r for _, r in seq])
                a, b = entries(e, so, sr)
                gain, code, i, second = best_move(a, b, cursor, reverse)
                if gain <= 0:
                    st["converged_groups"] += 1
                    break
                seq = apply_move(seq, code, i, second)
                st["rounds"] += 1
                if trace is not None:
                    trace.append((g, gain, code, i, second))
            order[lo:lo + m] = [s for s, _ in seq]; rev[lo:lo + m] = [r for _, r in seq]
        last = lo + m - 1
        cursor = e[order[last], :2] if rev[last] else e[order[last], 2:]
    st["travel_after"] = travel(e, order, rev, start)
    return order.astype(np.int32), rev, st
