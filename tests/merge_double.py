"""TEST INFRASTRUCTURE: --merge-paths restated sequentially (the rule of include/orip.h: orip_gcode_merge), independently of csrc/gcode_merge.hip and of
orip/: a dict from (group, x, y) to the ends on it, the joins by the four conditions, the chains walked one by one from their lowest member.  No hash
table, no pointer jumping, no scans."""
import numpy as np

HEAD, TAIL = 0, 1


def joins_of(off, pts, group, reverse):
    """{(path, end): (path, end)} for every joined end, both ways round"""
    nodes = {}
    for p in range(len(off) - 1):
        for end, i in ((HEAD, off[p]), (TAIL, off[p + 1] - 1)):
            nodes.setdefault((int(group[p]), int(pts[i][0]), int(pts[i][1])), []).append((p, end))
    partner = {}
    for ends in nodes.values():
        if len(ends) != 2:
            continue
        (p, a), (q, b) = ends
        if p != q and (a != b or reverse):
            partner[(p, a)] = (q, b); partner[(q, b)] = (p, a)
    return partner, nodes


def merge_numpy(off, pts, group, n_groups, reverse=False):
    """-> (off int64, pts int32 [total, 2], member_off int64, member int32 [n], rev bool [n], {"paths_out", "points_out", "joins", "cycles"})"""
    off = [int(v) for v in np.asarray(off, np.int64).reshape(-1)]
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    n = len(off) - 1
    group = [0] * n if group is None else [int(v) for v in np.asarray(group).reshape(-1)]
    assert len(group) == n and all(0 <= g < n_groups for g in group) and all(b - a >= 2 for a, b in zip(off[:-1], off[1:]))
    partner, _ = joins_of(off, pts, group, bool(reverse))
    used = [False] * n
    out_off, out_pts, member_off, member, rev = [0], [], [0], [], []
    cycles = 0
    for m in range(n):
        if used[m]:
            continue                                   # every path below m is placed: m is the lowest member of its chain
        chain = [(m, False)]
        leave, closed = (m, TAIL), False
        while leave in partner:                        # on from the tail of m
            q, end = partner[leave]
            if q == m:
                closed = True
                break
            chain.append((q, end == TAIL))             # entered through its tail: drawn backwards
            leave = (q, TAIL if end == HEAD else HEAD)
        if not closed:
            front, enter = [], (m, HEAD)
            while enter in partner:                    # and back from its head to the free end
                q, end = partner[enter]
                front.append((q, end == HEAD))         # left through its head: drawn backwards
                enter = (q, TAIL if end == HEAD else HEAD)
            chain = front[::-1] + chain
        cycles += closed
        for k, (p, r) in enumerate(chain):
            assert not used[p]
            used[p] = True
            seg = pts[off[p]:off[p + 1]]
            seg = seg[::-1] if r else seg
            if k:
                assert (seg[0] == out_pts[-1][-1]).all()
                seg = seg[1:]
            out_pts.append(seg); member.append(p); rev.append(r)
        out_off.append(out_off[-1] + sum(len(s) for s in out_pts[len(member) - len(chain):]))
        member_off.append(len(member))
    allp = np.concatenate(out_pts).astype(np.int32) if out_pts else np.zeros((0, 2), np.int32)
    st = {"paths_out": len(out_off) - 1, "points_out": len(allp), "joins": n - (len(out_off) - 1), "cycles": int(cycles)}
    return (np.asarray(out_off, np.int64), allp.reshape(-1, 2), np.asarray(member_off, np.int64), np.asarray(member, np.int32).reshape(-1),
            np.asarray(rev, bool).reshape(-1), st)
