"""Inputs of tests/test_gpu_greedy_windows.py: lists of 2 000 .. 4 000 polylines on the 25-px lattice of greedy_cases.lattice_polys that drive the grid
kernel of the greedy order (vector_greedy.hip: k_greedy_nn_fast) through its WIDE rounds -- windows of 7 x 7 cells and more, which the kernel scans
in one pass per 64 rows -- and a plain restatement of what the kernel does with them (window_stats): the host's grid side G, the kernel's cell shift,
the window sequence r = 1, 3, 7, ... and the gap rule, on top of greedy_cases.greedy07.  tests/test_oracle_greedy_windows.py holds the restatement to
the oracle's order and reads from it that the inputs do what they were chosen for.  Everything lies within 15 bits, so the grid kernel runs."""
import numpy as np

import greedy_cases as C

L = C.LATTICE


def tiny(x, y, dx=L, dy=0):
    """an isolated two-point polyline"""
    return [[x, y], [x + dx, y + dy]]


def square(x, y, s):
    """a closed contour entered at (x, y); under rule07 it ends at (x, y + s), which is never a candidate"""
    return [[x, y], [x + s, y], [x + s, y + s], [x, y + s], [x, y]]


def far_clusters():
    """four clusters in the corners of a 16 000-px square: an emptied cluster forces rounds up to r = 63, clipped at every border and corner"""
    return C.lattice_polys(21, 2200, [(400, 400), (15600, 400), (400, 15600), (15600, 15600)], 12)


def ladder():
    """isolated short polylines at gaps that double, along a diagonal and along one axis, and two chains at a constant pitch of 600 and of 1 400 px"""
    ex = []
    p = 2300
    for gap in (300, 600, 1200, 2400, 4800):                 # the diagonal
        p += gap
        ex.append(tiny(p, p))
    x = 1000
    for gap in (0, 300, 600, 1200, 2400, 4800, 4800):        # along x at y = 15 000
        x += gap
        ex.append(tiny(x, 15000))
    ex += [tiny(3000 + 600 * k, 100) for k in range(16)]     # every step along it ends at r = 3
    ex += [tiny(15900, 600 + 1400 * k, 0, L) for k in range(10)]      # ... at r = 7
    return C.lattice_polys(22, 2000, [(1500, 1500)], 20, ex)


def crowded():
    """blobs of several hundred end points inside one or two cells, thousands of px apart: the round that reaches the next blob holds more than 128 candidates"""
    big = C.lattice_polys(23, 1900, [(300, 300), (4300, 500), (900, 5500), (9000, 9000), (12000, 2000), (2500, 12000), (15000, 8000), (7000, 15500)], 3)
    return big + C.lattice_polys(33, 100, [(6000, 12000), (13000, 12500)], 2)        # two small ones: 65 .. 128 candidates, two trips


def closed_wide():
    """closed contours of 200 px at a pitch of 900 px next to a cluster: entered from wide rounds, their far ends nearer to the cursor than their starts"""
    ex = [square(3000 + 900 * i, 3000 + 900 * j, 200) for i in range(8) for j in range(8)]
    ex += [tiny(3450 + 1800 * i, 2500 + 1800 * j) for i in range(4) for j in range(4)]
    return C.lattice_polys(24, 2000, [(1200, 1200)], 16, ex)


def rows65():
    """88 rows of 256 px in use (y from -11 000 to 11 400, within the signed 15 bits): leaving the first cluster takes the window that covers the grid, and
    the nearest polyline lies beyond its 64th row (the kernel's second pass over the rows)"""
    ex = [tiny(x, y) for x in (-9000, 8000) for y in (-11000, 11400)]        # and four lone ones in the corners
    return C.lattice_polys(25, 2500, [(0, -10800), (3000, 6000), (-2000, 11200)], 6, ex)


CASES = {"far_clusters": far_clusters, "ladder": ladder, "crowded": crowded, "closed_wide": closed_wide, "rows65": rows65}


def host_G(n):
    """vreorder's grid side"""
    G = 8
    while G < 128 and (G + 8) * (G + 8) <= 4 * n and n * 12 + ((G + 8) * (G + 8) + 1) * 4 + 64 <= 158 * 1024:
        G += 8
    return G


def seed_index(polys):
    from oracle import oracle as O
    return int(np.argmax([O.arc_length(p, True) for p in polys]))            # the first of equal maxima


def window_stats(polys, order):
    """What k_greedy_nn_fast does along `order` (greedy_cases.greedy07's): per step the rounds r = 1, 3, 7, ... up to the first one whose best candidate
    passes the gap test or whose window covers the grid.  Returns a dict of counts; raises if a round's winner is not the order's."""
    start, end, closed = C.ends07(polys)
    n = len(polys); G = host_G(n); Gm1 = G - 1
    allxy = np.concatenate([start, end])
    ox, oy = int(allxy[:, 0].min()), int(allxy[:, 1].min())
    ext = max(int(allxy[:, 0].max()) - ox, int(allxy[:, 1].max()) - oy)
    sh = 0
    while (ext >> sh) >= G:
        sh += 1
    cell = 1 << sh
    # entries: the start of every polyline, the end of every polyline that may be read backwards
    opn = np.flatnonzero(~closed)
    ent_poly = np.concatenate([np.arange(n), opn])
    ent_xy = np.concatenate([start, end[opn]]) - np.array([ox, oy])
    ent_c = ent_xy >> sh
    ent_f = ent_xy.astype(np.float32)
    far_end = (end - np.array([ox, oy])).astype(np.float32)                  # of closed contours: no entry
    used = np.zeros(n, bool); used[order[0][0]] = True
    st = dict(G=G, sh=sh, ends={}, wide_rounds=0, wide_over64=0, wide_over128=0, wide_ties=0, wide_closed=0, wide_far_end_nearer=0, clips=set(),
              over64rows=0, winner_beyond_row64=0, max_rows=0)
    i0, f0 = order[0]
    cur = start[i0] if closed[i0] or f0 else end[i0]
    for k in range(1, n):
        cx, cy = int(cur[0]) - ox, int(cur[1]) - oy
        gx, gy = cx >> sh, cy >> sh
        D = np.abs(ent_c - np.array([gx, gy])).max(1)
        d = ent_f - np.array([cx, cy], np.float32)
        d2 = (d * d).sum(1, dtype=np.float32)
        free = ~used[ent_poly]
        r = 1
        while True:
            x0, x1, y0, y1 = max(0, gx - r), min(Gm1, gx + r), max(0, gy - r), min(Gm1, gy + r)
            inwin = D <= r
            cand = inwin & free
            total = int(inwin.sum())
            rows = y1 - y0 + 1
            if r >= 3:
                st["wide_rounds"] += 1; st["wide_over64"] += total > 64; st["wide_over128"] += total > 128
                st["over64rows"] += rows > 64; st["max_rows"] = max(st["max_rows"], rows)
                st["clips"] |= {s for s, c in (("x0", gx - r < 0), ("x1", gx + r > Gm1), ("y0", gy - r < 0), ("y1", gy + r > Gm1)) if c}
            final = x0 == 0 and y0 == 0 and x1 == Gm1 and y1 == Gm1
            mink = d2[cand].min() if cand.any() else None
            if not final and mink is not None:
                if r == 1:
                    lx, ly = cx & (cell - 1), cy & (cell - 1)
                    gap = cell + min(lx + 1, cell - lx, ly + 1, cell - ly)
                else:
                    gap = 0x7fff
                    if x0 > 0: gap = min(gap, cx - (x0 << sh) + 1)
                    if x1 < Gm1: gap = min(gap, ((x1 + 1) << sh) - cx)
                    if y0 > 0: gap = min(gap, cy - (y0 << sh) + 1)
                    if y1 < Gm1: gap = min(gap, ((y1 + 1) << sh) - cy)
                g2 = gap * gap
                final = int(np.floor(mink)) + 1 <= g2 - (g2 >> 18) - 1 and g2 > 1
            if final:
                break
            r = 2 * r + 1
        assert mink is not None, "the window that covers the grid holds every unused polyline"
        best = np.flatnonzero(cand & (d2 == mink))
        win = int(ent_poly[best].min())
        i, flip = order[k]
        assert win == i, (k, win, i)
        st["ends"][r] = st["ends"].get(r, 0) + 1
        if r >= 3:
            st["wide_ties"] += len(set(ent_poly[best].tolist())) > 1
            st["wide_closed"] += bool(closed[i])
            fe = closed & ~used
            if fe.any():
                df = far_end[fe] - np.array([cx, cy], np.float32)
                st["wide_far_end_nearer"] += bool(((df * df).sum(1, dtype=np.float32) < mink).any())
            if rows > 64:
                wr = ent_c[best[ent_poly[best] == win], 1]
                st["winner_beyond_row64"] += bool((wr - y0 >= 64).all())
        used[i] = True
        cur = start[i] if closed[i] or flip else end[i]
    return st
