// csrc/gcode_order.hip -- the nearest-neighbour order of the step polylines of svg_to_stream/gcode2stream.py (order_paths_nearest :151-172), as one list
// (orip_gcode_order) and group by group with reversible strokes (orip_gcode_order_pens); and, ours, the same walk with a closed stroke entered at its
// nearest ring vertex (orip_gcode_order_rings, 2c).  ONE search serves all three: gc_search below.
//
// 2. Order.  The reference starts at (0, 0) and takes, again and again, the remaining path whose FIRST point has the smallest L1 distance from the cursor,
//    the lowest index on ties; the cursor moves to that path's LAST point.  That is a chain of n dependent searches over n points: n^2 / 2 distances.  Here
//    the first points are bucketed into a grid of square cells (a power of two wide, about two points per cell, 16 bytes per point: x, y, id), in global
//    memory, where the grid of a 10^6-path plot (16 MB + 8 bytes per cell) stays in L2.  ONE wave walks the chain; its lanes do the search of a step:
//      * the window starts as the 3 x 3 cells around the cursor's cell and grows by one ring of cells at a time; four lanes share a cell (entries j, j + 4,
//        ...), so a pass looks at 16 cells; a cell of more than GC_BIG entries is scanned by all 64 lanes instead (thousands of paths that start on
//        one point are one such cell);
//      * the key of an entry is (L1 distance << 32) | id, id = 2 * index (+ 1 for a path's last point, 2b), the search takes the minimum: exactly the
//        reference's `d < best_d` over a list in index order;
//      * the search stops once the best distance is SMALLER than the distance from the cursor to the nearest window border that still has cells behind
//        it: every point outside the window is at least that far in one coordinate alone, hence in L1, so it can neither win nor tie.  A border on the
//        edge of the grid has nothing behind it; with all four there the whole grid has been seen.  A cursor outside the bounding box of the first
//        points adds its distance from the box in the OTHER coordinate to each border's bound (all first points on one row, the cursor far above it:
//        without that term every step would scan the whole row);
//      * the winner leaves its cell (the cell's last live entry takes its place), so a cell only ever holds paths that remain.
//    Integer arithmetic throughout; coordinates are int32 in [0, 2^30], so an L1 distance fits 32 bits.  The per-step cost is three dependent L2 round trips
//    (cell headers, entries, the winner's end point and the entry that takes its place) while the window stays at 3 x 3.
//    Degenerate inputs: all first points equal, or on one row or column, give a grid of one cell, one row or one column -- same code, the big-cell path does
//    the work; a cursor outside the grid's bounding box is clamped to the nearest cell and the borders behind it count as edges of the grid; n = 0 returns
//    before any launch.
//    2b. The same walk group by group, both ends of a path as candidates (orip_gcode_order_pens; the reference's demo sheet: order_paths_nearest :197-216 of
//    stream_generators/plotter_demo/omnirevolve_plotter_demo.py inside draw_color_group :317-333): one grid per group side by side in the same arrays, the
//    cursor carried from group to group inside one launch, and a slot table through which a winner's other end leaves its cell without a search.
//
// Two kernels around the one search, because the plain order must not pay for the groups (DESIGN 6 "pens": the group descriptor, the cell offset and the
// removal's range checks cost 6 % of the chain): k_gc_chain has its grid by value and a cell offset of constant 0, k_op_chain reads both per group.  The grid
// itself is built by the same kernels for both (gc_grids); a null group array there means "everything is group 0".
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>
#include <climits>
#include <cstring>
#include <vector>

namespace {
constexpr int GC_BIG = 64;                       // a cell with more entries than this is scanned by the whole wave

struct GcGrid { int x0, y0, x1, y1, sh, gx, gy; };      // bounding box of the candidate points, log2 of the cell width, cells per side
__device__ __forceinline__ int gc_cell(const GcGrid& g, int x, int y) { return ((y - g.y0) >> g.sh) * g.gx + ((x - g.x0) >> g.sh); }
// One grid per group, side by side in the same arrays: group g owns the cells cell0 .. cell0 + gx * gy - 1, and because the entries are laid out by one
// scan over all cells, its entries are one range too -- a search that stays inside its group's cells cannot see another group's candidate.
struct OpGroup { GcGrid g; int cell0, paths; };          // box and cells over the group's candidate points; how many paths it holds

// ------------------------------------------------------------------------------------------------ the grid
__global__ __launch_bounds__(256) void k_gc_ends(const long long* __restrict__ off, const int2* __restrict__ pts, int64_t n, int4* __restrict__ se) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int2 a = pts[off[p]], b = pts[off[p + 1] - 1];
    se[p] = make_int4(a.x, a.y, b.x, b.y);
}
// candidate t: its id 2i + r (path and end), its point and its group (grp == nullptr: group 0).  Without reversal the first points only (ids 2i), with it both ends
__device__ __forceinline__ int op_cand(const int4* __restrict__ se, const int* __restrict__ grp, int t, int rev, int2& p, int& g) {
    const int i = rev ? t >> 1 : t, r = rev ? t & 1 : 0;
    const int4 e = se[i];
    p = r ? make_int2(e.z, e.w) : make_int2(e.x, e.y);
    g = grp ? grp[i] : 0;
    return 2 * i + r;
}
__global__ __launch_bounds__(256) void k_op_bbox(const int4* __restrict__ se, const int* __restrict__ grp, int m, int rev, int* __restrict__ box) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    int2 p; int g; op_cand(se, grp, t, rev, p, g);
    int* b = box + 4 * g;
    atomicMin(&b[0], p.x); atomicMin(&b[1], p.y); atomicMax(&b[2], p.x); atomicMax(&b[3], p.y);
}
__global__ __launch_bounds__(256) void k_op_count(const int4* __restrict__ se, const int* __restrict__ grp, int m, int rev, const OpGroup* __restrict__ G, unsigned* __restrict__ cnt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    int2 p; int g; op_cand(se, grp, t, rev, p, g);
    const OpGroup o = G[g];
    atomicAdd(&cnt[o.cell0 + gc_cell(o.g, p.x, p.y)], 1u);
}
__global__ __launch_bounds__(256) void k_op_fill(const int4* __restrict__ se, const int* __restrict__ grp, int m, int rev, const OpGroup* __restrict__ G, const unsigned* __restrict__ start,
                                                 unsigned* __restrict__ fill, int4* __restrict__ ent, int* __restrict__ slot) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    int2 p; int g; const int id = op_cand(se, grp, t, rev, p, g);
    const OpGroup o = G[g];
    const int c = o.cell0 + gc_cell(o.g, p.x, p.y);
    const int at = (int)(start[c] + atomicAdd(&fill[c], 1u));
    ent[at] = make_int4(p.x, p.y, id, 0);
    if (rev) slot[id] = at;                              // where candidate id sits: how a winner's other end is found without a search
}
__global__ __launch_bounds__(256) void k_gc_hdr(const unsigned* __restrict__ start, const unsigned* __restrict__ cnt, int ncell, int2* __restrict__ hdr) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < ncell) hdr[c] = make_int2((int)start[c], (int)cnt[c]);
}

// ------------------------------------------------------------------------------------------------ the search of one step
// what a lane remembers about the best entry it has seen in the current step: its key, slot and cell, and the cell's header when it was read
struct GcBest { unsigned long long key; int slot, cell, first, count; };
// DEAD (the ring order, 2c): entries never move; one that has left has id -1 and is passed over.  Nothing is removed through cell and header there, and
// the three words carry the entry itself instead: cell = x, count = y, first = the stroke (the entry's fourth word)
template <bool DEAD> __device__ __forceinline__ void gc_look(GcBest& b, const int4 e, int slot, int cell, const int2 h, int cx, int cy) {
    if (DEAD && e.z < 0) return;
    const unsigned d = (unsigned)abs(e.x - cx) + (unsigned)abs(e.y - cy);
    const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)e.z;
    if (key < b.key) { b.key = key; b.slot = slot; b.cell = DEAD ? e.x : cell; b.count = DEAD ? e.y : h.y; b.first = DEAD ? e.w : h.x; }
}
#define GCU(x) __builtin_amdgcn_readfirstlane((int)(x))

// The nearest live entry to (cx, cy) among the cells cell0 .. cell0 + gx * gy - 1 of grid g, for a block of one wave: the winner's GcBest, the same in every
// lane (key = ~0ull: nothing found, which cannot happen while the grid holds an entry).  hdr and ent are read only; they change between two searches.
// DEAD: hdr does not change, a cell's entries stay where the fill put them and live[cell] counts those that remain; a cell with none is passed over
// from that count alone, which is read past the L1 because atomics, which the L1 does not see, decrement it.  Without DEAD `live` is not looked at.
template <bool DEAD> __device__ __forceinline__ GcBest gc_search(const GcGrid& g, const int cell0, const int cx, const int cy, const int2* hdr, const int4* ent, int* live) {
    __shared__ unsigned long long s_best;
    const int lane = threadIdx.x, sub = lane & 3, slot16 = lane >> 2;
    const long long INF = 1ll << 62;
    const int ccx = min(max(cx - g.x0, 0) >> g.sh, g.gx - 1), ccy = min(max(cy - g.y0, 0) >> g.sh, g.gy - 1);
    const long long ox = max(max(g.x0 - cx, cx - g.x1), 0), oy = max(max(g.y0 - cy, cy - g.y1), 0);
    GcBest b; b.key = ~0ull; b.slot = b.cell = b.first = b.count = 0;
    unsigned long long best = ~0ull;
    for (int r = 1;; r++) {
        const int xl = ccx - r, xh = ccx + r, yl = ccy - r, yh = ccy + r;
        const int cxl = max(xl, 0), cxh = min(xh, g.gx - 1), cyl = max(yl, 0), cyh = min(yh, g.gy - 1);
        // the cells of this pass: the whole clamped block for r == 1, afterwards the ring's four sides where they lie inside the grid
        const int w = cxh - cxl + 1;
        const int iyl = max(yl + 1, 0), iyh = min(yh - 1, g.gy - 1), hcol = max(iyh - iyl + 1, 0);
        const int n0 = r == 1 ? w * (cyh - cyl + 1) : (yl >= 0 ? w : 0);
        const int n1 = r == 1 ? 0 : (yh <= g.gy - 1 ? w : 0), n2 = r == 1 ? 0 : (xl >= 0 ? hcol : 0), n3 = r == 1 ? 0 : (xh <= g.gx - 1 ? hcol : 0);
        const int T = n0 + n1 + n2 + n3;
        for (int t0 = 0; t0 < T; t0 += 16) {
            int t = t0 + slot16, cell = -1;
            int2 h = make_int2(0, 0);
            if (t < T) {
                int x, y;
                if (r == 1) { x = cxl + t % w; y = cyl + t / w; }
                else if (t < n0) { x = cxl + t; y = yl; }
                else if ((t -= n0) < n1) { x = cxl + t; y = yh; }
                else if ((t -= n1) < n2) { x = xl; y = iyl + t; }
                else { x = xh; y = iyl + (t - n2); }
                cell = cell0 + y * g.gx + x;
                h = hdr[cell];
                if (DEAD && __hip_atomic_load(&live[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 0) h.y = 0;
                if (h.y <= GC_BIG)
                    for (int j = sub; j < h.y; j += 4) gc_look<DEAD>(b, ent[h.x + j], h.x + j, cell, h, cx, cy);
            }
            unsigned long long big = __ballot(cell >= 0 && h.y > GC_BIG && sub == 0);
            while (big) {                                                  // wave-uniform loop: a crowded cell, all lanes on it
                const int l = __ffsll((long long)big) - 1;
                big &= big - 1;
                const int bc = __shfl(cell, l), bx = __shfl(h.x, l), by = __shfl(h.y, l);
                for (int j = lane; j < by; j += 64) gc_look<DEAD>(b, ent[bx + j], bx + j, bc, make_int2(bx, by), cx, cy);
            }
        }
        // the wave's minimum through LDS (one wave: the three accesses below happen in program order)
        if (lane == 0) s_best = ~0ull;
        __syncthreads();
        if (b.key != ~0ull) atomicMin(&s_best, b.key);
        __syncthreads();
        best = s_best;
        __syncthreads();
        // the least distance of a point behind each border that still has cells behind it: the way to the border in that coordinate, plus
        // the cursor's distance from the bounding box in the other one (every candidate lies inside the box; a group whose points all lie far
        // from where the previous group ended is this term's case too)
        long long bd = INF;
        if (xl > 0) bd = min(bd, (long long)cx - ((long long)g.x0 + ((long long)xl << g.sh)) + 1 + oy);
        if (yl > 0) bd = min(bd, (long long)cy - ((long long)g.y0 + ((long long)yl << g.sh)) + 1 + ox);
        if (xh < g.gx - 1) bd = min(bd, (long long)g.x0 + ((long long)(xh + 1) << g.sh) - (long long)cx + oy);
        if (yh < g.gy - 1) bd = min(bd, (long long)g.y0 + ((long long)(yh + 1) << g.sh) - (long long)cy + ox);
        if (bd == INF || (long long)(best >> 32) < bd) break;
    }
    // the winner's lane hands over where the entry sits
    const unsigned long long mine = __ballot(b.key == best);
    const int wl = __ffsll((long long)mine) - 1;
    GcBest w;
    w.key = mine ? best : ~0ull;
    w.slot = GCU(__shfl(b.slot, wl)); w.cell = GCU(__shfl(b.cell, wl)); w.first = GCU(__shfl(b.first, wl)); w.count = GCU(__shfl(b.count, wl));
    return w;
}

// ------------------------------------------------------------------------------------------------ 2. one list, first points only
// hdr and ent change under the chain (lane 0 removes the winner of every step); `se` does not
__global__ __launch_bounds__(64) void k_gc_chain(const int4* __restrict__ se, int n, int2* hdr, int4* ent, GcGrid g, int* __restrict__ order) {
    const int lane = threadIdx.x;
    int cx = 0, cy = 0;
    for (int step = 0; step < n; step++) {
        const GcBest w = gc_search<false>(g, 0, cx, cy, hdr, ent, nullptr);
        const int id = GCU((unsigned)w.key), win = id >> 1;
        if (id < 0 || win >= n) { if (lane == 0) order[0] = -1; return; }                    // cannot happen: n - step paths remain somewhere in the grid
        // the cell's last live entry takes the winner's place
        const int4 last = ent[w.first + w.count - 1];
        const int4 e = se[win];
        if (lane == 0) { ent[w.slot] = last; hdr[w.cell] = make_int2(w.first, w.count - 1); order[step] = win; }
        __threadfence_block();
        cx = GCU(e.z); cy = GCU(e.w);
    }
}

// ------------------------------------------------------------------------------------------------ 2b. order by pen group, strokes reversible
// The same walk, group after group with the cursor carried over: gc_search on the cells of the current group.  hdr, ent and slot change under the chain;
// `se` and the groups do not.  With `rev` the winner's other end leaves too: lane 0 does both removals one after the other in program order, so the second
// one reads the slot table and the cell header as the first one left them (both ends in one cell; the other end being the entry that has just been moved
// into the winner's place; a closed path, whose forward end wins).
__global__ __launch_bounds__(64) void k_op_chain(const int4* __restrict__ se, int n, const OpGroup* __restrict__ groups, int n_groups, int rev, int sx, int sy, int ncell, int m,
                                                 int2* hdr, int4* ent, int* slot, int* __restrict__ order, uint8_t* __restrict__ rev_out) {
    const int lane = threadIdx.x;
    int cx = sx, cy = sy, k = 0;
    for (int gi = 0; gi < n_groups; gi++) {
        const GcGrid g = groups[gi].g;
        const int cell0 = groups[gi].cell0, paths = groups[gi].paths;
        for (int step = 0; step < paths; step++, k++) {
            const GcBest w = gc_search<false>(g, cell0, cx, cy, hdr, ent, nullptr);
            const int id = GCU((unsigned)w.key), win = id >> 1, wr = id & 1;
            // cannot happen: paths - step paths of the group remain somewhere in its cells.  Every index below is checked before it is used all the same
            if (id < 0 || win >= n || (wr && !rev)) { if (lane == 0) order[0] = -1; return; }
            const int4 last = ent[w.first + w.count - 1];
            const int4 e = se[win];
            int lost = 0;
            if (lane == 0) {
                ent[w.slot] = last; hdr[w.cell] = make_int2(w.first, w.count - 1); order[k] = win; rev_out[k] = (uint8_t)wr;
                if (rev) {
                    if ((unsigned)last.z < 2u * (unsigned)n) slot[last.z] = w.slot; else lost = 1;
                    const int pc = cell0 + gc_cell(g, wr ? e.x : e.z, wr ? e.y : e.w);       // the other end's cell, from its coordinates
                    if (!lost && pc >= 0 && pc < ncell) {
                        const int ps = slot[id ^ 1];                                         // read behind the first removal, in this lane's program order
                        const int2 ph = hdr[pc];
                        if (ph.y > 0 && ps >= ph.x && ps < ph.x + ph.y && ph.x + ph.y <= m) {
                            const int4 l2 = ent[ph.x + ph.y - 1];
                            if ((unsigned)l2.z < 2u * (unsigned)n) { ent[ps] = l2; slot[l2.z] = ps; hdr[pc] = make_int2(ph.x, ph.y - 1); } else lost = 1;
                        } else lost = 1;
                    } else lost = 1;
                }
            }
            __threadfence_block();
            if (__shfl(lost, 0)) { if (lane == 0) order[0] = -1; return; }
            cx = GCU(wr ? e.x : e.z); cy = GCU(wr ? e.y : e.w);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 2c. the ring order: a closed stroke is entered at any ring vertex
// orip_gcode_order_rings (ours; include/orip.h states the rule).  The walk of 2b over CANDIDATES: every ring vertex of a closed stroke, the first point of an
// open one and, under ORIP_ORDER_REVERSE, its last.  Candidate c of stroke i has the id cbase[i] + c (a scan of the per-stroke counts), so ids ascend with
// (i, c) and the key (L1 distance << 32) | id is the rule's (d, i, c).  The grid is built over the candidates, per group as in gc_grids.
// When a stroke wins, ALL its candidates leave -- the 63 other vertices of a circle as well as the one entered.  Swap-removal, which 2 and 2b use, would be a
// chain of dependent read-modify-writes by one lane per vertex (a moved entry may be the next one to leave).  Here entries never move: slot[id] = (entry,
// cell) is fixed at fill time, the lanes mark the winner's entries dead 64 at a time (id = -1: one independent store each) and decrement the cell's live count
// by an atomic; the search passes over a dead entry and over a cell without a live one.  The cost is that a cell keeps its dead entries to the end: with
// about two candidates per cell that is a few wasted words per window.  A stroke is closed iff it has three candidates or more (L - 1 >= 3; an open one has
// one or two).
struct RoCounters { unsigned long long closed, moved, travel; };
#ifndef RO_CELL_CANDS
#define RO_CELL_CANDS 2                          // candidates per cell the grid aims at; make EXTRA=-DRO_CELL_CANDS=... builds another one for tools/time_ring_entry.py
#endif

// thread per stroke: its ends and how many candidates it has, which its group counts too
__global__ __launch_bounds__(256) void k_ro_strokes(const long long* __restrict__ off, const int2* __restrict__ pts, const int* __restrict__ grp, int n, int rev,
                                                    int4* __restrict__ se, int* __restrict__ cnt, unsigned long long* __restrict__ gcand) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long a = off[i], b = off[i + 1];
    const int2 A = pts[a], B = pts[b - 1];
    const int k = (b - a >= 4 && A.x == B.x && A.y == B.y) ? (int)(b - a - 1) : 1 + rev;
    se[i] = make_int4(A.x, A.y, B.x, B.y);
    cnt[i] = k;
    if (i == 0) cnt[n] = 0;
    atomicAdd(&gcand[grp ? grp[i] : 0], (unsigned long long)k);
}
// thread per candidate id: its stroke (the last i with cbase[i] <= id; every stroke has a candidate), its point, cd[id] = (x, y, stroke, group), the group's box
__global__ __launch_bounds__(256) void k_ro_cands(const long long* __restrict__ off, const int2* __restrict__ pts, const int* __restrict__ grp, const int* __restrict__ cbase, int n,
                                                  int4* __restrict__ cd, int* __restrict__ box) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    const bool ok = id < cbase[n];
    int g = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
    if (ok) {
        int lo = 0, hi = n;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (cbase[mid] <= id) lo = mid; else hi = mid; }
        const int i = lo, c = id - cbase[i], k = cbase[i + 1] - cbase[i];
        const int2 p = k >= 3 ? pts[off[i] + c] : pts[c ? off[i + 1] - 1 : off[i]];
        g = grp ? grp[i] : 0;
        cd[id] = make_int4(p.x, p.y, i, g);
        x0 = x1 = p.x; y0 = y1 = p.y;
    }
    // a ring's vertices are 64 neighbours of one group: one box update per wave then, not one per candidate
    const unsigned long long act = __ballot(ok);
    if (!act) return;
    const int g0 = __shfl(g, __ffsll((long long)act) - 1);
    if (__all(!ok || g == g0)) {
        for (int o = 32; o; o >>= 1) { x0 = min(x0, __shfl_xor(x0, o)); y0 = min(y0, __shfl_xor(y0, o)); x1 = max(x1, __shfl_xor(x1, o)); y1 = max(y1, __shfl_xor(y1, o)); }
        if ((threadIdx.x & 63) != 0) return;
        g = g0;
    } else if (!ok) return;
    int* b = box + 4 * g;
    atomicMin(&b[0], x0); atomicMin(&b[1], y0); atomicMax(&b[2], x1); atomicMax(&b[3], y1);
}
__global__ __launch_bounds__(256) void k_ro_cells(const int4* __restrict__ cd, int m, const OpGroup* __restrict__ G, unsigned* __restrict__ cnt) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= m) return;
    const int4 q = cd[id];
    const OpGroup o = G[q.w];
    atomicAdd(&cnt[o.cell0 + gc_cell(o.g, q.x, q.y)], 1u);
}
__global__ __launch_bounds__(256) void k_ro_fill(const int4* __restrict__ cd, int m, const OpGroup* __restrict__ G, const unsigned* __restrict__ start, unsigned* __restrict__ fill,
                                                 int4* __restrict__ ent, int2* __restrict__ slot) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= m) return;
    const int4 q = cd[id];
    const OpGroup o = G[q.w];
    const int c = o.cell0 + gc_cell(o.g, q.x, q.y);
    const int at = (int)(start[c] + atomicAdd(&fill[c], 1u));
    ent[at] = make_int4(q.x, q.y, id, q.z);
    slot[id] = make_int2(at, c);
}

// One wave, group after group with the cursor carried over.  ent and live change under the chain: every lane's stores and atomics of a step are behind
// the fence when the next search reads (the pattern of k_op_chain, whose lane 0 writes what all lanes read next; those pointers stay unqualified).  hdr,
// slot, se and cbase do not change.  Every index read from memory is checked before it is used.
__global__ __launch_bounds__(64) void k_ro_chain(const int4* __restrict__ se, const int* __restrict__ cbase, int n, const OpGroup* __restrict__ groups, int n_groups, int sx, int sy,
                                                 int ncell, int m, const int2* hdr, int4* ent, const int2* slot, int* live, int* __restrict__ order, uint8_t* __restrict__ rev_out,
                                                 int* __restrict__ seam, RoCounters* __restrict__ out) {
    const int lane = threadIdx.x;
    int cx = sx, cy = sy, k = 0;
    unsigned long long travel = 0, closed = 0, moved = 0;
    for (int gi = 0; gi < n_groups; gi++) {
        const GcGrid g = groups[gi].g;
        const int cell0 = groups[gi].cell0, paths = groups[gi].paths;
        for (int step = 0; step < paths; step++, k++) {
            const GcBest w = gc_search<true>(g, cell0, cx, cy, hdr, ent, live);
            const int id = GCU((unsigned)w.key), i = w.first, ex = w.cell, ey = w.count;     // DEAD: the entry's own words (gc_look)
            // cannot happen: paths - step strokes of the group have live candidates in its cells
            if (w.key == ~0ull || id < 0 || id >= m || i < 0 || i >= n || k >= n) { if (lane == 0) order[0] = -1; return; }
            const int cb = GCU(cbase[i]), kc = GCU(cbase[i + 1]) - cb, c = id - cb;
            const int4 e = se[i];
            if (c < 0 || c >= kc) { if (lane == 0) order[0] = -1; return; }
            const bool ring = kc >= 3;
            int lost = 0;
            for (int j = lane; j < kc; j += 64) {                                            // all candidates of the stroke leave
                const int2 s = slot[cb + j];
                if ((unsigned)s.x < (unsigned)m && (unsigned)s.y < (unsigned)ncell) { ent[s.x].z = -1; atomicSub(&live[s.y], 1); }
                else lost = 1;
            }
            travel += (unsigned long long)max(abs(ex - cx), abs(ey - cy));
            closed += ring; moved += ring && c != 0;
            if (lane == 0) { order[k] = i; rev_out[k] = (uint8_t)(ring ? 0 : c); seam[k] = ring ? c : 0; }
            __threadfence_block();
            if (__any(lost)) { if (lane == 0) order[0] = -1; return; }
            cx = GCU(ring ? ex : (c ? e.x : e.z)); cy = GCU(ring ? ey : (c ? e.y : e.w));    // a ring: the vertex entered; an open stroke: its other end
        }
    }
    if (lane == 0) { out->closed = closed; out->moved = moved; out->travel = travel; }
}

// ------------------------------------------------------------------------------------------------ host: ends and grids, the same for both orders
// square cells, a power of two wide: the smallest for which the grid over box b has at most cand / 2 cells (one cell at least), each side at most 2^15
GcGrid gc_grid_for(const int* b, int64_t cand) {
    GcGrid g{b[0], b[1], b[2], b[3], 0, 1, 1};
    const int64_t wx = (int64_t)b[2] - b[0], wy = (int64_t)b[3] - b[1], want = std::max<int64_t>(1, cand / 2);
    for (g.sh = 0;; g.sh++) {
        g.gx = (int)(wx >> g.sh) + 1; g.gy = (int)(wy >> g.sh) + 1;
        if (g.gx <= (1 << 15) && g.gy <= (1 << 15) && (int64_t)g.gx * g.gy <= want) break;
    }
    return g;
}

struct GcOrder { int4* se; int* order; uint8_t* rv; OpGroup* dG; int2* hdr; int4* ent; int* slot; int ncell; OpGroup hG[ORIP_ORDER_MAX_GROUPS]; };
// Checks and uploads the ends (NULL: the resident step polylines), boxes every group's candidates, chooses the grids and fills them: everything in front of
// the chain, enqueued on the lane's stream.  group == NULL: one group of all n paths, no group array on the device.  paths[g] = paths of group g.  Nothing
// is launched before the ends are known to be good.  The layout of c->gc_ends and c->gc_grid is stated in orip_ctx.h.
int gc_grids(orip_ctx* c, const char* who, const int32_t* ends, const int32_t* group, int64_t n, int G, int rev, const int64_t* paths, GcOrder& o) {
    if (ends)
        for (int64_t i = 0; i < 4 * n; i++) if (ends[i] < 0 || ends[i] > GC_COORD_MAX) ORIP_FAIL_AS(c, who, "path %lld: coordinate %d outside 0..2^30", (long long)(i / 4), ends[i]);
    const int64_t m = n << rev;                                             // candidates
    hipStream_t s = LN(c).stream;
    int *grp, *box;
    { Carve L; L.take(o.se, (size_t)n); L.take(grp, group ? (size_t)n : 0); L.take(o.order, (size_t)n); L.take(o.rv, group ? (size_t)n : 0); L.take(box, (size_t)4 * G);
      L.take(o.dG, (size_t)G); HIPC(c, L.commit(c->gc_ends, 64)); }
    if (ends) HIPC(c, hipMemcpyAsync(o.se, ends, (size_t)n * 16, hipMemcpyHostToDevice, s));
    else hipLaunchKernelGGL(k_gc_ends, dim3(cdiv(n, 256)), dim3(256), 0, s, c->gc_off.as<long long>(), c->gc_pts.as<int2>(), n, o.se);
    if (group) HIPC(c, hipMemcpyAsync(grp, group, (size_t)n * 4, hipMemcpyHostToDevice, s)); else grp = nullptr;
    int hbox[4 * ORIP_ORDER_MAX_GROUPS];
    for (int g = 0; g < G; g++) { hbox[4 * g] = hbox[4 * g + 1] = INT_MAX; hbox[4 * g + 2] = hbox[4 * g + 3] = INT_MIN; }
    HIPC(c, hipMemcpyAsync(box, hbox, (size_t)16 * G, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_op_bbox, dim3(cdiv(m, 256)), dim3(256), 0, s, o.se, grp, (int)m, rev, box);
    HIPC(c, hipMemcpyAsync(hbox, box, (size_t)16 * G, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    int64_t ncell = 0;
    for (int g = 0; g < G; g++) {
        OpGroup& q = o.hG[g];
        q.g = GcGrid{0, 0, 0, 0, 0, 1, 1}; q.cell0 = (int)ncell; q.paths = (int)paths[g];
        if (!paths[g]) continue;                                              // an empty group: no cells, no steps
        const int* b = hbox + 4 * g;
        if (b[0] < 0 || b[1] < 0 || b[2] > GC_COORD_MAX || b[3] > GC_COORD_MAX || b[0] > b[2] || b[1] > b[3]) {
            if (group) ORIP_FAIL_AS(c, who, "bounding box of group %d is off", g);
            ORIP_FAIL_AS(c, who, "bounding box of the first points is off");
        }
        q.g = gc_grid_for(b, paths[g] << rev);
        ncell += (int64_t)q.g.gx * q.g.gy;                                    // at most m / 2 + G over all groups
    }
    o.ncell = (int)ncell;
    unsigned *cnt, *start, *fill;
    { Carve L; L.take(cnt, (size_t)ncell + 1); L.take(start, (size_t)ncell + 1); L.take(fill, (size_t)ncell); L.take(o.hdr, (size_t)ncell); L.take(o.ent, (size_t)m);
      L.take(o.slot, rev ? (size_t)m : 0); HIPC(c, L.commit(c->gc_grid, 64)); }
    HIPC(c, hipMemcpyAsync(o.dG, o.hG, sizeof(OpGroup) * G, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(cnt, 0, ((size_t)ncell + 1) * 4, s));
    HIPC(c, hipMemsetAsync(fill, 0, (size_t)ncell * 4, s));
    hipLaunchKernelGGL(k_op_count, dim3(cdiv(m, 256)), dim3(256), 0, s, o.se, grp, (int)m, rev, o.dG, cnt);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, cnt, start, 0u, (size_t)ncell + 1, rocprim::plus<unsigned>(), s); }));
    hipLaunchKernelGGL(k_op_fill, dim3(cdiv(m, 256)), dim3(256), 0, s, o.se, grp, (int)m, rev, o.dG, start, fill, o.ent, o.slot);
    hipLaunchKernelGGL(k_gc_hdr, dim3(cdiv(ncell, 256)), dim3(256), 0, s, start, cnt, (int)ncell, o.hdr);
    return 0;
}
}  // namespace

// order[k] = index of the k-th path to draw.  ends: (first x, first y, last x, last y) per path, or NULL for the resident step polylines.
extern "C" int orip_gcode_order(orip_ctx* c, const int32_t* ends, int64_t n, int32_t* order_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (n < 0 || (n > 0 && !order_out)) ORIP_FAIL(c, "bad arguments");
    if (n == 0) return 0;
    if (!ends) ORIP_TRY(gc_check_resident(c, __func__, n));
    if (n > (1 << 27)) ORIP_FAIL(c, "%lld paths: at most 2^27", (long long)n);
    GcOrder o;
    ORIP_TRY(gc_grids(c, __func__, ends, nullptr, n, 1, 0, &n, o));
    hipStream_t s = LN(c).stream;
    { ProfScope ps(c, "k_gc_chain");
      hipLaunchKernelGGL(k_gc_chain, dim3(1), dim3(64), 0, s, o.se, (int)n, o.hdr, o.ent, o.hG[0].g, o.order); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(order_out, o.order, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (order_out[0] < 0) ORIP_FAIL(c, "the chain lost a path (internal error)");
    return 0;
}

// group after group from start_xy, inside a group the nearest remaining end (first points only without ORIP_ORDER_REVERSE); include/orip.h states the rule
extern "C" int orip_gcode_order_pens(orip_ctx* c, const int32_t* ends, const int32_t* group, int64_t n, int32_t n_groups, int32_t flags, const int32_t* start_xy,
                                     int32_t* order_out, uint8_t* rev_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (n < 0 || (n > 0 && (!group || !order_out || !rev_out)) || (flags & ~ORIP_ORDER_REVERSE)) ORIP_FAIL(c, "bad arguments");
    int sx, sy;
    ORIP_TRY(gc_check_groups(c, __func__, nullptr, 0, n_groups, nullptr));
    ORIP_TRY(gc_check_start(c, __func__, start_xy, sx, sy));
    if (n == 0) return 0;
    if (!ends) ORIP_TRY(gc_check_resident(c, __func__, n));
    if (n > (1 << 26)) ORIP_FAIL(c, "%lld paths: at most 2^26", (long long)n);
    int64_t paths[ORIP_ORDER_MAX_GROUPS] = {0};
    ORIP_TRY(gc_check_groups(c, __func__, group, n, n_groups, paths));
    const int rev = flags & ORIP_ORDER_REVERSE ? 1 : 0;
    GcOrder o;
    ORIP_TRY(gc_grids(c, __func__, ends, group, n, n_groups, rev, paths, o));
    hipStream_t s = LN(c).stream;
    { ProfScope ps(c, "k_op_chain");
      hipLaunchKernelGGL(k_op_chain, dim3(1), dim3(64), 0, s, o.se, (int)n, o.dG, (int)n_groups, rev, sx, sy, o.ncell, (int)(n << rev), o.hdr, o.ent, o.slot, o.order, o.rv); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(order_out, o.order, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(rev_out, o.rv, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (order_out[0] < 0) ORIP_FAIL(c, "the chain lost a path (internal error)");
    return 0;
}

// the walk over candidates, a closed stroke entered at its nearest ring vertex; include/orip.h states the rule, 2c above the kernels
extern "C" int orip_gcode_order_rings(orip_ctx* c, const int64_t* off, const int32_t* pts, const int32_t* group, int64_t n, int32_t n_groups, int32_t flags,
                                      const int32_t* start_xy, int32_t* order_out, uint8_t* rev_out, int32_t* seam_out, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats || (n > 0 && (!order_out || !rev_out || !seam_out)) || (flags & ~ORIP_ORDER_REVERSE)) ORIP_FAIL(c, "bad arguments");
    if (n < 0 || n > (1 << 26)) ORIP_FAIL(c, "%lld paths: 0..2^26", (long long)n);
    int sx, sy;
    ORIP_TRY(gc_check_groups(c, __func__, nullptr, 0, n_groups, nullptr));
    ORIP_TRY(gc_check_start(c, __func__, start_xy, sx, sy));
    if (n == 0) { for (int k = 0; k < 4; k++) stats[k] = 0; return 0; }
    if (!off != !pts) ORIP_FAIL(c, "off and pts: both or neither");
    int64_t total;
    if (off) {                                                                // one-point strokes are legal here (the dots of a stipple), so not gc_steps_check
        if (off[0] != 0) ORIP_FAIL(c, "offsets must start at 0");
        for (int64_t p = 0; p < n; p++) if (off[p + 1] - off[p] < 1) ORIP_FAIL(c, "path %lld has no point", (long long)p);
        total = off[n];
    } else {
        ORIP_TRY(gc_check_resident(c, __func__, n));
        total = c->gc_total;
    }
    if (total >= (int64_t)1 << 28) ORIP_FAIL(c, "%lld points: fewer than 2^28", (long long)total);
    for (int64_t i = 0; off && i < 2 * total; i++) if (pts[i] < 0 || pts[i] > GC_COORD_MAX) ORIP_FAIL(c, "point %lld: coordinate %d outside 0..2^30", (long long)(i / 2), pts[i]);
    int64_t paths[ORIP_ORDER_MAX_GROUPS] = {0};
    ORIP_TRY(gc_check_groups(c, __func__, group, n, n_groups, paths));
    if (!group) paths[0] = n;
    const int rev = flags & ORIP_ORDER_REVERSE ? 1 : 0, G = n_groups, N = (int)n;
    const int64_t ub = total + n;                                             // candidates at most: known before the scan is read back
    hipStream_t s = LN(c).stream;
    const long long* d_off = c->gc_off.as<long long>(); const int2* d_pts = c->gc_pts.as<int2>();
    if (off) {
        long long* o2; int2* p2;
        { Carve L; L.take(o2, (size_t)n + 1); L.take(p2, (size_t)total); HIPC(c, L.commit(c->ro_in, 64)); }
        HIPC(c, hipMemcpyAsync(o2, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        HIPC(c, hipMemcpyAsync(p2, pts, (size_t)total * 8, hipMemcpyHostToDevice, s));
        d_off = o2; d_pts = p2;
    }
    int4 *se, *cd; int *grp, *cnt, *cbase, *order, *seam, *box; uint8_t* rv; unsigned long long* gcand; OpGroup* dG; RoCounters* rc;
    { Carve L; L.take(se, (size_t)n); L.take(grp, group ? (size_t)n : 0); L.take(cnt, (size_t)n + 1); L.take(cbase, (size_t)n + 1); L.take(order, (size_t)n); L.take(seam, (size_t)n);
      L.take(rv, (size_t)n); L.take(box, (size_t)4 * G); L.take(gcand, (size_t)G); L.take(dG, (size_t)G); L.take(rc, 1); L.take(cd, (size_t)ub); HIPC(c, L.commit(c->ro_state, 64)); }
    if (group) HIPC(c, hipMemcpyAsync(grp, group, (size_t)n * 4, hipMemcpyHostToDevice, s)); else grp = nullptr;
    int hbox[4 * ORIP_ORDER_MAX_GROUPS]; unsigned long long hcand[ORIP_ORDER_MAX_GROUPS]; int m32 = 0;
    for (int g = 0; g < G; g++) { hbox[4 * g] = hbox[4 * g + 1] = INT_MAX; hbox[4 * g + 2] = hbox[4 * g + 3] = INT_MIN; }
    HIPC(c, hipMemcpyAsync(box, hbox, (size_t)16 * G, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(gcand, 0, (size_t)8 * G, s));
    HIPC(c, hipMemsetAsync(rc, 0, sizeof(RoCounters), s));
    hipLaunchKernelGGL(k_ro_strokes, dim3(cdiv(n, 256)), dim3(256), 0, s, d_off, d_pts, grp, N, rev, se, cnt, gcand);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, cnt, cbase, 0, (size_t)n + 1, rocprim::plus<int>(), s); }));
    hipLaunchKernelGGL(k_ro_cands, dim3(cdiv(ub, 256)), dim3(256), 0, s, d_off, d_pts, grp, cbase, N, cd, box);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(hbox, box, (size_t)16 * G, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(hcand, gcand, (size_t)8 * G, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&m32, cbase + n, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    const int64_t m = m32;
    int64_t ncell = 0, msum = 0;
    OpGroup hG[ORIP_ORDER_MAX_GROUPS];
    for (int g = 0; g < G; g++) {
        OpGroup& q = hG[g];
        q.g = GcGrid{0, 0, 0, 0, 0, 1, 1}; q.cell0 = (int)ncell; q.paths = (int)paths[g];
        msum += (int64_t)hcand[g];
        if (!paths[g]) { if (hcand[g]) ORIP_FAIL(c, "the candidates do not add up (internal error)"); continue; }
        const int* b = hbox + 4 * g;
        if (b[0] < 0 || b[1] < 0 || b[2] > GC_COORD_MAX || b[3] > GC_COORD_MAX || b[0] > b[2] || b[1] > b[3] || (int64_t)hcand[g] < paths[g])
            ORIP_FAIL(c, "bounding box or candidates of group %d are off (internal error)", g);
        q.g = gc_grid_for(b, (int64_t)hcand[g] * 2 / RO_CELL_CANDS);      // gc_grid_for aims at two per cell
        ncell += (int64_t)q.g.gx * q.g.gy;                                    // at most m / 2 + G over all groups
    }
    if (m < n || m > ub || msum != m) ORIP_FAIL(c, "the candidates do not add up (internal error)");
    unsigned *ccnt, *start, *fill; int2 *hdr, *slot; int4* ent;
    { Carve L; L.take(ccnt, (size_t)ncell + 1); L.take(start, (size_t)ncell + 1); L.take(fill, (size_t)ncell); L.take(hdr, (size_t)ncell); L.take(ent, (size_t)m);
      L.take(slot, (size_t)m); HIPC(c, L.commit(c->ro_grid, 64)); }
    HIPC(c, hipMemcpyAsync(dG, hG, sizeof(OpGroup) * G, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(ccnt, 0, ((size_t)ncell + 1) * 4, s));
    HIPC(c, hipMemsetAsync(fill, 0, (size_t)ncell * 4, s));
    hipLaunchKernelGGL(k_ro_cells, dim3(cdiv(m, 256)), dim3(256), 0, s, cd, (int)m, dG, ccnt);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, ccnt, start, 0u, (size_t)ncell + 1, rocprim::plus<unsigned>(), s); }));
    hipLaunchKernelGGL(k_ro_fill, dim3(cdiv(m, 256)), dim3(256), 0, s, cd, (int)m, dG, start, fill, ent, slot);
    hipLaunchKernelGGL(k_gc_hdr, dim3(cdiv(ncell, 256)), dim3(256), 0, s, start, ccnt, (int)ncell, hdr);
    { ProfScope ps(c, "k_ro_chain");
      hipLaunchKernelGGL(k_ro_chain, dim3(1), dim3(64), 0, s, se, cbase, N, dG, G, sx, sy, (int)ncell, (int)m, hdr, ent, slot, (int*)ccnt, order, rv, seam, rc); }
    HIPC(c, hipGetLastError());
    std::vector<int32_t> ho((size_t)n), hs((size_t)n); std::vector<uint8_t> hr((size_t)n); RoCounters hc;
    HIPC(c, hipMemcpyAsync(ho.data(), order, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(hs.data(), seam, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(hr.data(), rv, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&hc, rc, sizeof hc, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (ho[0] < 0) ORIP_FAIL(c, "the chain lost a path (internal error)");
    if (hc.moved > hc.closed || hc.closed > (unsigned long long)n) ORIP_FAIL(c, "the counts do not add up (internal error)");
    memcpy(order_out, ho.data(), (size_t)n * 4); memcpy(seam_out, hs.data(), (size_t)n * 4); memcpy(rev_out, hr.data(), (size_t)n);
    stats[0] = (int64_t)hc.closed; stats[1] = (int64_t)hc.moved; stats[2] = m; stats[3] = (int64_t)hc.travel;
    return 0;
}
