// csrc/gcode.hip -- the device side of svg_to_stream/gcode2stream.py: pen-down paths in mm -> step polylines (convert_polylines_to_steps :305-341 with
// mm_to_steps :79-110), the nearest-neighbour order of the paths (order_paths_nearest :151-172) and the bytes of the finished stream
// (StreamWriter.add_steps / finalize, shared/omnirevolve_plotter_stream_creator_helper.py :55-68, :166-175).  Parsing and the speed plan stay on the host.
//
// 1. Paths to steps.  One thread per point: (v * scale + offset) * steps_per_mm in IEEE double, the three operations kept apart (_rn intrinsics, and the
//    tree builds with -ffp-contract=off), (H - 1) - y under invert_y, round half to even, clamp to the sheet.  A point is kept when its step position differs
//    from its predecessor's (the reference compares with the last point it appended, which is always the predecessor's position).  A scan compacts the
//    points, a second one drops the paths left with fewer than two.  A non-finite coordinate in a path of two or more points is an error, as it is for the
//    reference (int(round(inf)) raises).
//
// 2. Order.  The reference starts at (0, 0) and takes, again and again, the remaining path whose FIRST point has the smallest L1 distance from the cursor,
//    the lowest index on ties; the cursor moves to that path's LAST point.  That is a chain of n dependent searches over n points: n^2 / 2 distances.  Here
//    the first points are bucketed into a grid of square cells (a power of two wide, about two points per cell, 16 bytes per point: x, y, index), in global
//    memory, where the grid of a 10^6-path plot (16 MB + 8 bytes per cell) stays in L2.  ONE wave walks the chain; its lanes do the search of a step:
//      * the window starts as the 3 x 3 cells around the cursor's cell and grows by one ring of cells at a time; four lanes share a cell (entries j, j + 4,
//        ...), so a pass looks at 16 cells; a cell of more than GC_BIG entries is scanned by all 64 lanes instead (thousands of paths that start on
//        one point are one such cell);
//      * the key of an entry is (L1 distance << 32) | index, the search takes the minimum: exactly the reference's `d < best_d` over a list in index order;
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
// 3. Pack.  The host plans the pieces (first code, step count, byte position, speed byte or none) and the service bytes; one thread per output byte finds
//    its piece by binary search over the byte positions and writes the speed byte or the step byte (two codes per byte, paired inside the piece; the last
//    byte of an odd piece holds one), or zero; a second kernel drops the service bytes (the end byte among them) in.  The direction codes are the resident
//    result of orip_stream_codes and never leave the device.
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>
#include <climits>

namespace {
constexpr int GC_COORD_MAX = 1 << 30;
constexpr int GC_BIG = 64;                       // a cell with more entries than this is scanned by the whole wave

// ------------------------------------------------------------------------------------------------ 1. paths to steps
__device__ __forceinline__ bool gc_step(const orip_gcode_map& g, double xm, double ym, int2& o) {
    double xf, yf;
    o = make_int2(0, 0);
    if (!gc_round_mm(g, xm, ym, xf, yf)) return false;                // gc_convert.h: the arithmetic and Python's round(), shared with gcode_clip.hip
    const double xmax = (double)(g.W - 1), ymax = (double)(g.H - 1);
    xf = xf < 0.0 ? 0.0 : (xf > xmax ? xmax : xf);
    yf = yf < 0.0 ? 0.0 : (yf > ymax ? ymax : yf);
    o = make_int2((int)xf, (int)yf);
    return true;
}

__global__ __launch_bounds__(256) void k_gc_points(const long long* __restrict__ off, int64_t n, const double2* __restrict__ mm, int64_t total, orip_gcode_map g,
                                                   int2* __restrict__ xy, unsigned* __restrict__ keep, unsigned* __restrict__ pid, int* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > total) return;
    if (i == total) { keep[i] = 0; return; }
    const int64_t p = gc_path_of(off, n, i);
    const bool first = i == off[p];
    const double2 a = mm[i];
    int2 me, pv;
    bool ok = gc_step(g, a.x, a.y, me), k = true;
    if (!first) { const double2 b = mm[i - 1]; ok = gc_step(g, b.x, b.y, pv) && ok; k = pv.x != me.x || pv.y != me.y; }
    if (!ok && off[p + 1] - off[p] >= 2) atomicOr(err, 1);
    xy[i] = me; keep[i] = k ? 1u : 0u; pid[i] = (unsigned)p;
}

__global__ __launch_bounds__(256) void k_gc_paths(const long long* __restrict__ off, int64_t n, const unsigned* __restrict__ kpos, unsigned* __restrict__ pc,
                                                  unsigned* __restrict__ pk) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    unsigned cnt = 0;
    if (p < n) cnt = kpos[off[p + 1]] - kpos[off[p]];
    pc[p] = cnt >= 2 ? cnt : 0u; pk[p] = cnt >= 2 ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_gc_emit(const long long* __restrict__ off, int64_t n, int64_t total, const int2* __restrict__ xy, const unsigned* __restrict__ keep,
                                                 const unsigned* __restrict__ pid, const unsigned* __restrict__ kpos, const unsigned* __restrict__ pk,
                                                 const unsigned* __restrict__ noff, const unsigned* __restrict__ nidx, int2* __restrict__ out_pts, long long* __restrict__ out_off, int* __restrict__ out_src) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) {                                                       // offsets of the kept paths and the closing one; where each kept path came from
        if (i == n) out_off[nidx[n]] = (long long)noff[n];
        else if (pk[i]) { out_off[nidx[i]] = (long long)noff[i]; out_src[nidx[i]] = (int)i; }
    }
    if (i >= total || !keep[i]) return;
    const unsigned p = pid[i];
    if (pk[p]) out_pts[noff[p] + (kpos[i] - kpos[off[p]])] = xy[i];
}

// ------------------------------------------------------------------------------------------------ 2. order
struct GcGrid { int x0, y0, x1, y1, sh, gx, gy; };      // bounding box of the first points, log2 of the cell width, cells per side
__device__ __forceinline__ int gc_cell(const GcGrid& g, int x, int y) { return ((y - g.y0) >> g.sh) * g.gx + ((x - g.x0) >> g.sh); }

__global__ __launch_bounds__(256) void k_gc_ends(const long long* __restrict__ off, const int2* __restrict__ pts, int64_t n, int4* __restrict__ se) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int2 a = pts[off[p]], b = pts[off[p + 1] - 1];
    se[p] = make_int4(a.x, a.y, b.x, b.y);
}
__global__ __launch_bounds__(256) void k_gc_bbox(const int4* __restrict__ se, int n, int* __restrict__ box) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 e = se[i];
    atomicMin(&box[0], e.x); atomicMin(&box[1], e.y); atomicMax(&box[2], e.x); atomicMax(&box[3], e.y);
}
__global__ __launch_bounds__(256) void k_gc_count(const int4* __restrict__ se, int n, GcGrid g, unsigned* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[gc_cell(g, se[i].x, se[i].y)], 1u);
}
__global__ __launch_bounds__(256) void k_gc_fill(const int4* __restrict__ se, int n, GcGrid g, const unsigned* __restrict__ start, unsigned* __restrict__ fill,
                                                 int4* __restrict__ ent) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 e = se[i];
    const int c = gc_cell(g, e.x, e.y);
    ent[start[c] + atomicAdd(&fill[c], 1u)] = make_int4(e.x, e.y, i, 0);
}
__global__ __launch_bounds__(256) void k_gc_hdr(const unsigned* __restrict__ start, const unsigned* __restrict__ cnt, int ncell, int2* __restrict__ hdr) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < ncell) hdr[c] = make_int2((int)start[c], (int)cnt[c]);
}

// what a lane remembers about the best entry it has seen in the current step: its key, slot and cell, and the cell's header when it was read
struct GcBest { unsigned long long key; int slot, cell, first, count; };
__device__ __forceinline__ void gc_look(GcBest& b, const int4 e, int slot, int cell, const int2 h, int cx, int cy) {
    const unsigned d = (unsigned)abs(e.x - cx) + (unsigned)abs(e.y - cy);
    const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)e.z;
    if (key < b.key) { b.key = key; b.slot = slot; b.cell = cell; b.first = h.x; b.count = h.y; }
}
#define GCU(x) __builtin_amdgcn_readfirstlane((int)(x))

// hdr and ent change under the chain (lane 0 removes the winner of every step); `se` does not
__global__ __launch_bounds__(64) void k_gc_chain(const int4* __restrict__ se, int n, int2* hdr, int4* ent, GcGrid g, int* __restrict__ order) {
    __shared__ unsigned long long s_best;
    const int lane = threadIdx.x, sub = lane & 3, slot16 = lane >> 2;
    const long long INF = 1ll << 62;
    int cx = 0, cy = 0;
    for (int step = 0; step < n; step++) {
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
                    cell = y * g.gx + x;
                    h = hdr[cell];
                    if (h.y <= GC_BIG)
                        for (int j = sub; j < h.y; j += 4) gc_look(b, ent[h.x + j], h.x + j, cell, h, cx, cy);
                }
                unsigned long long big = __ballot(cell >= 0 && h.y > GC_BIG && sub == 0);
                while (big) {                                                  // wave-uniform loop: a crowded cell, all lanes on it
                    const int l = __ffsll((long long)big) - 1;
                    big &= big - 1;
                    const int bc = __shfl(cell, l), bx = __shfl(h.x, l), by = __shfl(h.y, l);
                    for (int j = lane; j < by; j += 64) gc_look(b, ent[bx + j], bx + j, bc, make_int2(bx, by), cx, cy);
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
            // the cursor's distance from the bounding box in the other one (every first point lies inside the box)
            long long bd = INF;
            if (xl > 0) bd = min(bd, (long long)cx - ((long long)g.x0 + ((long long)xl << g.sh)) + 1 + oy);
            if (yl > 0) bd = min(bd, (long long)cy - ((long long)g.y0 + ((long long)yl << g.sh)) + 1 + ox);
            if (xh < g.gx - 1) bd = min(bd, (long long)g.x0 + ((long long)(xh + 1) << g.sh) - (long long)cx + oy);
            if (yh < g.gy - 1) bd = min(bd, (long long)g.y0 + ((long long)(yh + 1) << g.sh) - (long long)cy + ox);
            if (bd == INF || (long long)(best >> 32) < bd) break;
        }
        // the winner's lane hands over where the entry sits; the cell's last live entry takes the place
        const unsigned long long mine = __ballot(b.key == best);
        const int wl = __ffsll((long long)mine) - 1;
        const int win = GCU((unsigned)best), wslot = GCU(__shfl(b.slot, wl)), wcell = GCU(__shfl(b.cell, wl)), wfirst = GCU(__shfl(b.first, wl)),
                  wcount = GCU(__shfl(b.count, wl));
        if (mine == 0 || win < 0 || win >= n) { if (lane == 0) order[0] = -1; return; }      // cannot happen: n - step paths remain somewhere in the grid
        const int4 last = ent[wfirst + wcount - 1];
        const int4 e = se[win];
        if (lane == 0) { ent[wslot] = last; hdr[wcell] = make_int2(wfirst, wcount - 1); order[step] = win; }
        __threadfence_block();
        cx = GCU(e.z); cy = GCU(e.w);
    }
}

// ------------------------------------------------------------------------------------------------ 2b. order by pen group, strokes reversible
// One grid per group, side by side in the same arrays: group g owns the cells cell0 .. cell0 + gx * gy - 1, and because the entries are laid out by one
// scan over all cells, its entries are one range too -- a search that stays inside its group's cells cannot see another group's candidate.
struct OpGroup { GcGrid g; int cell0, paths; };          // box and cells over the group's candidate points; how many paths it holds
// candidate t: path and end.  Without reversal the first points only (ids 2i), with it both ends (2i, 2i + 1)
__device__ __forceinline__ int op_cand(const int4* __restrict__ se, int t, int rev, int2& p) {
    const int i = rev ? t >> 1 : t, r = rev ? t & 1 : 0;
    const int4 e = se[i];
    p = r ? make_int2(e.z, e.w) : make_int2(e.x, e.y);
    return 2 * i + r;
}
__global__ __launch_bounds__(256) void k_op_bbox(const int4* __restrict__ se, const int* __restrict__ grp, int m, int rev, int* __restrict__ box) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    int2 p; const int id = op_cand(se, t, rev, p);
    int* b = box + 4 * grp[id >> 1];
    atomicMin(&b[0], p.x); atomicMin(&b[1], p.y); atomicMax(&b[2], p.x); atomicMax(&b[3], p.y);
}
__global__ __launch_bounds__(256) void k_op_count(const int4* __restrict__ se, const int* __restrict__ grp, int m, int rev, const OpGroup* __restrict__ G, unsigned* __restrict__ cnt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    int2 p; const int id = op_cand(se, t, rev, p);
    const OpGroup o = G[grp[id >> 1]];
    atomicAdd(&cnt[o.cell0 + gc_cell(o.g, p.x, p.y)], 1u);
}
__global__ __launch_bounds__(256) void k_op_fill(const int4* __restrict__ se, const int* __restrict__ grp, int m, int rev, const OpGroup* __restrict__ G, const unsigned* __restrict__ start,
                                                 unsigned* __restrict__ fill, int4* __restrict__ ent, int* __restrict__ slot) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    int2 p; const int id = op_cand(se, t, rev, p);
    const OpGroup o = G[grp[id >> 1]];
    const int c = o.cell0 + gc_cell(o.g, p.x, p.y);
    const int at = (int)(start[c] + atomicAdd(&fill[c], 1u));
    ent[at] = make_int4(p.x, p.y, id, 0);
    if (rev) slot[id] = at;                              // where candidate id sits: how a winner's other end is found without a search
}

// k_gc_chain's walk, group after group with the cursor carried over; the search of a step is the same code on the cells of the current group, the key's low
// word is the candidate id 2i + r.  hdr, ent and slot change under the chain; `se` and the groups do not.  With `rev` the winner's other end leaves too:
// lane 0 does both removals one after the other in program order, so the second one reads the slot table and the cell header as the first one left
// them (both ends in one cell; the other end being the entry that has just been moved into the winner's place; a closed path, whose forward end wins).
__global__ __launch_bounds__(64) void k_op_chain(const int4* __restrict__ se, int n, const OpGroup* __restrict__ groups, int n_groups, int rev, int sx, int sy, int ncell, int m,
                                                 int2* hdr, int4* ent, int* slot, int* __restrict__ order, uint8_t* __restrict__ rev_out) {
    __shared__ unsigned long long s_best;
    const int lane = threadIdx.x, sub = lane & 3, slot16 = lane >> 2;
    const long long INF = 1ll << 62;
    int cx = sx, cy = sy, k = 0;
    for (int gi = 0; gi < n_groups; gi++) {
        const GcGrid g = groups[gi].g;
        const int cell0 = groups[gi].cell0, paths = groups[gi].paths;
        for (int step = 0; step < paths; step++, k++) {
            const int ccx = min(max(cx - g.x0, 0) >> g.sh, g.gx - 1), ccy = min(max(cy - g.y0, 0) >> g.sh, g.gy - 1);
            const long long ox = max(max(g.x0 - cx, cx - g.x1), 0), oy = max(max(g.y0 - cy, cy - g.y1), 0);
            GcBest b; b.key = ~0ull; b.slot = b.cell = b.first = b.count = 0;
            unsigned long long best = ~0ull;
            for (int r = 1;; r++) {
                const int xl = ccx - r, xh = ccx + r, yl = ccy - r, yh = ccy + r;
                const int cxl = max(xl, 0), cxh = min(xh, g.gx - 1), cyl = max(yl, 0), cyh = min(yh, g.gy - 1);
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
                        if (h.y <= GC_BIG)
                            for (int j = sub; j < h.y; j += 4) gc_look(b, ent[h.x + j], h.x + j, cell, h, cx, cy);
                    }
                    unsigned long long big = __ballot(cell >= 0 && h.y > GC_BIG && sub == 0);
                    while (big) {                                              // wave-uniform loop: a crowded cell, all lanes on it
                        const int l = __ffsll((long long)big) - 1;
                        big &= big - 1;
                        const int bc = __shfl(cell, l), bx = __shfl(h.x, l), by = __shfl(h.y, l);
                        for (int j = lane; j < by; j += 64) gc_look(b, ent[bx + j], bx + j, bc, make_int2(bx, by), cx, cy);
                    }
                }
                if (lane == 0) s_best = ~0ull;
                __syncthreads();
                if (b.key != ~0ull) atomicMin(&s_best, b.key);
                __syncthreads();
                best = s_best;
                __syncthreads();
                // as in k_gc_chain: the way to each border that has cells behind it, plus the cursor's distance from the group's box in the other coordinate
                // (a group whose points all lie far from where the previous group ended is this term's case)
                long long bd = INF;
                if (xl > 0) bd = min(bd, (long long)cx - ((long long)g.x0 + ((long long)xl << g.sh)) + 1 + oy);
                if (yl > 0) bd = min(bd, (long long)cy - ((long long)g.y0 + ((long long)yl << g.sh)) + 1 + ox);
                if (xh < g.gx - 1) bd = min(bd, (long long)g.x0 + ((long long)(xh + 1) << g.sh) - (long long)cx + oy);
                if (yh < g.gy - 1) bd = min(bd, (long long)g.y0 + ((long long)(yh + 1) << g.sh) - (long long)cy + ox);
                if (bd == INF || (long long)(best >> 32) < bd) break;
            }
            const unsigned long long mine = __ballot(b.key == best);
            const int wl = __ffsll((long long)mine) - 1;
            const int id = GCU((unsigned)best), wslot = GCU(__shfl(b.slot, wl)), wcell = GCU(__shfl(b.cell, wl)), wfirst = GCU(__shfl(b.first, wl)), wcount = GCU(__shfl(b.count, wl));
            const int win = id >> 1, wr = id & 1;
            // cannot happen: paths - step paths of the group remain somewhere in its cells.  Every index below is checked before it is used all the same
            if (mine == 0 || id < 0 || win >= n || (wr && !rev)) { if (lane == 0) order[0] = -1; return; }
            const int4 last = ent[wfirst + wcount - 1];
            const int4 e = se[win];
            int lost = 0;
            if (lane == 0) {
                ent[wslot] = last; hdr[wcell] = make_int2(wfirst, wcount - 1); order[k] = win; rev_out[k] = (uint8_t)wr;
                if (rev) {
                    if ((unsigned)last.z < 2u * (unsigned)n) slot[last.z] = wslot; else lost = 1;
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

// ------------------------------------------------------------------------------------------------ 3. pack
__global__ __launch_bounds__(256) void k_pk_bytes(const long long* __restrict__ pos, const long long* __restrict__ code0, const int* __restrict__ cnt,
                                                  const int* __restrict__ speed, int64_t np, const uint8_t* __restrict__ codes, int64_t nbytes, uint8_t* __restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nbytes) return;
    unsigned v = 0;
    if (np > 0 && b >= pos[0]) {
        int64_t lo = 0, hi = np;                                             // last piece that starts at or before this byte
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (pos[mid] <= b) lo = mid; else hi = mid; }
        const int c = cnt[lo], sp = speed[lo];
        const int64_t j = b - pos[lo] - (sp >= 0 ? 1 : 0);                   // step byte j of the piece; -1: its speed byte
        if (j < 0) v = (unsigned)sp;
        else if (2 * j < c) {
            const uint8_t* q = codes + code0[lo] + 2 * j;
            const unsigned a = q[0] & 7u;
            v = 2 * j + 1 < c ? (0xC0u | (a << 3) | (q[1] & 7u)) : (0x80u | (a << 3));
        }
    }
    out[b] = (uint8_t)v;
}
__global__ __launch_bounds__(256) void k_pk_service(const long long* __restrict__ pos, const uint8_t* __restrict__ val, int64_t ns, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ns) out[pos[i]] = val[i];
}
}  // namespace

// mm paths -> resident step polylines; *n_out paths with *total_out points remain.  off == NULL and pts_mm == NULL: the n resident fitted paths of svg.hip
extern "C" int orip_gcode_to_steps(orip_ctx* c, const int64_t* off, const double* pts_mm, int64_t n, const orip_gcode_map* map, int64_t* n_out, int64_t* total_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    c->gc_n = 0; c->gc_total = 0; c->gc_ready = false; c->gc_merged = false;
    const bool resident = !off && !pts_mm && n > 0;         // the fitted paths orip_svg_flatten / orip_svg_fit left on the device (svg.hip)
    if (!map || !n_out || !total_out || n < 0 || (n > 0 && !off && !resident)) ORIP_FAIL(c, "bad arguments");
    *n_out = 0; *total_out = 0;
    if (resident && (!c->sv_ready || n != c->sv_n)) ORIP_FAIL(c, "%lld paths asked for, %lld fitted paths resident", (long long)n, (long long)(c->sv_ready ? c->sv_n : -1));
    if (map->W < 1 || map->H < 1 || map->W > GC_COORD_MAX || map->H > GC_COORD_MAX)
        ORIP_FAIL(c, "target size %d x %d steps: each side must be in 1..2^30 (step coordinates are int32 on the device)", map->W, map->H);
    const int64_t total = resident ? c->sv_total : n > 0 ? off[n] : 0;
    if (!resident) {
        if (n > 0 && off[0] != 0) ORIP_FAIL(c, "offsets must start at 0");
        for (int64_t p = 0; p < n; p++) if (off[p + 1] < off[p]) ORIP_FAIL(c, "offsets must not decrease (path %lld)", (long long)p);
    }
    if (n >= INT32_MAX / 2 || total >= INT32_MAX / 2) ORIP_FAIL(c, "%lld paths, %lld points: at most 2^30 of each", (long long)n, (long long)total);
    if (total > 0 && !pts_mm && !resident) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, c->gc_off.ensure(64)); HIPC(c, hipMemsetAsync(c->gc_off.p, 0, 8, s));
    if (total == 0) { HIPC(c, hipStreamSynchronize(s)); c->gc_ready = true; return 0; }
    long long* d_off; double2* d_mm; int2* xy; unsigned *keep, *kpos, *pid, *pc, *pk, *noff, *nidx; int* err;
    Carve L;
    L.take(d_off, resident ? 0 : (size_t)n + 1); L.take(d_mm, resident ? 0 : (size_t)total); L.take(xy, (size_t)total); L.take(keep, (size_t)total + 1); L.take(kpos, (size_t)total + 1);
    L.take(pid, (size_t)total); L.take(pc, (size_t)n + 1); L.take(pk, (size_t)n + 1); L.take(noff, (size_t)n + 1); L.take(nidx, (size_t)n + 1); L.take(err, 1);
    HIPC(c, L.commit(c->gc_tmp, 64));
    HIPC(c, c->gc_off.ensure((size_t)(n + 1) * 8 + 64)); HIPC(c, c->gc_pts.ensure((size_t)total * 8 + 64));     // the output is never larger than the input
    HIPC(c, c->gc_src.ensure((size_t)n * 4 + 64));
    HIPC(c, hipMemsetAsync(c->gc_off.p, 0, 8, s));
    if (resident) { d_off = c->sv_off.as<long long>(); d_mm = c->sv_pts.as<double2>(); }
    else {
        HIPC(c, hipMemcpyAsync(d_off, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        HIPC(c, hipMemcpyAsync(d_mm, pts_mm, (size_t)total * 16, hipMemcpyHostToDevice, s));
    }
    HIPC(c, hipMemsetAsync(err, 0, 4, s));
    { ProfScope ps(c, "k_gc_points");
      hipLaunchKernelGGL(k_gc_points, dim3(cdiv(total + 1, 256)), dim3(256), 0, s, d_off, n, d_mm, total, *map, xy, keep, pid, err); }
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, keep, kpos, 0u, (size_t)total + 1, rocprim::plus<unsigned>(), s); }));
    hipLaunchKernelGGL(k_gc_paths, dim3(cdiv(n + 1, 256)), dim3(256), 0, s, d_off, n, kpos, pc, pk);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, pc, noff, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), s); }));
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, pk, nidx, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), s); }));
    { ProfScope ps(c, "k_gc_emit");
      hipLaunchKernelGGL(k_gc_emit, dim3(cdiv(std::max(total, n + 1), 256)), dim3(256), 0, s, d_off, n, total, xy, keep, pid, kpos, pk, noff, nidx, c->gc_pts.as<int2>(),
                         c->gc_off.as<long long>(), c->gc_src.as<int>()); }
    HIPC(c, hipGetLastError());
    struct { unsigned tot, cnt; int err; } h = {0, 0, 0};
    HIPC(c, hipMemcpyAsync(&h.tot, noff + n, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.cnt, nidx + n, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.err, err, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (h.err) ORIP_FAIL(c, "a path holds a coordinate that is not finite after the conversion to steps");
    c->gc_n = h.cnt; c->gc_total = h.tot; c->gc_ready = true;
    *n_out = h.cnt; *total_out = h.tot;
    return 0;
}

extern "C" int orip_gcode_steps_fetch(orip_ctx* c, int64_t* off_out, int32_t* pts_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!off_out) ORIP_FAIL(c, "bad arguments");
    if (!c->gc_ready) ORIP_FAIL(c, "no step polylines: orip_gcode_to_steps has not succeeded since the last failure");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(off_out, c->gc_off.p, (size_t)(c->gc_n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (c->gc_total && pts_out) HIPC(c, hipMemcpyAsync(pts_out, c->gc_pts.p, (size_t)c->gc_total * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}

// src_out[k] = the input path step polyline k came from
extern "C" int orip_gcode_steps_source_fetch(orip_ctx* c, int32_t* src_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!c->gc_ready) ORIP_FAIL(c, "no step polylines: orip_gcode_to_steps has not succeeded since the last failure");
    if (c->gc_merged) ORIP_FAIL(c, "the step polylines have been merged: ask for the sources before orip_gcode_merge");
    if (c->gc_n == 0) return 0;
    if (!src_out) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(src_out, c->gc_src.p, (size_t)c->gc_n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}

// order[k] = index of the k-th path to draw.  ends: (first x, first y, last x, last y) per path, or NULL for the resident step polylines.
extern "C" int orip_gcode_order(orip_ctx* c, const int32_t* ends, int64_t n, int32_t* order_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (n < 0 || (n > 0 && !order_out)) ORIP_FAIL(c, "bad arguments");
    if (n == 0) return 0;
    if (!ends && (!c->gc_ready || n != c->gc_n)) ORIP_FAIL(c, "%lld paths asked for, %lld step polylines resident", (long long)n, (long long)(c->gc_ready ? c->gc_n : -1));
    if (n > (1 << 27)) ORIP_FAIL(c, "%lld paths: at most 2^27", (long long)n);
    if (ends)
        for (int64_t i = 0; i < 4 * n; i++) if (ends[i] < 0 || ends[i] > GC_COORD_MAX) ORIP_FAIL(c, "path %lld: coordinate %d outside 0..2^30", (long long)(i / 4), ends[i]);
    hipStream_t s = LN(c).stream;
    int4* se; int* box; int* order;
    { Carve L; L.take(se, (size_t)n); L.take(order, (size_t)n); L.take(box, 4); HIPC(c, L.commit(c->gc_ends, 64)); }
    if (ends) HIPC(c, hipMemcpyAsync(se, ends, (size_t)n * 16, hipMemcpyHostToDevice, s));
    else hipLaunchKernelGGL(k_gc_ends, dim3(cdiv(n, 256)), dim3(256), 0, s, c->gc_off.as<long long>(), c->gc_pts.as<int2>(), n, se);
    int hbox[4] = {INT_MAX, INT_MAX, INT_MIN, INT_MIN};
    HIPC(c, hipMemcpyAsync(box, hbox, 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gc_bbox, dim3(cdiv(n, 256)), dim3(256), 0, s, se, (int)n, box);
    HIPC(c, hipMemcpyAsync(hbox, box, 16, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (hbox[0] < 0 || hbox[1] < 0 || hbox[2] > GC_COORD_MAX || hbox[3] > GC_COORD_MAX || hbox[0] > hbox[2] || hbox[1] > hbox[3]) ORIP_FAIL(c, "bounding box of the first points is off");
    // square cells, a power of two wide: the smallest for which the grid has at most n / 2 cells (one cell at least), each side at most 2^15
    GcGrid g; g.x0 = hbox[0]; g.y0 = hbox[1]; g.x1 = hbox[2]; g.y1 = hbox[3];
    const int64_t wx = (int64_t)hbox[2] - hbox[0], wy = (int64_t)hbox[3] - hbox[1], want = std::max<int64_t>(1, n / 2);
    for (g.sh = 0;; g.sh++) {
        g.gx = (int)(wx >> g.sh) + 1; g.gy = (int)(wy >> g.sh) + 1;
        if (g.gx <= (1 << 15) && g.gy <= (1 << 15) && (int64_t)g.gx * g.gy <= want) break;
    }
    const int ncell = g.gx * g.gy;
    unsigned *cnt, *start, *fill; int2* hdr; int4* ent;
    { Carve L; L.take(cnt, (size_t)ncell + 1); L.take(start, (size_t)ncell + 1); L.take(fill, (size_t)ncell); L.take(hdr, (size_t)ncell); L.take(ent, (size_t)n);
      HIPC(c, L.commit(c->gc_grid, 64)); }
    HIPC(c, hipMemsetAsync(cnt, 0, ((size_t)ncell + 1) * 4, s));
    HIPC(c, hipMemsetAsync(fill, 0, (size_t)ncell * 4, s));
    hipLaunchKernelGGL(k_gc_count, dim3(cdiv(n, 256)), dim3(256), 0, s, se, (int)n, g, cnt);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, cnt, start, 0u, (size_t)ncell + 1, rocprim::plus<unsigned>(), s); }));
    hipLaunchKernelGGL(k_gc_fill, dim3(cdiv(n, 256)), dim3(256), 0, s, se, (int)n, g, start, fill, ent);
    hipLaunchKernelGGL(k_gc_hdr, dim3(cdiv(ncell, 256)), dim3(256), 0, s, start, cnt, ncell, hdr);
    { ProfScope ps(c, "k_gc_chain");
      hipLaunchKernelGGL(k_gc_chain, dim3(1), dim3(64), 0, s, se, (int)n, hdr, ent, g, order); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(order_out, order, (size_t)n * 4, hipMemcpyDeviceToHost, s));
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
    if (n_groups < 1 || n_groups > ORIP_ORDER_MAX_GROUPS) ORIP_FAIL(c, "%d groups: 1..%d", n_groups, ORIP_ORDER_MAX_GROUPS);
    const int sx = start_xy ? start_xy[0] : 0, sy = start_xy ? start_xy[1] : 0;
    if (sx < 0 || sy < 0 || sx > GC_COORD_MAX || sy > GC_COORD_MAX) ORIP_FAIL(c, "start (%d, %d) outside 0..2^30", sx, sy);
    if (n == 0) return 0;
    if (!ends && (!c->gc_ready || n != c->gc_n)) ORIP_FAIL(c, "%lld paths asked for, %lld step polylines resident", (long long)n, (long long)(c->gc_ready ? c->gc_n : -1));
    if (n > (1 << 26)) ORIP_FAIL(c, "%lld paths: at most 2^26", (long long)n);
    int64_t paths[ORIP_ORDER_MAX_GROUPS] = {0};
    for (int64_t i = 0; i < n; i++) {
        if (group[i] < 0 || group[i] >= n_groups) ORIP_FAIL(c, "path %lld: group %d of %d", (long long)i, group[i], n_groups);
        paths[group[i]]++;
    }
    if (ends)
        for (int64_t i = 0; i < 4 * n; i++) if (ends[i] < 0 || ends[i] > GC_COORD_MAX) ORIP_FAIL(c, "path %lld: coordinate %d outside 0..2^30", (long long)(i / 4), ends[i]);
    const int rev = flags & ORIP_ORDER_REVERSE ? 1 : 0, G = n_groups;
    const int64_t m = n << rev;                                             // candidates
    hipStream_t s = LN(c).stream;
    int4* se; int *grp, *order, *box; uint8_t* rv; OpGroup* dG;
    { Carve L; L.take(se, (size_t)n); L.take(grp, (size_t)n); L.take(order, (size_t)n); L.take(rv, (size_t)n); L.take(box, (size_t)4 * G); L.take(dG, (size_t)G); HIPC(c, L.commit(c->op_ends, 64)); }
    if (ends) HIPC(c, hipMemcpyAsync(se, ends, (size_t)n * 16, hipMemcpyHostToDevice, s));
    else hipLaunchKernelGGL(k_gc_ends, dim3(cdiv(n, 256)), dim3(256), 0, s, c->gc_off.as<long long>(), c->gc_pts.as<int2>(), n, se);
    HIPC(c, hipMemcpyAsync(grp, group, (size_t)n * 4, hipMemcpyHostToDevice, s));
    int hbox[4 * ORIP_ORDER_MAX_GROUPS];
    for (int g = 0; g < G; g++) { hbox[4 * g] = hbox[4 * g + 1] = INT_MAX; hbox[4 * g + 2] = hbox[4 * g + 3] = INT_MIN; }
    HIPC(c, hipMemcpyAsync(box, hbox, (size_t)16 * G, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_op_bbox, dim3(cdiv(m, 256)), dim3(256), 0, s, se, grp, (int)m, rev, box);
    HIPC(c, hipMemcpyAsync(hbox, box, (size_t)16 * G, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    // per group the grid of orip_gcode_order over its candidates: square cells, a power of two wide, at most half as many cells as candidates
    OpGroup hG[ORIP_ORDER_MAX_GROUPS];
    int64_t ncell = 0;
    for (int g = 0; g < G; g++) {
        OpGroup& o = hG[g];
        o.g = GcGrid{0, 0, 0, 0, 0, 1, 1}; o.cell0 = (int)ncell; o.paths = (int)paths[g];
        if (!paths[g]) continue;                                              // an empty group: no cells, no steps
        const int* b = hbox + 4 * g;
        if (b[0] < 0 || b[1] < 0 || b[2] > GC_COORD_MAX || b[3] > GC_COORD_MAX || b[0] > b[2] || b[1] > b[3]) ORIP_FAIL(c, "bounding box of group %d is off", g);
        o.g.x0 = b[0]; o.g.y0 = b[1]; o.g.x1 = b[2]; o.g.y1 = b[3];
        const int64_t wx = (int64_t)b[2] - b[0], wy = (int64_t)b[3] - b[1], want = std::max<int64_t>(1, (paths[g] << rev) / 2);
        for (o.g.sh = 0;; o.g.sh++) {
            o.g.gx = (int)(wx >> o.g.sh) + 1; o.g.gy = (int)(wy >> o.g.sh) + 1;
            if (o.g.gx <= (1 << 15) && o.g.gy <= (1 << 15) && (int64_t)o.g.gx * o.g.gy <= want) break;
        }
        ncell += (int64_t)o.g.gx * o.g.gy;                                    // at most m / 2 + G over all groups
    }
    unsigned *cnt, *start, *fill; int2* hdr; int4* ent; int* slot;
    { Carve L; L.take(cnt, (size_t)ncell + 1); L.take(start, (size_t)ncell + 1); L.take(fill, (size_t)ncell); L.take(hdr, (size_t)ncell); L.take(ent, (size_t)m);
      L.take(slot, rev ? (size_t)m : 0); HIPC(c, L.commit(c->op_grid, 64)); }
    HIPC(c, hipMemcpyAsync(dG, hG, sizeof(OpGroup) * G, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(cnt, 0, ((size_t)ncell + 1) * 4, s));
    HIPC(c, hipMemsetAsync(fill, 0, (size_t)ncell * 4, s));
    hipLaunchKernelGGL(k_op_count, dim3(cdiv(m, 256)), dim3(256), 0, s, se, grp, (int)m, rev, dG, cnt);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, cnt, start, 0u, (size_t)ncell + 1, rocprim::plus<unsigned>(), s); }));
    hipLaunchKernelGGL(k_op_fill, dim3(cdiv(m, 256)), dim3(256), 0, s, se, grp, (int)m, rev, dG, start, fill, ent, slot);
    hipLaunchKernelGGL(k_gc_hdr, dim3(cdiv(ncell, 256)), dim3(256), 0, s, start, cnt, (int)ncell, hdr);
    { ProfScope ps(c, "k_op_chain");
      hipLaunchKernelGGL(k_op_chain, dim3(1), dim3(64), 0, s, se, (int)n, dG, G, rev, sx, sy, (int)ncell, (int)m, hdr, ent, slot, order, rv); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(order_out, order, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(rev_out, rv, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (order_out[0] < 0) ORIP_FAIL(c, "the chain lost a path (internal error)");
    return 0;
}

// the bytes of a stream from the resident direction codes of orip_stream_codes and the host's plan
extern "C" int orip_stream_pack(orip_ctx* c, int64_t n_pieces, const int64_t* code0, const int32_t* cnt, const int64_t* pos, const int32_t* speed, int64_t n_service,
                                const int64_t* svc_pos, const uint8_t* svc_val, int64_t nbytes) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    c->pk_bytes = -1;
    if (n_pieces < 0 || n_service < 0 || nbytes < 0 || (n_pieces > 0 && (!code0 || !cnt || !pos || !speed)) || (n_service > 0 && (!svc_pos || !svc_val))) ORIP_FAIL(c, "bad arguments");
    // every piece reads inside the resident codes and writes inside the stream, behind the piece before it: nothing below can leave its buffers
    int64_t end = 0;
    for (int64_t i = 0; i < n_pieces; i++) {
        const int64_t size = (speed[i] >= 0 ? 1 : 0) + ((int64_t)cnt[i] + 1) / 2;
        if (cnt[i] < 0 || speed[i] > 255 || size < 1 || code0[i] < 0 || code0[i] + cnt[i] > c->stream_total || pos[i] < end || pos[i] + size > nbytes)
            ORIP_FAIL(c, "piece %lld does not fit (%lld codes from %lld of %lld resident, %lld bytes at %lld of %lld, previous piece ends at %lld)", (long long)i, (long long)cnt[i],
                      (long long)code0[i], (long long)c->stream_total, (long long)size, (long long)pos[i], (long long)nbytes, (long long)end);
        end = pos[i] + size;
    }
    for (int64_t i = 0; i < n_service; i++) if (svc_pos[i] < 0 || svc_pos[i] >= nbytes) ORIP_FAIL(c, "service byte %lld at %lld of %lld", (long long)i, (long long)svc_pos[i], (long long)nbytes);
    if (nbytes == 0) { c->pk_bytes = 0; return 0; }
    hipStream_t s = LN(c).stream;
    long long *d_pos, *d_code0, *d_spos; int *d_cnt, *d_speed; uint8_t* d_sval;
    { Carve L; L.take(d_pos, (size_t)n_pieces); L.take(d_code0, (size_t)n_pieces); L.take(d_spos, (size_t)n_service); L.take(d_cnt, (size_t)n_pieces); L.take(d_speed, (size_t)n_pieces);
      L.take(d_sval, (size_t)n_service); HIPC(c, L.commit(c->pk_tab, 64)); }
    HIPC(c, c->pk_out.ensure((size_t)nbytes + 64));
    if (n_pieces) {
        HIPC(c, hipMemcpyAsync(d_pos, pos, (size_t)n_pieces * 8, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_code0, code0, (size_t)n_pieces * 8, hipMemcpyHostToDevice, s));
        HIPC(c, hipMemcpyAsync(d_cnt, cnt, (size_t)n_pieces * 4, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_speed, speed, (size_t)n_pieces * 4, hipMemcpyHostToDevice, s));
    }
    if (n_service) { HIPC(c, hipMemcpyAsync(d_spos, svc_pos, (size_t)n_service * 8, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_sval, svc_val, (size_t)n_service, hipMemcpyHostToDevice, s)); }
    { ProfScope ps(c, "k_pk_bytes");
      hipLaunchKernelGGL(k_pk_bytes, dim3((unsigned)((nbytes + 255) / 256)), dim3(256), 0, s, d_pos, d_code0, d_cnt, d_speed, n_pieces, c->stream_codes.as<uint8_t>(), nbytes,
                         c->pk_out.as<uint8_t>()); }
    if (n_service) hipLaunchKernelGGL(k_pk_service, dim3((unsigned)((n_service + 255) / 256)), dim3(256), 0, s, d_spos, d_sval, n_service, c->pk_out.as<uint8_t>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    c->pk_bytes = nbytes;
    return 0;
}

extern "C" int orip_stream_pack_fetch(orip_ctx* c, uint8_t* out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (c->pk_bytes < 0) ORIP_FAIL(c, "no packed stream: orip_stream_pack has not succeeded since the last failure");
    if (c->pk_bytes == 0) return 0;
    if (!out) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(out, c->pk_out.p, (size_t)c->pk_bytes, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
