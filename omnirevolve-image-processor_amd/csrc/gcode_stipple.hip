// csrc/gcode_stipple.hip -- --stipple-mm of svg2stream.py: closed shapes are filled with dots, the plotter's taps (orip_gcode_stipple, orip_svg_stipple; the
// rule is stated in include/orip.h, is exact in integers on the step grid and has one answer for every input).  Ours: the reference has no such pass.
//
// SHAPE s is the s-th distinct ring group, ascending: its rings, and with them its EDGES (edge i runs from ring point i to the next point of its ring, the
// first one behind the last), are contiguous because ring_group is sorted; a later shape is a higher one.  The SLOTS of a shape are the lattice points of
// its bounding box, row after row: nrows rows from j0 = ceil(box y0 / q) and, in every row, `cols` = floor(box width / p) + 1 columns from the row's first
// lattice x >= box x0 (a row of the other parity may hold one point fewer: a slot beyond box x1 is no lattice point of the box and is never looked at).
// Slot k = row * cols + column, so the slots ascend as the dots leave: row ascending, x ascending.  A CHUNK is 64 consecutive slots of one shape: the work
// of one wave, one slot a lane, whatever the shape's width.
//
// 1. Rings, as the occlusion takes them: orip_svg_stipple gathers ring r from the resident fitted path ring_sub[r] and converts every point with
//    gc_ring_step (gc_convert.h); the offsets of the fitted paths are read back once for the ring sizes.  k_st_edges, one thread per ring point: the edge,
//    the shape's bounding box by integer atomics, and whether the shape has an edge of positive length.
// 2. k_st_plan, one thread per shape: j0, nrows, cols and the number of chunks; a scan places the chunks.  The host reads the chunks, the rows and what the
//    conversion found (first read-back: 2^28 rows or chunks or more is refused) and sizes the per-chunk arrays.
// 3. k_st_test, one WAVE per chunk.  The shape's edges are read 64 at a time, those that can matter to the chunk (st_walk: a ballot over one edge a lane)
//    go through an LDS tile, and every lane walks the tile for its own slot: the parity of the
//    edges that cross the ray towards +x (half-open in y, so a vertex on the ray counts once), "on an edge", and the CLEAR test behind a box test (a point
//    further than `inset` from an edge's box is clear of it, exactly) -- one pass over the edges gives all three.  Then the rect; then, under
//    ORIP_STIPPLE_OCCLUDE, the shapes above: 64 boxes at a time against the box of the lanes still alive, a ballot names the shapes that meet it, and their
//    edges go through the same tile for the parity alone.  The verdict is a ballot: the chunk's dot mask and its count; the five counters are summed per
//    wave and added once.  A scan of the counts places the dots; the host reads their number (second read-back: 2^26 or more is refused).
// 4. k_st_emit, one wave per chunk with a dot: a dot's place is its chunk's base plus the dots below it in the mask; under ORIP_STIPPLE_SERPENTINE a dot of
//    an odd row counts from the row's other end (the row's first and last place come from the same scan and masks).
// Why not crossings sorted into spans: the candidates must be exactly the INSIDE set, so a span kernel would still have to decide the lattice points on
// vertices and on horizontal edges by the orientation tests; deciding every slot of the box by them needs no sort, no per-row list and no size class, and
// the CLEAR test, which reads every edge of the shape for every candidate anyway, rides on the same pass over the tile (DESIGN 5 "stipple").
// Everything on the calling lane's stream; a third read-back fetches the counters behind the last launch.
//
// Scratch (orip_ctx.h states the three buffers).  c->st_tmp, ONE Carve: roff long long[m + 1]; rsub int[m]; rpts int2[R]; edges int4[R]; spt long long
// [ns + 1] (first ring point of every shape); sgrp int[ns]; sbox int4[ns]; shas int[ns]; plan StPlan[ns]; nch u64[ns + 1], cbase u64[ns + 1] (chunks per
// shape, their scan); StCounters.  c->st_ch, one Carve behind the first read-back, C chunks: mask u64[C]; cnt u64[C + 1], dbase u64[C + 1] (dots per
// chunk, their scan).  Resident until the next call: c->st_out = xy int2[dots], grp int[dots].
#include "orip_ctx.h"
#include "gc_convert.h"
#include <algorithm>
#include <climits>
#include <vector>

namespace {
typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;
constexpr int ST_BLOCKS = 8192;                                                       // one wave each; they stride over the chunks
constexpr u64 ST_MAX_DOTS = 1ull << 26, ST_MAX_ROWS = 1ull << 28, ST_MAX_CHUNKS = 1ull << 28;
constexpr unsigned ST_BAD_NOT_FINITE = 1, ST_BAD_RANGE = 2, ST_BAD_PLACE = 4;
struct StCounters { u64 groups, rows, candidates, near, outside, hidden, dots; unsigned bad; };
struct StLattice { int p, q, s, inset; };
struct StPlan { long long j0, nrows, cols; };
struct StShapes { const long long* spt; const int* sgrp; const int4* sbox; const int* shas; const StPlan* plan; const int4* edges; const u64* cbase; int64_t ns; };

__host__ __device__ __forceinline__ long long st_floordiv(long long a, long long b) { const long long q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }     // b > 0
__host__ __device__ __forceinline__ long long st_ceildiv(long long a, long long b) { return -st_floordiv(-a, b); }

// the shape that owns chunk ch: the last s with cbase[s] <= ch (shapes without chunks are skipped by the search)
__device__ __forceinline__ int64_t st_shape_of(const u64* __restrict__ cbase, int64_t ns, u64 ch) {
    int64_t lo = 0, hi = ns;
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (cbase[mid] <= ch) lo = mid; else hi = mid; }
    return lo;
}
// slot k of a shape: its row number j and its point; false when the slot lies beyond the shape's rows or beyond the box in its row
__device__ __forceinline__ bool st_slot(const StPlan pl, const int4 box, const StLattice lt, u64 k, long long& j, int2& P) {
    P = make_int2(0, 0); j = 0;
    if (pl.cols < 1 || k >= (u64)pl.nrows * (u64)pl.cols) return false;
    const long long row = (long long)(k / (u64)pl.cols), col = (long long)(k % (u64)pl.cols);
    j = pl.j0 + row;
    const long long sh = (j & 1) ? lt.s : 0;
    const long long x = (st_ceildiv((long long)box.x - sh, lt.p) + col) * lt.p + sh, y = j * lt.q;
    if (x > box.z) return false;
    P = make_int2((int)x, (int)y);
    return true;
}
// edge e against P: the parity of the crossings of the ray towards +x, P on the edge, and (inset > 0) P nearer than inset to the edge
template <bool CLEAR>
__device__ __forceinline__ void st_edge(const int4 e, const int2 P, int inset, bool& par, bool& on, bool& nearb) {
    if (e.x == e.z && e.y == e.w) return;
    const int xlo = min(e.x, e.z), xhi = max(e.x, e.z), ylo = min(e.y, e.w), yhi = max(e.y, e.w);
    const bool row = P.y >= ylo && P.y <= yhi;
    const bool box = CLEAR && inset > 0 && P.x >= xlo - inset && P.x <= xhi + inset && P.y >= ylo - inset && P.y <= yhi + inset;
    if (!row && !box) return;
    const long long dx = (long long)e.z - e.x, dy = (long long)e.w - e.y, wx = (long long)P.x - e.x, wy = (long long)P.y - e.y;
    const i128 cr = (i128)dx * wy - (i128)dy * wx;
    if (row) {
        if (cr == 0) { if (P.x >= xlo && P.x <= xhi) on = true; }                     // off the segment only along a horizontal edge, which crosses nothing
        else if ((e.y <= P.y) != (e.w <= P.y)) par ^= dy > 0 ? cr > 0 : cr < 0;
    }
    if (box) {
        const u64 L = (u64)(dx * dx) + (u64)(dy * dy), in2 = (u64)inset * (u64)inset;
        const i128 t = (i128)wx * dx + (i128)wy * dy;
        if (t <= 0) nearb |= (u64)(wx * wx) + (u64)(wy * wy) < in2;
        else if (t >= (i128)L) { const long long vx = (long long)P.x - e.z, vy = (long long)P.y - e.w; nearb |= (u64)(vx * vx) + (u64)(vy * vy) < in2; }
        else { const u128 a = (u128)(cr < 0 ? -cr : cr); nearb |= a * a < (u128)in2 * L; }
    }
}

// the box (x0, y0, x1, y1) of the points of the lanes in `act`; of no lane: (INT_MAX, INT_MAX, INT_MIN, INT_MIN), which meets nothing
__device__ __forceinline__ int4 st_wave_box(bool act, const int2 P) {
    int4 b = act ? make_int4(P.x, P.y, P.x, P.y) : make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { b.x = min(b.x, __shfl_xor(b.x, d, 64)); b.y = min(b.y, __shfl_xor(b.y, d, 64)); b.z = max(b.z, __shfl_xor(b.z, d, 64)); b.w = max(b.w, __shfl_xor(b.w, d, 64)); }
    return b;
}
// The edges [e0, e1) of one shape against the points of the lanes in `act`, 64 edges at a time: every lane looks at one edge, and a ballot names those that can
// matter to a point of the wave's box wb -- their y range, widened by inset, meets the box's, and they do not lie wholly to the left of it (such an edge
// crosses no ray towards +x and holds no point of the box).  Those go through the LDS tile and every lane walks them.  A chunk is a row or two of the
// lattice, so of a long outline a few edges in a thousand are walked; a tile without one costs its load and the ballot.  Called by the whole block.
template <bool CLEAR>
__device__ __forceinline__ void st_walk(const int4* __restrict__ edges, long long e0, long long e1, int4* tile, int lane, const int4 wb, bool act, const int2 P, int inset,
                                        bool& par, bool& on, bool& nearb) {
    for (long long eb = e0; eb < e1; eb += 64) {
        int4 e = make_int4(0, 0, 0, 0);
        bool rel = false;
        if (eb + lane < e1) {
            e = edges[eb + lane];
            rel = (e.x != e.z || e.y != e.w) && max(e.y, e.w) + inset >= wb.y && min(e.y, e.w) - inset <= wb.w && max(e.x, e.z) + inset >= wb.x;
        }
        u64 mm = __ballot(rel);                                                       // wave-uniform, and the block is one wave
        if (!mm) continue;
        __syncthreads();                                                              // the tile before this one has been read
        tile[lane] = e;
        __syncthreads();
        for (; mm; mm &= mm - 1) if (act) st_edge<CLEAR>(tile[__ffsll((long long)mm) - 1], P, inset, par, on, nearb);
    }
}

// ------------------------------------------------------------------------------------------------ 1. rings
__global__ __launch_bounds__(256) void k_st_rings(const long long* __restrict__ roff, int64_t m, int64_t R, const int* __restrict__ rsub, const long long* __restrict__ sv_off,
                                                  const double2* __restrict__ sv_pts, orip_gcode_map g, int clamp, int2* __restrict__ rpts, StCounters* cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int64_t r = gc_path_of(roff, m, i);
    int2 o;
    const unsigned why = gc_ring_step(g, sv_pts[sv_off[rsub[r]] + (i - roff[r])], clamp, o);                  // gc_convert.h: shared with the occlusion and the hatch link
    if (why) atomicOr(&cn->bad, why == GC_RING_NOT_FINITE ? ST_BAD_NOT_FINITE : ST_BAD_RANGE);
    rpts[i] = o;
}
__global__ __launch_bounds__(256) void k_st_boxinit(int4* __restrict__ sbox, int* __restrict__ shas, int64_t ns) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < ns) { sbox[s] = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN); shas[s] = 0; }
}
__global__ __launch_bounds__(256) void k_st_edges(const long long* __restrict__ roff, int64_t m, int64_t R, const int2* __restrict__ rpts, const long long* __restrict__ spt,
                                                  int64_t ns, int4* __restrict__ edges, int4* sbox, int* shas) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int64_t r = gc_path_of(roff, m, i), s = gc_path_of(spt, ns, i);
    const int2 P = rpts[i], Q = rpts[i + 1 < roff[r + 1] ? i + 1 : roff[r]];
    edges[i] = make_int4(P.x, P.y, Q.x, Q.y);
    int* const b = (int*)&sbox[s];
    atomicMin(b + 0, P.x); atomicMin(b + 1, P.y); atomicMax(b + 2, P.x); atomicMax(b + 3, P.y);
    if (P.x != Q.x || P.y != Q.y) atomicOr(&shas[s], 1);
}

// ------------------------------------------------------------------------------------------------ 2. the slots of every shape
__global__ __launch_bounds__(256) void k_st_plan(const int4* __restrict__ sbox, const int* __restrict__ shas, int64_t ns, StLattice lt, StPlan* __restrict__ plan,
                                                 u64* __restrict__ nch, StCounters* cn) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > ns) return;
    if (s == ns) { nch[s] = 0; return; }
    StPlan pl = {0, 0, 0};
    u64 chunks = 0;
    if (shas[s]) {                                                                    // a shape without an edge of positive length has no interior
        const int4 b = sbox[s];
        pl.j0 = st_ceildiv(b.y, lt.q);
        const long long nr = st_floordiv(b.w, lt.q) - pl.j0 + 1;
        pl.nrows = nr > 0 ? nr : 0;
        pl.cols = ((long long)b.z - b.x) / lt.p + 1;
        const u64 slots = (u64)pl.nrows * (u64)pl.cols;                               // at most 2^31 * 2^30
        chunks = (slots + 63) / 64 < ST_MAX_CHUNKS ? (slots + 63) / 64 : ST_MAX_CHUNKS;                          // capped, so that the sum over 2^26 shapes cannot wrap: the total is refused all the same
        atomicAdd(&cn->groups, 1ull);
        if (pl.nrows) atomicAdd(&cn->rows, (u64)pl.nrows);
    }
    plan[s] = pl; nch[s] = chunks;
}

// ------------------------------------------------------------------------------------------------ 3. the verdict of every slot
__global__ __launch_bounds__(64) void k_st_test(StShapes sh, StLattice lt, int4 rect, int occlude, u64 C, u64* __restrict__ mask, u64* __restrict__ cnt, StCounters* cn) {
    __shared__ int4 tile[64];
    const int lane = threadIdx.x;
    u64 n_cand = 0, n_near = 0, n_out = 0, n_hid = 0, n_dot = 0;
    if (blockIdx.x == 0 && lane == 0) cnt[C] = 0;
    for (u64 ch = blockIdx.x; ch < C; ch += gridDim.x) {                              // ch, and with it the shape, is the same in the whole block of one wave
        const int64_t g = st_shape_of(sh.cbase, sh.ns, ch);
        long long j; int2 P;
        const bool valid = st_slot(sh.plan[g], sh.sbox[g], lt, (ch - sh.cbase[g]) * 64 + (u64)lane, j, P);
        bool par = false, on = false, nearb = false;
        st_walk<true>(sh.edges, sh.spt[g], sh.spt[g + 1], tile, lane, st_wave_box(valid, P), valid, P, lt.inset, par, on, nearb);
        const bool cand = valid && par && !on;
        const bool nr = cand && nearb;
        const bool out = cand && !nr && (P.x < rect.x || P.x > rect.z || P.y < rect.y || P.y > rect.w);
        bool live = cand && !nr && !out, hid = false;
        if (occlude && __ballot(live)) {                                              // the shapes above, behind their boxes
            const int4 wb = st_wave_box(live, P);
            for (int64_t sb = g + 1; sb < sh.ns; sb += 64) {
                bool meet = false;
                if (sb + lane < sh.ns && sh.shas[sb + lane]) { const int4 b = sh.sbox[sb + lane]; meet = b.x <= wb.z && b.z >= wb.x && b.y <= wb.w && b.w >= wb.y; }
                for (u64 mm = __ballot(meet); mm; mm &= mm - 1) {                     // wave-uniform: a ballot
                    const int64_t s = sb + (__ffsll((long long)mm) - 1);
                    const int4 b = sh.sbox[s];
                    const bool in_box = live && !hid && P.x >= b.x && P.x <= b.z && P.y >= b.y && P.y <= b.w;
                    bool par2 = false, on2 = false, unused = false;
                    st_walk<false>(sh.edges, sh.spt[s], sh.spt[s + 1], tile, lane, wb, in_box, P, 0, par2, on2, unused);
                    hid = hid || (in_box && par2 && !on2);
                }
                if (!__ballot(live && !hid)) break;
            }
        }
        const bool dot = live && !hid;
        const u64 md = __ballot(dot);
        n_cand += (u64)__popcll(__ballot(cand)); n_near += (u64)__popcll(__ballot(nr)); n_out += (u64)__popcll(__ballot(out));
        n_hid += (u64)__popcll(__ballot(live && hid)); n_dot += (u64)__popcll(md);
        if (lane == 0) { mask[ch] = md; cnt[ch] = (u64)__popcll(md); }
    }
    if (lane == 0 && n_cand) {
        atomicAdd(&cn->candidates, n_cand); atomicAdd(&cn->near, n_near); atomicAdd(&cn->outside, n_out); atomicAdd(&cn->hidden, n_hid); atomicAdd(&cn->dots, n_dot);
    }
}

// ------------------------------------------------------------------------------------------------ 4. emit
// the dots in front of slot k of shape g (k may be the shape's slot count: the dots in front of the next shape)
__device__ __forceinline__ u64 st_before(const u64* __restrict__ mask, const u64* __restrict__ dbase, u64 c0, u64 k) {
    const u64 ch = c0 + k / 64; const unsigned r = (unsigned)(k % 64);
    return r ? dbase[ch] + (u64)__popcll(mask[ch] & ((1ull << r) - 1)) : dbase[ch];
}
__global__ __launch_bounds__(64) void k_st_emit(StShapes sh, StLattice lt, int serpentine, u64 C, const u64* __restrict__ mask, const u64* __restrict__ dbase, u64 D,
                                                int2* __restrict__ xy, int* __restrict__ grp, StCounters* cn) {
    const int lane = threadIdx.x;
    for (u64 ch = blockIdx.x; ch < C; ch += gridDim.x) {
        const u64 md = mask[ch];
        if (!((md >> lane) & 1)) continue;
        const int64_t g = st_shape_of(sh.cbase, sh.ns, ch);
        const StPlan pl = sh.plan[g];
        const u64 c0 = sh.cbase[g], k = (ch - c0) * 64 + (u64)lane;
        long long j; int2 P;
        if (!st_slot(pl, sh.sbox[g], lt, k, j, P)) { atomicOr(&cn->bad, ST_BAD_PLACE); continue; }
        u64 at = dbase[ch] + (u64)__popcll(md & ((1ull << lane) - 1));
        if (serpentine && (j & 1)) {                                                  // from the row's other end
            const u64 k0 = k - k % (u64)pl.cols;
            at = st_before(mask, dbase, c0, k0) + st_before(mask, dbase, c0, k0 + (u64)pl.cols) - 1 - at;
        }
        if (at >= D) { atomicOr(&cn->bad, ST_BAD_PLACE); continue; }
        xy[at] = P; grp[at] = sh.sgrp[g];
    }
}

// the rings of one call: explicit in steps, or the resident fitted paths ring_sub of orip_svg_stipple
struct StRings { const int64_t* off; const int32_t* pts; const int32_t* sub; const int32_t* group; int64_t m; const orip_gcode_map* map; int clamp; };

// both entry points behind their own checks: the other checks, then the pass
int st_core(orip_ctx* c, const char* who, const StRings& rg, int32_t pitch, int32_t row, int32_t shift, int32_t inset, const int32_t* rect, int32_t flags, int64_t* stats) {
    const int64_t m = rg.m;
    if (!stats || !rect) ORIP_FAIL_AS(c, who, "bad arguments");
    if (pitch < 2 || pitch > ORIP_STIPPLE_MAX) ORIP_FAIL_AS(c, who, "pitch %d: 2..2^20", pitch);
    if (row < 1 || row > ORIP_STIPPLE_MAX) ORIP_FAIL_AS(c, who, "row %d: 1..2^20", row);
    if (shift < 0 || shift >= pitch) ORIP_FAIL_AS(c, who, "shift %d: 0..pitch - 1", shift);
    if (inset < 0 || inset > ORIP_STIPPLE_MAX) ORIP_FAIL_AS(c, who, "inset %d: 0..2^20", inset);
    if (rect[2] < rect[0] || rect[3] < rect[1]) ORIP_FAIL_AS(c, who, "rect (%d, %d, %d, %d): x1 < x0 or y1 < y0", rect[0], rect[1], rect[2], rect[3]);
    for (int k = 0; k < 4; k++) if (rect[k] < -GC_COORD_MAX || rect[k] > GC_COORD_MAX) ORIP_FAIL_AS(c, who, "rect coordinate %d outside -2^30..2^30", rect[k]);
    if (m < 0 || m > (1 << 26)) ORIP_FAIL_AS(c, who, "%lld rings: 0..2^26", (long long)m);
    if (m > 0 && (!rg.group || (rg.sub ? false : !rg.off))) ORIP_FAIL_AS(c, who, "bad arguments");
    for (int64_t r = 0; r < m; r++) {
        if (rg.group[r] < 0 || rg.group[r] >= GC_COORD_MAX) ORIP_FAIL_AS(c, who, "ring %lld: group %d outside 0..2^30 - 1", (long long)r, rg.group[r]);
        if (r && rg.group[r] < rg.group[r - 1]) ORIP_FAIL_AS(c, who, "ring %lld: group %d below the group before it (ring_group must not decrease)", (long long)r, rg.group[r]);
    }
    hipStream_t s = LN(c).stream;
    std::vector<long long> roff((size_t)m + 1, 0);
    if (rg.sub) {                                                             // the sizes of the resident fitted paths: one read-back of their offsets
        if (m > 0 && !c->sv_ready) ORIP_FAIL_AS(c, who, "no fitted paths resident");
        for (int64_t r = 0; r < m; r++) if (rg.sub[r] < 0 || rg.sub[r] >= c->sv_n) ORIP_FAIL_AS(c, who, "ring %lld: path %d of %lld resident fitted paths", (long long)r, rg.sub[r], (long long)c->sv_n);
        if (m > 0) {
            std::vector<long long> sv((size_t)c->sv_n + 1);
            HIPC_AS(c, who, hipMemcpyAsync(sv.data(), c->sv_off.p, sv.size() * 8, hipMemcpyDeviceToHost, s));
            HIPC_AS(c, who, hipStreamSynchronize(s));
            for (int64_t r = 0; r < m; r++) {
                const long long k = sv[(size_t)rg.sub[r] + 1] - sv[(size_t)rg.sub[r]];
                if (k < 1) ORIP_FAIL_AS(c, who, "ring %lld has no points", (long long)r);
                roff[(size_t)r + 1] = roff[(size_t)r] + k;
                if (roff[(size_t)r + 1] >= (1ll << 28)) ORIP_FAIL_AS(c, who, "%lld ring points or more: fewer than 2^28", (long long)roff[(size_t)r + 1]);
            }
        }
    } else if (m > 0) {
        if (rg.off[0] != 0) ORIP_FAIL_AS(c, who, "ring offsets must start at 0");
        for (int64_t r = 0; r < m; r++) {
            if (rg.off[r + 1] < rg.off[r]) ORIP_FAIL_AS(c, who, "ring offsets must not decrease (ring %lld)", (long long)r);
            if (rg.off[r + 1] == rg.off[r]) ORIP_FAIL_AS(c, who, "ring %lld has no points", (long long)r);
            if (rg.off[r + 1] >= (1ll << 28)) ORIP_FAIL_AS(c, who, "%lld ring points or more: fewer than 2^28", (long long)rg.off[r + 1]);
            roff[(size_t)r + 1] = rg.off[r + 1];
        }
        if (!rg.pts) ORIP_FAIL_AS(c, who, "bad arguments");
        for (int64_t i = 0; i < 2 * rg.off[m]; i++)
            if (rg.pts[i] < -GC_COORD_MAX || rg.pts[i] > GC_COORD_MAX) ORIP_FAIL_AS(c, who, "ring point %lld: coordinate %d outside -2^30..2^30", (long long)(i / 2), rg.pts[i]);
    }
    const int64_t R = roff[(size_t)m];
    std::vector<long long> spt; std::vector<int> sgrp;                        // the shapes: runs of one group
    for (int64_t r = 0; r < m; r++) if (r == 0 || rg.group[r] != rg.group[r - 1]) { spt.push_back(roff[(size_t)r]); sgrp.push_back(rg.group[r]); }
    const int64_t ns = (int64_t)sgrp.size();
    spt.push_back(R);

    for (int k = 0; k < ORIP_STIPPLE_STATS; k++) stats[k] = 0;
    if (m == 0) { c->st_dots = 0; return 0; }                                 // nothing to launch: the list of no dots
    c->st_dots = -1;                                                          // no dot list from here to the last read-back
    const size_t Z = (size_t)ns;
    int *rsub, *d_sgrp, *shas; long long *d_roff, *d_spt; int2* rpts; int4 *edges, *sbox; StPlan* plan; u64 *nch, *cbase; StCounters* cn;
    { Carve L; L.take(d_roff, (size_t)m + 1); L.take(rsub, (size_t)m); L.take(rpts, (size_t)R); L.take(edges, (size_t)R); L.take(d_spt, Z + 1); L.take(d_sgrp, Z); L.take(sbox, Z);
      L.take(shas, Z); L.take(plan, Z); L.take(nch, Z + 1); L.take(cbase, Z + 1); L.take(cn, 1); HIPC_AS(c, who, L.commit(c->st_tmp, 64)); }
    HIPC_AS(c, who, hipMemcpyAsync(d_roff, roff.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemcpyAsync(d_spt, spt.data(), (Z + 1) * 8, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemcpyAsync(d_sgrp, sgrp.data(), Z * 4, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemsetAsync(cn, 0, sizeof(StCounters), s));
    const dim3 b(256);
    if (rg.sub) {
        HIPC_AS(c, who, hipMemcpyAsync(rsub, rg.sub, (size_t)m * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_st_rings, dim3(cdiv(R, 256)), b, 0, s, d_roff, m, R, rsub, c->sv_off.as<long long>(), c->sv_pts.as<double2>(), *rg.map, rg.clamp, rpts, cn);
    } else HIPC_AS(c, who, hipMemcpyAsync(rpts, rg.pts, (size_t)R * 8, hipMemcpyHostToDevice, s));
    const StLattice lt = {pitch, row, shift, inset};
    hipLaunchKernelGGL(k_st_boxinit, dim3(cdiv(ns, 256)), b, 0, s, sbox, shas, ns);
    hipLaunchKernelGGL(k_st_edges, dim3(cdiv(R, 256)), b, 0, s, d_roff, m, R, rpts, d_spt, ns, edges, sbox, shas);
    hipLaunchKernelGGL(k_st_plan, dim3(cdiv(ns + 1, 256)), b, 0, s, sbox, shas, ns, lt, plan, nch, cn);
    HIPC_AS(c, who, gc_scan_u64(c, nch, cbase, Z + 1));
    HIPC_AS(c, who, hipGetLastError());
    struct { u64 C; StCounters cn; } h1;                                      // first read-back: the chunks and the rows, and what the conversion of the rings found
    HIPC_AS(c, who, hipMemcpyAsync(&h1.C, cbase + Z, 8, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipMemcpyAsync(&h1.cn, cn, sizeof(StCounters), hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    if (h1.cn.bad & ST_BAD_NOT_FINITE) ORIP_FAIL_AS(c, who, "a ring holds a coordinate that is not finite after the conversion to steps");
    if (h1.cn.bad & ST_BAD_RANGE) ORIP_FAIL_AS(c, who, "a ring holds a point more than 2^30 steps off the sheet after the conversion to steps");
    if (h1.cn.rows >= ST_MAX_ROWS) ORIP_FAIL_AS(c, who, "%llu lattice rows over the shapes' boxes: fewer than 2^28", h1.cn.rows);
    if (h1.C >= ST_MAX_CHUNKS) ORIP_FAIL_AS(c, who, "%llu blocks of 64 lattice points over the shapes' boxes: fewer than 2^28", h1.C);
    const u64 C = h1.C;
    u64 D = 0;
    StCounters h = h1.cn;
    if (C) {
        u64 *mask, *cnt, *dbase;
        { Carve L; L.take(mask, (size_t)C); L.take(cnt, (size_t)C + 1); L.take(dbase, (size_t)C + 1); HIPC_AS(c, who, L.commit(c->st_ch, 64)); }
        const StShapes sh = {d_spt, d_sgrp, sbox, shas, plan, edges, cbase, ns};
        const int4 rc = make_int4(rect[0], rect[1], rect[2], rect[3]);
        const dim3 gw((unsigned)std::min<u64>(C, ST_BLOCKS));
        { ProfScope ps(c, "st_test");
          hipLaunchKernelGGL(k_st_test, gw, dim3(64), 0, s, sh, lt, rc, (flags & ORIP_STIPPLE_OCCLUDE) ? 1 : 0, C, mask, cnt, cn);
          HIPC_AS(c, who, gc_scan_u64(c, cnt, dbase, (size_t)C + 1)); }
        HIPC_AS(c, who, hipGetLastError());
        HIPC_AS(c, who, hipMemcpyAsync(&D, dbase + C, 8, hipMemcpyDeviceToHost, s));      // second read-back: the dots
        HIPC_AS(c, who, hipStreamSynchronize(s));
        if (D >= ST_MAX_DOTS) ORIP_FAIL_AS(c, who, "%llu dots: fewer than 2^26", D);
        int2* xy; int* grp;
        { Carve L; L.take(xy, (size_t)D); L.take(grp, (size_t)D); HIPC_AS(c, who, L.commit(c->st_out, 64)); }
        if (D) { ProfScope ps(c, "st_emit");
          hipLaunchKernelGGL(k_st_emit, gw, dim3(64), 0, s, sh, lt, (flags & ORIP_STIPPLE_SERPENTINE) ? 1 : 0, C, mask, dbase, D, xy, grp, cn); }
        HIPC_AS(c, who, hipGetLastError());
        HIPC_AS(c, who, hipMemcpyAsync(&h, cn, sizeof(StCounters), hipMemcpyDeviceToHost, s));      // third read-back: the counters
        HIPC_AS(c, who, hipStreamSynchronize(s));
    }
    if (h.bad || h.dots != D || h.candidates != h.near + h.outside + h.hidden + h.dots || (!(flags & ORIP_STIPPLE_OCCLUDE) && h.hidden))
        ORIP_FAIL_AS(c, who, "the dots do not add up (internal error %u)", h.bad);
    c->st_dots = (int64_t)D;
    stats[0] = (int64_t)h.groups; stats[1] = (int64_t)h.rows; stats[2] = (int64_t)h.candidates; stats[3] = (int64_t)h.near; stats[4] = (int64_t)h.outside;
    stats[5] = (int64_t)h.hidden; stats[6] = (int64_t)h.dots;
    return 0;
}
}  // namespace

// include/orip.h states the rule; the dots wait in c->st_out for the fetch
extern "C" int orip_gcode_stipple(orip_ctx* c, const int64_t* ring_off, const int32_t* ring_pts, const int32_t* ring_group, int64_t m, int32_t pitch, int32_t row, int32_t shift,
                                  int32_t inset, const int32_t* rect, int32_t flags, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (flags & ~(ORIP_STIPPLE_SERPENTINE | ORIP_STIPPLE_OCCLUDE)) ORIP_FAIL(c, "unknown flags %d", flags);
    const StRings rg = {ring_off, ring_pts, nullptr, ring_group, m, nullptr, 0};
    return st_core(c, __func__, rg, pitch, row, shift, inset, rect, flags, stats);
}

extern "C" int orip_svg_stipple(orip_ctx* c, const int32_t* ring_sub, const int32_t* ring_group, int64_t m, const orip_gcode_map* map, int32_t pitch, int32_t row, int32_t shift,
                                int32_t inset, const int32_t* rect, int32_t flags, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!map || (m > 0 && !ring_sub)) ORIP_FAIL(c, "bad arguments");
    if (flags & ~(ORIP_STIPPLE_SERPENTINE | ORIP_STIPPLE_OCCLUDE | ORIP_STIPPLE_CLAMP)) ORIP_FAIL(c, "unknown flags %d", flags);
    if (map->W < 1 || map->H < 1 || map->W > GC_COORD_MAX || map->H > GC_COORD_MAX) ORIP_FAIL(c, "target size %d x %d steps: each side must be in 1..2^30", map->W, map->H);
    static const int32_t none = 0;
    const StRings rg = {nullptr, nullptr, ring_sub ? ring_sub : &none, ring_group, m, map, (flags & ORIP_STIPPLE_CLAMP) ? 1 : 0};
    return st_core(c, __func__, rg, pitch, row, shift, inset, rect, flags, stats);
}

extern "C" int orip_gcode_stipple_fetch(orip_ctx* c, int32_t* xy, int32_t* group) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (c->st_dots < 0) ORIP_FAIL(c, "no result: the stipple has not succeeded since the last failure");
    if (c->st_dots == 0) return 0;
    if (!xy || !group) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    const size_t D = (size_t)c->st_dots;
    int2* d_xy; int* d_grp;                                                   // the layout st_core carved; the buffer already holds it, so nothing grows
    { Carve L; L.take(d_xy, D); L.take(d_grp, D); HIPC(c, L.commit(c->st_out, 64)); }
    HIPC(c, hipMemcpyAsync(xy, d_xy, D * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(group, d_grp, D * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
