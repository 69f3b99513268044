// csrc/gcode_occlude.hip -- --occlude of svg2stream.py: filled shapes hide what lies under them (orip_gcode_occlude, orip_svg_occlude; the rule is stated
// in include/orip.h, is exact in integers and rationals on the step grid and has one answer for every input).  Ours: the reference has no such pass.
//
// SEGMENT g is the g-th segment of the drawing, strokes in order, S = points - strokes of them.  SHAPE s is the s-th distinct ring level, ascending: its
// rings, and with them its points and its EDGES (edge i runs from ring point i to the next point of its ring, the first one behind the last), are
// contiguous because ring_level is sorted.  A PARAMETER is a rational num / den on one segment, clamped into [0, 1], so 0 <= num <= den <= 2^63: two
// unsigned 64-bit words, compared through 128-bit products.  The clamp is monotone, so the order of the events survives it, and what it merges lies outside.
//
// 1. Rings.  orip_svg_occlude: k_oc_rings gathers ring r from the resident fitted path ring_sub[r] and converts every point with gc_round_mm
//    (gc_convert.h), clamped under ORIP_OCCLUDE_CLAMP; the offsets of the fitted paths are read back once for the ring sizes.  k_oc_edges, one thread
//    per ring point: the edge, and the shape's bounding box by integer atomics.
// 2. k_oc_cand, one thread per point (the point ends segment g unless it starts its stroke).  The shapes above the stroke are a suffix of the shape table,
//    found by one binary search on the levels; the thread tests the segment's box against theirs.  WHAT IS CULLED BY: the level and the shape's box,
//    nothing finer.  A segment that meets no box is whole and costs these tests only; any other goes on the work list.
// 3. k_oc_count, one WAVE per listed segment: the lanes stride over the edges of every candidate shape and count the EVENTS:
//      a proper crossing (kind 0) at cross(e, P - A) / cross(e, d), counted with the half-open rule against the segment's own line: an edge end ON the line
//      counts as on its positive side, so an edge crosses iff exactly one end is strictly negative;
//      the two ends (kinds +1, -1) of the closed interval of a collinear edge, as (P - A) / d on the dominant axis.
//    A scan places every segment's events; the host reads the total (first read-back) and sizes the event buffers by it.
// 4. k_oc_pieces, one wave per listed segment, in the segment's own slice of the event buffers:
//      per candidate shape: the events are written, then ranked by (parameter, index) among the shape's own -- every lane takes an event and walks over
//      all of them, which also gives it the parity of the crossings and the balance of the collinear ends up to itself: the state BEHIND the event.  The
//      stretch from a ranked event to the next one is hidden by the shape iff the parity is odd, no collinear interval is open and the stretch is not
//      empty; those stretches are appended to the segment's interval list.  (Between events of equal parameter the state is unfinished, and the stretch empty.)
//      over all shapes: the intervals are ranked by (start, index) and swept 64 at a time with a wave prefix maximum of the ends, as k_dd_long sweeps: a
//      gap in front of an interval that starts beyond everything before it is a PIECE, and so is what is left behind the last one.  Intervals that touch
//      merge: a visible point of no length is not a piece.  Piece ends are rounded (oc_point) and the kept pieces are written in order.
//    Ranking by walking is quadratic in the events of one (segment, shape) and in the intervals of one segment, shared by 64 lanes; it needs no bound on
//    either, so a comb of any number of teeth and a shape of any number of edges take the same path as a square.
// 5. The cutting passes' compaction (gc_cut.h: k_gc_cut_compact, gc_scan_u64).  The host reads the totals (second read-back), refuses 2^30 points, sizes
//    the output, and k_oc_emit, one thread per segment, copies the pieces to where the scan says (gc_cut_piece), with origin and the gathered sources.
// Everything on the calling lane's stream; a third read-back fetches the counters behind the last launch.
//
// Scratch, free between calls.  c->oc_tmp, ONE Carve (oc_core): lvl int[n]; roff long long[m + 1]; rsub int[m]; rpts int2[R]; edges int4[R]; spt long
// long[ns + 1] (first ring point of every shape); slevel int[ns]; sbox int4[ns]; sinfo int2[S] (the segment's end point, its stroke); rec unsigned[S] (kept
// pieces | whole << 29 | first kept piece starts at the first vertex << 30 | last one ends at the second << 31); work unsigned[S]; evs u64[2 S + 2] (events
// per segment, their scan); scans u64[2 S + 2] (cs, scan); OcCounters.  c->oc_ev, one Carve behind the first read-back, E = all events: ev_t ulonglong2[E]
// and ev_k int[E] (the events), so_t ulonglong2[E] and so_h int[E] (ranked, with the state behind), iv_s and iv_e ulonglong2[E] (the hidden stretches).
// Ranked intervals reuse ev_t / so_t, the pieces (int4) reuse iv_s: a segment with K events has at most K - 1 stretches and K pieces.  72 bytes an event.
// Output: the record c->oc (gc_cut.h states the frame, orip_ctx.h the contract).
#include "orip_ctx.h"
#include "gc_convert.h"
#include <algorithm>
#include <climits>
#include <vector>

namespace {
typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;
constexpr int OC_BLOCKS = 4096;                                                       // one wave each; they stride over the work list
constexpr unsigned OC_NP = GC_CUT_NP, OC_WHOLE = GC_CUT_OWN, OC_FA = GC_CUT_FA, OC_FB = GC_CUT_FB;       // the pass's own bit: the segment is whole
constexpr unsigned OC_BAD_REPEAT = 1, OC_BAD_PLACE = 2, OC_BAD_LIST = 4, OC_BAD_COUNT = 8, OC_BAD_NOT_FINITE = 16, OC_BAD_RANGE = 32;
struct OcCounters { u64 whole, cut, hidden, pieces, collapsed, steps_in, steps_out; unsigned n_work, bad; };
struct OcShapes { const long long* spt; const int* slevel; const int4* sbox; const int4* edges; int64_t ns; };
struct OcSeg { int2 A, B; long long dx, dy; bool xdom; };

__device__ __forceinline__ bool oc_lt(const ulonglong2 a, const ulonglong2 b) { return (u128)a.x * b.y < (u128)b.x * a.y; }
__device__ __forceinline__ bool oc_eq(const ulonglong2 a, const ulonglong2 b) { return (u128)a.x * b.y == (u128)b.x * a.y; }
// num / den, den > 0, clamped into [0, 1]
__device__ __forceinline__ ulonglong2 oc_param(i128 num, i128 den) {
    if (num <= 0) return make_ulonglong2(0, 1);
    if (num >= den) return make_ulonglong2(1, 1);
    return make_ulonglong2((u64)num, (u64)den);
}
__device__ __forceinline__ OcSeg oc_seg(const int2 A, const int2 B) {
    OcSeg s; s.A = A; s.B = B; s.dx = (long long)B.x - A.x; s.dy = (long long)B.y - A.y;
    s.xdom = (s.dx < 0 ? -s.dx : s.dx) >= (s.dy < 0 ? -s.dy : s.dy);
    return s;
}
// the events of one edge on the segment: 0, 1 (a crossing) or 2 (the ends of a collinear overlap)
__device__ __forceinline__ int oc_events(const OcSeg& s, const int4 e, ulonglong2* t, int* kind) {
    if (e.x == e.z && e.y == e.w) return 0;
    const long long px = (long long)e.x - s.A.x, py = (long long)e.y - s.A.y, qx = (long long)e.z - s.A.x, qy = (long long)e.w - s.A.y;
    const i128 sp = (i128)s.dx * py - (i128)s.dy * px, sq = (i128)s.dx * qy - (i128)s.dy * qx;
    if (sp == 0 && sq == 0) {
        const long long d = s.xdom ? s.dx : s.dy, den = d < 0 ? -d : d;
        long long a = s.xdom ? px : py, b = s.xdom ? qx : qy;
        if (d < 0) { a = -a; b = -b; }
        if (a > b) { const long long w = a; a = b; b = w; }
        if (b <= 0 || a >= den) return 0;                                          // touches the segment in an end at most
        t[0] = oc_param(a, den); kind[0] = 1;
        t[1] = oc_param(b, den); kind[1] = -1;
        return 2;
    }
    if ((sp >= 0) == (sq >= 0)) return 0;
    const long long ex = (long long)e.z - e.x, ey = (long long)e.w - e.y;
    i128 num = (i128)ex * py - (i128)ey * px, den = (i128)ex * s.dy - (i128)ey * s.dx;      // den = sp - sq, not 0
    if (den < 0) { num = -num; den = -den; }
    t[0] = oc_param(num, den); kind[0] = 0;
    return 1;
}
// v + num d / den to the nearest step, halves toward +inf; 0 <= num <= den, |d| <= 2^30.  The quotient is at most |d|: found by bisection on 128-bit products
__device__ __forceinline__ int oc_coord(int v, long long d, const ulonglong2 t) {
    const u64 a = (u64)(d < 0 ? -d : d);
    const u128 N = (u128)t.x * a;
    u64 lo = 0, hi = a;                                                           // floor(N / den) is in [lo, hi]
    while (lo < hi) { const u64 mid = lo + (hi - lo + 1) / 2; if ((u128)mid * t.y <= N) lo = mid; else hi = mid - 1; }
    const u64 r = (u64)(N - (u128)lo * t.y);                                      // < den <= 2^63
    long long q = (long long)lo;
    if (d >= 0) return (int)(v + q + (2 * r >= t.y ? 1 : 0));
    if (r == 0) return (int)(v - q);
    return (int)(v - q - 1 + (2 * r <= t.y ? 1 : 0));                             // -q - r / den: floor is -q - 1, the remainder den - r
}
__device__ __forceinline__ int2 oc_point(const OcSeg& s, const ulonglong2 t) {
    if (t.x == 0) return s.A;
    if (t.x == t.y) return s.B;
    return make_int2(oc_coord(s.A.x, s.dx, t), oc_coord(s.A.y, s.dy, t));
}
__device__ __forceinline__ u64 oc_steps(const int2 a, const int2 b) {
    const long long dx = (long long)b.x - a.x, dy = (long long)b.y - a.y;
    const long long x = dx < 0 ? -dx : dx, y = dy < 0 ? -dy : dy;
    return (u64)(x > y ? x : y);
}
__device__ __forceinline__ bool oc_box_meets(const int4 b, const int2 A, const int2 B) {
    const int x0 = A.x < B.x ? A.x : B.x, x1 = A.x < B.x ? B.x : A.x, y0 = A.y < B.y ? A.y : B.y, y1 = A.y < B.y ? B.y : A.y;
    return b.x <= x1 && b.z >= x0 && b.y <= y1 && b.w >= y0;
}
// the first shape above the level
__device__ __forceinline__ int64_t oc_first_above(const int* __restrict__ slevel, int64_t ns, int lv) {
    int64_t lo = 0, hi = ns;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (slevel[mid] > lv) hi = mid; else lo = mid + 1; }
    return lo;
}

__global__ __launch_bounds__(256) void k_oc_rings(const long long* __restrict__ roff, int64_t m, int64_t R, const int* __restrict__ rsub, const long long* __restrict__ sv_off,
                                                  const double2* __restrict__ sv_pts, orip_gcode_map g, int clamp, int2* __restrict__ rpts, OcCounters* cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int64_t r = gc_path_of(roff, m, i);
    int2 o;
    const unsigned why = gc_ring_step(g, sv_pts[sv_off[rsub[r]] + (i - roff[r])], clamp, o);                  // gc_convert.h: shared with the hatch link
    if (why) atomicOr(&cn->bad, why == GC_RING_NOT_FINITE ? OC_BAD_NOT_FINITE : OC_BAD_RANGE);
    rpts[i] = o;
}
__global__ __launch_bounds__(256) void k_oc_boxinit(int4* __restrict__ sbox, int64_t ns) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < ns) sbox[s] = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
}
__global__ __launch_bounds__(256) void k_oc_edges(const long long* __restrict__ roff, int64_t m, int64_t R, const int2* __restrict__ rpts, const long long* __restrict__ spt,
                                                  int64_t ns, int4* __restrict__ edges, int4* sbox) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int64_t r = gc_path_of(roff, m, i), s = gc_path_of(spt, ns, i);
    const int2 P = rpts[i], Q = rpts[i + 1 < roff[r + 1] ? i + 1 : roff[r]];
    edges[i] = make_int4(P.x, P.y, Q.x, Q.y);
    int* const b = (int*)&sbox[s];
    atomicMin(b + 0, P.x); atomicMin(b + 1, P.y); atomicMax(b + 2, P.x); atomicMax(b + 3, P.y);
}

__global__ __launch_bounds__(256) void k_oc_cand(const long long* __restrict__ off, int64_t n, const int2* __restrict__ pts, int64_t total, const int* __restrict__ lvl, OcShapes sh,
                                                 int2* __restrict__ sinfo, unsigned* __restrict__ rec, unsigned* __restrict__ work, u64* __restrict__ evcnt, OcCounters* cn) {
    __shared__ u64 s_sum[2];                                                      // steps in, whole
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, S = total - n;
    if (i == 0) evcnt[S] = 0;
    if (i < total) {
        const int64_t p = gc_path_of(off, n, i);
        if (i > off[p]) {
            const int64_t g = i - 1 - p;
            const int2 A = pts[i - 1], B = pts[i];
            if (A.x == B.x && A.y == B.y) atomicOr(&cn->bad, OC_BAD_REPEAT);
            sinfo[g] = make_int2((int)i, (int)p);
            evcnt[g] = 0;
            atomicAdd(&s_sum[0], oc_steps(A, B));
            bool cand = false;
            for (int64_t s = oc_first_above(sh.slevel, sh.ns, lvl[p]); s < sh.ns && !cand; s++) cand = oc_box_meets(sh.sbox[s], A, B);
            if (cand) { const unsigned at = atomicAdd(&cn->n_work, 1u); if (at < (unsigned)S) work[at] = (unsigned)g; else atomicOr(&cn->bad, OC_BAD_LIST); rec[g] = 0; }
            else { rec[g] = 1u | OC_WHOLE | OC_FA | OC_FB; atomicAdd(&s_sum[1], 1ull); }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum[0]) atomicAdd(&cn->steps_in, s_sum[0]);
    if (threadIdx.x == 1 && s_sum[1]) atomicAdd(&cn->whole, s_sum[1]);
}

// the listed segment q of this wave: false when the list or the record is not what it must be
__device__ __forceinline__ bool oc_listed(unsigned q, int64_t S, int64_t total, int64_t n, const unsigned* __restrict__ work, const int2* __restrict__ sinfo,
                                          const int2* __restrict__ pts, unsigned& g, int& p, OcSeg& s) {
    g = work[q];
    if (g >= (unsigned)S) return false;
    const int2 si = sinfo[g];
    if (si.x < 1 || si.x >= total || si.y < 0 || si.y >= n) return false;
    p = si.y;
    s = oc_seg(pts[si.x - 1], pts[si.x]);
    return true;
}

__global__ __launch_bounds__(64) void k_oc_count(int64_t n, const int2* __restrict__ pts, int64_t total, const int* __restrict__ lvl, OcShapes sh, const int2* __restrict__ sinfo,
                                                 const unsigned* __restrict__ work, u64* __restrict__ evcnt, OcCounters* cn) {
    const int lane = threadIdx.x;
    const int64_t S = total - n;
    const unsigned count = cn->n_work < (unsigned)S ? cn->n_work : (unsigned)S;
    for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
        unsigned g; int p; OcSeg sg;
        if (!oc_listed(q, S, total, n, work, sinfo, pts, g, p, sg)) { if (lane == 0) atomicOr(&cn->bad, OC_BAD_LIST); continue; }
        u64 k = 0;
        for (int64_t s = oc_first_above(sh.slevel, sh.ns, lvl[p]); s < sh.ns; s++) {
            if (!oc_box_meets(sh.sbox[s], sg.A, sg.B)) continue;
            const int64_t e1 = sh.spt[s + 1];
            for (int64_t e = sh.spt[s] + lane; e < e1; e += 64) { ulonglong2 t[2]; int kind[2]; k += (u64)oc_events(sg, sh.edges[e], t, kind); }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) k += __shfl_xor(k, d, 64);
        if (lane == 0) evcnt[g] = k;
    }
}

// the event buffers; not __restrict__: lanes of the wave read what other lanes wrote, behind a barrier
struct OcEv { ulonglong2* ev_t; int* ev_k; ulonglong2* so_t; int* so_h; ulonglong2* iv_s; ulonglong2* iv_e; u64 E; };

__global__ __launch_bounds__(64) void k_oc_pieces(int64_t n, const int2* __restrict__ pts, int64_t total, const int* __restrict__ lvl, OcShapes sh, const int2* __restrict__ sinfo,
                                                  const unsigned* __restrict__ work, const u64* __restrict__ evcnt, const u64* __restrict__ evbase, OcEv ev, unsigned* __restrict__ rec,
                                                  OcCounters* cn) {
    const int lane = threadIdx.x;
    const int64_t S = total - n;
    const u64 below = (1ull << lane) - 1;
    const unsigned count = cn->n_work < (unsigned)S ? cn->n_work : (unsigned)S;
    for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {                    // q, and with it the segment, is the same in the whole block of one wave
        unsigned g; int p; OcSeg sg;
        if (!oc_listed(q, S, total, n, work, sinfo, pts, g, p, sg)) continue;     // k_oc_count has said so
        const u64 K = evcnt[g], base = evbase[g];
        if (K == 0) { if (lane == 0) { rec[g] = 1u | OC_WHOLE | OC_FA | OC_FB; atomicAdd(&cn->whole, 1ull); } continue; }
        if (base > ev.E || K > ev.E - base) { if (lane == 0) atomicOr(&cn->bad, OC_BAD_COUNT); continue; }
        ulonglong2 *const ev_t = ev.ev_t + base, *const so_t = ev.so_t + base, *const iv_s = ev.iv_s + base, *const iv_e = ev.iv_e + base;
        int *const ev_k = ev.ev_k + base, *const so_h = ev.so_h + base;
        u64 at = 0, I = 0;                                                        // events written, hidden stretches listed
        bool bad = false;
        for (int64_t s = oc_first_above(sh.slevel, sh.ns, lvl[p]); s < sh.ns; s++) {
            if (!oc_box_meets(sh.sbox[s], sg.A, sg.B)) continue;
            const u64 s0 = at;
            const int64_t e0 = sh.spt[s], e1 = sh.spt[s + 1];
            for (int64_t eb = e0; eb < e1; eb += 64) {                            // the shape's events, in edge order
                ulonglong2 t[2]; int kind[2]; int c = 0;
                if (eb + lane < e1) c = oc_events(sg, sh.edges[eb + lane], t, kind);
                const u64 m1 = __ballot(c >= 1), m2 = __ballot(c == 2);
                const u64 w = at + (u64)__popcll(m1 & below) + (u64)__popcll(m2 & below);
                if (w + (u64)c > K) bad = true;
                else for (int u = 0; u < c; u++) { ev_t[w + u] = t[u]; ev_k[w + u] = kind[u]; }
                at += (u64)__popcll(m1) + (u64)__popcll(m2);
            }
            if (__ballot(bad) || at > K) { bad = true; break; }
            __syncthreads();
            const u64 s1 = at;
            for (u64 i = s0 + lane; i < s1; i += 64) {                            // rank, and the state behind the event
                const ulonglong2 ti = ev_t[i];
                u64 rank = s0; int par = 0, blk = 0;
                for (u64 j = s0; j < s1; j++) {
                    const ulonglong2 tj = ev_t[j];
                    if (oc_lt(tj, ti) || (j <= i && oc_eq(tj, ti))) { const int kj = ev_k[j]; rank += j != i; par ^= kj == 0; blk += kj; }
                }
                so_t[rank] = ti; so_h[rank] = (par && blk == 0) ? 1 : 0;
            }
            __syncthreads();
            for (u64 b = s0; b + 1 < s1; b += 64) {                               // the hidden stretches, from a ranked event to the next
                const u64 i = b + lane;
                const bool hid = i + 1 < s1 && so_h[i] && oc_lt(so_t[i], so_t[i + 1]);
                const u64 mk = __ballot(hid);
                if (hid) { const u64 w = I + (u64)__popcll(mk & below); iv_s[w] = so_t[i]; iv_e[w] = so_t[i + 1]; }
                I += (u64)__popcll(mk);
            }
            __syncthreads();                                                      // the next shape writes behind s1, but ranks into so_t from there as well
        }
        if (bad || at != K || I >= K) { if (lane == 0) atomicOr(&cn->bad, OC_BAD_COUNT); continue; }
        if (I == 0) { if (lane == 0) { rec[g] = 1u | OC_WHOLE | OC_FA | OC_FB; atomicAdd(&cn->whole, 1ull); } continue; }
        ulonglong2 *const rs = ev_t, *const re = so_t;                            // the events are done with: the stretches ranked by (start, index)
        __syncthreads();
        for (u64 i = lane; i < I; i += 64) {
            const ulonglong2 ti = iv_s[i];
            u64 rank = 0;
            for (u64 j = 0; j < I; j++) { const ulonglong2 tj = iv_s[j]; if (oc_lt(tj, ti) || (j < i && oc_eq(tj, ti))) rank++; }
            rs[rank] = ti; re[rank] = iv_e[i];
        }
        __syncthreads();
        int4* const pc = (int4*)iv_s;                                             // the stretches are ranked: the kept pieces, in order
        ulonglong2 cover = make_ulonglong2(0, 1);
        u64 np = 0, nk = 0, col = 0, steps = 0;
        bool fa = false;
        for (u64 b = 0; b < I; b += 64) {
            const bool valid = b + lane < I;
            const ulonglong2 st = valid ? rs[b + lane] : make_ulonglong2(1, 1);
            ulonglong2 pm = valid ? re[b + lane] : make_ulonglong2(0, 1);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {                                    // the inclusive prefix maximum of the ends
                const ulonglong2 o = make_ulonglong2(__shfl_up(pm.x, d, 64), __shfl_up(pm.y, d, 64));
                if (lane >= d && oc_lt(pm, o)) pm = o;
            }
            ulonglong2 before = make_ulonglong2(__shfl_up(pm.x, 1, 64), __shfl_up(pm.y, 1, 64));
            if (lane == 0 || oc_lt(before, cover)) before = cover;                // how far everything in front of this lane's stretch hides
            const bool gap = valid && oc_lt(before, st);
            int2 P = make_int2(0, 0), Q = P;
            if (gap) { P = oc_point(sg, before); Q = oc_point(sg, st); }
            const bool kept = gap && (P.x != Q.x || P.y != Q.y);
            const u64 mg = __ballot(gap), mk = __ballot(kept);
            if (kept) { pc[nk + (u64)__popcll(mk & below)] = make_int4(P.x, P.y, Q.x, Q.y); steps += oc_steps(P, Q); }
            fa |= __ballot(kept && before.x == 0) != 0;                           // only the first piece starts at 0
            np += (u64)__popcll(mg); nk += (u64)__popcll(mk); col += (u64)__popcll(mg & ~mk);
            const ulonglong2 last = make_ulonglong2(__shfl(pm.x, 63, 64), __shfl(pm.y, 63, 64));
            if (oc_lt(cover, last)) cover = last;
        }
        bool fb = false;
        if (oc_lt(cover, make_ulonglong2(1, 1))) {                                // what is left behind the last stretch
            const int2 P = oc_point(sg, cover), Q = sg.B;
            np++;
            if (P.x != Q.x || P.y != Q.y) { if (lane == 0) { pc[nk] = make_int4(P.x, P.y, Q.x, Q.y); steps += oc_steps(P, Q); } nk++; fb = true; }
            else col++;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) steps += __shfl_xor(steps, d, 64);
        if (lane == 0) {
            if (nk > OC_NP || nk > K) { atomicOr(&cn->bad, OC_BAD_COUNT); rec[g] = 0; }
            else rec[g] = (unsigned)nk | (nk && fa ? OC_FA : 0u) | (nk && fb ? OC_FB : 0u);
            atomicAdd(np == 0 ? &cn->hidden : &cn->cut, 1ull);
            atomicAdd(&cn->pieces, np); atomicAdd(&cn->collapsed, col); atomicAdd(&cn->steps_out, steps);
        }
    }
}

__global__ __launch_bounds__(256) void k_oc_emit(int64_t S, int64_t total, int64_t n, const int2* __restrict__ pts, const unsigned* __restrict__ rec, const int2* __restrict__ sinfo,
                                                 const u64* __restrict__ cs, const u64* __restrict__ scan, const u64* __restrict__ evbase, const int4* __restrict__ pc, u64 E, GcCutOut o,
                                                 OcCounters* cn) {
    __shared__ u64 s_steps;
    if (threadIdx.x == 0) s_steps = 0;
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g == 0) gc_cut_close(o, scan[S]);
    if (g < S) {
        const unsigned r = rec[g], nk = r & OC_NP;
        const int2 si = sinfo[g];
        if (nk && (si.x < 1 || si.x >= total || si.y < 0 || si.y >= n || (!(r & OC_WHOLE) && (evbase[g] > E || nk > E - evbase[g])))) atomicOr(&cn->bad, OC_BAD_PLACE);
        else if (nk) {
            const bool cont = (unsigned)cs[g] == nk - 1;
            const long long pbase = (long long)(scan[g] >> 32), sbase = (long long)(unsigned)scan[g];
            u64 steps = 0;
            for (unsigned t = 0; t < nk; t++) {
                const int4 pq = (r & OC_WHOLE) ? make_int4(pts[si.x - 1].x, pts[si.x - 1].y, pts[si.x].x, pts[si.x].y) : pc[evbase[g] + t];
                if (!gc_cut_piece(o, pbase, sbase, cont, t, nk, si.y, make_int2(pq.x, pq.y), make_int2(pq.z, pq.w))) { atomicOr(&cn->bad, OC_BAD_PLACE); break; }
                if (r & OC_WHOLE) steps += oc_steps(make_int2(pq.x, pq.y), make_int2(pq.z, pq.w));
            }
            if (steps) atomicAdd(&s_steps, steps);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_steps) atomicAdd(&cn->steps_out, s_steps);          // the whole segments' steps: nobody else counted them
}

// the rings of one call: explicit in steps, or the resident fitted paths ring_sub of orip_svg_occlude
struct OcRings { const int64_t* off; const int32_t* pts; const int32_t* sub; const int32_t* level; int64_t m; const orip_gcode_map* map; int clamp; };

// both entry points behind their own checks of the strokes: the ring checks, then the pass.  `up_off` / `up_pts`: an explicit stroke list, uploaded once everything is checked
int oc_core(orip_ctx* c, const char* who, const int64_t* up_off, const int32_t* up_pts, const int32_t* level, int64_t n, int64_t total, const OcRings& rg, int64_t* stats) {
    const int64_t m = rg.m;
    if (m < 0 || m > (1 << 26)) ORIP_FAIL_AS(c, who, "%lld rings: 0..2^26", (long long)m);
    if ((n > 0 && !level) || (m > 0 && (!rg.level || (rg.sub ? false : !rg.off)))) ORIP_FAIL_AS(c, who, "bad arguments");
    for (int64_t k = 0; k < n; k++) if (level[k] < 0 || level[k] >= GC_COORD_MAX) ORIP_FAIL_AS(c, who, "stroke %lld: level %d outside 0..2^30 - 1", (long long)k, level[k]);
    for (int64_t r = 0; r < m; r++) {
        if (rg.level[r] < 0 || rg.level[r] >= GC_COORD_MAX) ORIP_FAIL_AS(c, who, "ring %lld: level %d outside 0..2^30 - 1", (long long)r, rg.level[r]);
        if (r && rg.level[r] < rg.level[r - 1]) ORIP_FAIL_AS(c, who, "ring %lld: level %d below the level before it (ring_level must not decrease)", (long long)r, rg.level[r]);
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
    std::vector<long long> spt; std::vector<int> slevel;                      // the shapes: runs of one level
    for (int64_t r = 0; r < m; r++) if (r == 0 || rg.level[r] != rg.level[r - 1]) { spt.push_back(roff[(size_t)r]); slevel.push_back(rg.level[r]); }
    const int64_t ns = (int64_t)slevel.size();
    spt.push_back(R);

    for (int k = 0; k < ORIP_OCCLUDE_STATS; k++) stats[k] = 0;
    if (n == 0) return gc_cut_empty(c, who, c->oc, up_off != nullptr);
    const int64_t S = total - n;
    const size_t Z = (size_t)S;
    int *lvl, *rsub, *d_slevel; long long *d_roff, *d_spt; int2 *rpts, *sinfo; int4 *edges, *sbox; unsigned *rec, *work; u64 *evs, *scans; OcCounters* cn;
    { Carve L; L.take(lvl, (size_t)n); L.take(d_roff, (size_t)m + 1); L.take(rsub, (size_t)m); L.take(rpts, (size_t)R); L.take(edges, (size_t)R); L.take(d_spt, (size_t)ns + 1);
      L.take(d_slevel, (size_t)ns); L.take(sbox, (size_t)ns); L.take(sinfo, Z); L.take(rec, Z); L.take(work, Z); L.take(evs, 2 * Z + 2); L.take(scans, 2 * Z + 2); L.take(cn, 1);
      HIPC_AS(c, who, L.commit(c->oc_tmp, 64)); }
    u64 *evcnt = evs, *evbase = evs + Z + 1, *cs = scans, *scan = scans + Z + 1;
    bool sources;
    ORIP_TRY(gc_cut_intake(c, who, c->oc, up_off, up_pts, n, total, sources));
    HIPC_AS(c, who, hipMemcpyAsync(lvl, level, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemcpyAsync(d_roff, roff.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemcpyAsync(d_spt, spt.data(), ((size_t)ns + 1) * 8, hipMemcpyHostToDevice, s));
    if (ns) HIPC_AS(c, who, hipMemcpyAsync(d_slevel, slevel.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemsetAsync(cn, 0, sizeof(OcCounters), s));
    const dim3 b(256), gs1(cdiv(S + 1, 256));
    if (R) {
        if (rg.sub) {
            HIPC_AS(c, who, hipMemcpyAsync(rsub, rg.sub, (size_t)m * 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_oc_rings, dim3(cdiv(R, 256)), b, 0, s, d_roff, m, R, rsub, c->sv_off.as<long long>(), c->sv_pts.as<double2>(), *rg.map, rg.clamp, rpts, cn);
        } else HIPC_AS(c, who, hipMemcpyAsync(rpts, rg.pts, (size_t)R * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_oc_boxinit, dim3(cdiv(ns, 256)), b, 0, s, sbox, ns);
        hipLaunchKernelGGL(k_oc_edges, dim3(cdiv(R, 256)), b, 0, s, d_roff, m, R, rpts, d_spt, ns, edges, sbox);
    }
    const long long* d_off = c->gc_off.as<long long>(); const int2* d_pts = c->gc_pts.as<int2>();
    const OcShapes sh = {d_spt, d_slevel, sbox, edges, ns};
    const int wblocks = (int)std::min<int64_t>(S, OC_BLOCKS);
    { ProfScope ps(c, "oc_cand");
      hipLaunchKernelGGL(k_oc_cand, dim3(cdiv(total, 256)), b, 0, s, d_off, n, d_pts, total, lvl, sh, sinfo, rec, work, evcnt, cn); }
    { ProfScope ps(c, "oc_count");
      hipLaunchKernelGGL(k_oc_count, dim3(wblocks), dim3(64), 0, s, n, d_pts, total, lvl, sh, sinfo, work, evcnt, cn);
      HIPC_AS(c, who, gc_scan_u64(c, evcnt, evbase, Z + 1)); }
    HIPC_AS(c, who, hipGetLastError());
    struct { u64 E; OcCounters cn; } h1;                                      // first read-back: the events, and what the conversion of the rings found
    HIPC_AS(c, who, hipMemcpyAsync(&h1.E, evbase + Z, 8, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipMemcpyAsync(&h1.cn, cn, sizeof(OcCounters), hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    if (h1.cn.bad & OC_BAD_NOT_FINITE) { gc_drop(c); ORIP_FAIL_AS(c, who, "a ring holds a coordinate that is not finite after the conversion to steps"); }
    if (h1.cn.bad & OC_BAD_RANGE) { gc_drop(c); ORIP_FAIL_AS(c, who, "a ring holds a point more than 2^30 steps off the sheet after the conversion to steps"); }
    if (h1.cn.bad & OC_BAD_REPEAT) { gc_drop(c); ORIP_FAIL_AS(c, who, "a resident polyline holds a point equal to the one before it"); }
    if (h1.cn.bad) { gc_drop(c); ORIP_FAIL_AS(c, who, "the work list does not add up (internal error %u)", h1.cn.bad); }
    const u64 E = h1.E;
    OcEv ev = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, E};
    { Carve L; L.take(ev.ev_t, (size_t)E); L.take(ev.so_t, (size_t)E); L.take(ev.iv_s, (size_t)E); L.take(ev.iv_e, (size_t)E); L.take(ev.ev_k, (size_t)E); L.take(ev.so_h, (size_t)E);
      HIPC_AS(c, who, L.commit(c->oc_ev, 64)); }
    if (h1.cn.n_work) { ProfScope ps(c, "oc_pieces");                         // a listed segment without an event is whole: the same kernel says so
      hipLaunchKernelGGL(k_oc_pieces, dim3(wblocks), dim3(64), 0, s, n, d_pts, total, lvl, sh, sinfo, work, evcnt, evbase, ev, rec, cn); }
    { ProfScope ps(c, "oc_compact");
      hipLaunchKernelGGL(k_gc_cut_compact, gs1, b, 0, s, S, rec, sinfo, cs);
      HIPC_AS(c, who, gc_scan_u64(c, cs, scan, Z + 1)); }
    HIPC_AS(c, who, hipGetLastError());
    u64 tot = 0;                                                              // second read-back: the size of the output
    HIPC_AS(c, who, hipMemcpyAsync(&tot, scan + Z, 8, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    int64_t paths, points;
    gc_cut_totals(tot, paths, points);
    if (points >= (int64_t)1 << 30) { gc_drop(c); ORIP_FAIL_AS(c, who, "%lld output points: fewer than 2^30", (long long)points); }
    ORIP_TRY(gc_cut_ensure(c, who, c->oc, paths, points));
    const GcCutOut o = gc_cut_out(c, c->oc, sources, points, paths);
    { ProfScope ps(c, "oc_emit");
      hipLaunchKernelGGL(k_oc_emit, gs1, b, 0, s, S, total, n, d_pts, rec, sinfo, cs, scan, evbase, (const int4*)ev.iv_s, E, o, cn); }
    HIPC_AS(c, who, hipGetLastError());
    OcCounters h;
    HIPC_AS(c, who, hipMemcpyAsync(&h, cn, sizeof(OcCounters), hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    const u64 pieces = h.pieces + h.whole;                                    // a whole segment is one piece; the wave kernel counts the others'
    if (h.bad || h.whole + h.cut + h.hidden != (u64)S || pieces < h.collapsed || (int64_t)(pieces - h.collapsed) != points - paths || 2 * paths > points) {
        gc_drop(c); ORIP_FAIL_AS(c, who, "the pieces do not add up (internal error %u)", h.bad);
    }
    gc_cut_publish(c, c->oc, sources, paths, points);                         // everything hidden: the list of no polylines
    stats[0] = S; stats[1] = (int64_t)h.whole; stats[2] = (int64_t)h.cut; stats[3] = (int64_t)h.hidden; stats[4] = (int64_t)pieces; stats[5] = (int64_t)h.collapsed;
    stats[6] = paths; stats[7] = points; stats[8] = (int64_t)h.steps_in; stats[9] = (int64_t)h.steps_out;
    return 0;
}
}  // namespace

// include/orip.h states the rule; the visible pieces become the resident step polylines
extern "C" int orip_gcode_occlude(orip_ctx* c, const int64_t* off, const int32_t* pts, const int32_t* level, int64_t n, const int64_t* ring_off, const int32_t* ring_pts,
                                  const int32_t* ring_level, int64_t m, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats) ORIP_FAIL(c, "bad arguments");
    int64_t total;
    ORIP_TRY(gc_steps_check(c, __func__, off, pts, n, true, total, 28));
    const OcRings rg = {ring_off, ring_pts, nullptr, ring_level, m, nullptr, 0};
    return oc_core(c, __func__, off, pts, level, n, total, rg, stats);
}

extern "C" int orip_svg_occlude(orip_ctx* c, const int32_t* level, int64_t n, const int32_t* ring_sub, const int32_t* ring_level, int64_t m, const orip_gcode_map* map,
                                int32_t flags, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats || !map || (m > 0 && !ring_sub)) ORIP_FAIL(c, "bad arguments");
    if (flags & ~ORIP_OCCLUDE_CLAMP) ORIP_FAIL(c, "unknown flags %d", flags);
    if (map->W < 1 || map->H < 1 || map->W > GC_COORD_MAX || map->H > GC_COORD_MAX) ORIP_FAIL(c, "target size %d x %d steps: each side must be in 1..2^30", map->W, map->H);
    int64_t total;
    ORIP_TRY(gc_steps_check(c, __func__, nullptr, nullptr, n, true, total, 28));
    static const int32_t none = 0;
    const OcRings rg = {nullptr, nullptr, ring_sub ? ring_sub : &none, ring_level, m, map, (flags & ORIP_OCCLUDE_CLAMP) ? 1 : 0};
    return oc_core(c, __func__, nullptr, nullptr, level, n, total, rg, stats);
}

extern "C" int orip_gcode_occlude_fetch(orip_ctx* c, int32_t* origin) { return gc_cut_fetch(c, __func__, c->oc, "the occlusion", origin); }
