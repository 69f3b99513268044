// csrc/gcode_dash.hip -- --dashes of svg2stream.py / --dash-mm of gcode2stream.py: a stroke with a dash pattern is drawn as its dashes (orip_gcode_dash; the
// rule is stated in include/orip.h, is exact in integers on the step grid and has one answer for every input).  Ours: the reference has no such pass.
//
// Lengths are in u = 1/256 step.  POINT i is the i-th point of the drawing, strokes in order; the point that does not end its stroke heads SEGMENT i, i -> i + 1.
// A pattern of m entries is kept as its prefix sums A_0 = 0 .. A_m = P and the on-lengths On_t in front of every entry (the host builds both, ds_tables).
// BOUNDARY b of a stroke, b = r m + t, lies at the arc position r P + A_t - phase; even b begins a dash and odd b ends one, since m is even.
//
// 1. k_ds_len, one thread per point: l = floor(256 sqrt(D)) of the segment it heads (ds_isqrt: a double estimate, made exact on the 78-bit radicand), 0 for a
//    solid stroke, whose length nobody asks for, and for the stroke's last point; the high part l >> 20 goes beside it.  One exclusive scan over both halves:
//    S_j = X[i] - X[head of the stroke].  The low halves may wrap; the high halves cannot (2^28 points of 2^19 at most), and a stroke whose high halves add
//    up to less than 2^42 is shorter than 2^63, so its wrapped difference is its length (k_ds_count looks, per stroke: DS_BAD_LENGTH).
// 2. Everything about a segment follows from S_j and S_{j+1} alone (ds_segment).  With y = x + phase, the boundaries at or before x number
//    floor(y / P) m + #{t : A_t <= y mod P} (ds_pos: one 64-bit division and a search in A).  So the segment knows its CUT POINTS, the boundaries in
//    (S_j, S_{j+1}], by their first index and their number c, whether its head vertex lies strictly inside a dash (it is then a point of that dash), and
//    which of its points begin a dash.  The stroke's first vertex begins a dash when a dash runs from arc position 0; the last segment adds the last
//    vertex when a dash runs up to S_end, and leaves out a dash that would begin exactly there.  A solid stroke is one dash that never ends.
//    k_ds_count, one thread per point: cs[i] = (points << 32) | dashes begun; per stroke the length, the on-length (closed form again) and the counts,
//    summed over the wave, then over the block, then by one atomic per block and sum.
//    One 64-bit exclusive scan places every RAW point and numbers every raw dash.  FIRST READ-BACK: the totals R and Q, and what went wrong.
// 3. Emit, into the raw arrays: point, and (dash number | begins it << 31); the thread that begins a dash leaves its stroke in dpath.
//      k_ds_emit, one THREAD per segment, writes the head vertex, the closing vertex and up to DS_THREAD_CUTS cut points.  A segment with more was listed
//      by the count pass for
//      k_ds_emit_long, one WAVE per listed segment: lane e, e + 64, .. takes cut e.  A 2-point stroke cut into a thousand dashes is one such segment.
//    A cut point costs one division by m (32-bit), and per coordinate one 72-bit by 40-bit division: ds_round_div estimates the quotient in double and
//    corrects it against the exact 128-bit remainder, so no result of floating point is trusted.
// 4. Compaction.  k_ds_alive: a raw point that does not begin its dash and differs from the raw point before it marks its dash alive (a dash of one
//    distinct point has none: collapsed).  k_ds_flag: a point stays when it begins its dash or differs from the point before it, and its dash is alive;
//    cs2 = (1 << 32) | begins.  One more scan (gc_cut.h: gc_scan_u64, as the one of step 2), and k_ds_out writes points, offsets, origin and the
//    gathered sources (gc_cut_start, gc_cut_close).
// Everything on the calling lane's stream; two read-backs and two host synchronisations: behind the count (the raw arrays are sized by it) and behind the
// last launch.
//
// Scratch in c->ds_tmp, free between calls, ONE Carve (orip_gcode_dash): X DsLen[total + 1] twice (lengths, scanned); pat int[n], ph u64[n]; poff int[np + 1],
// A u64[E + np], On u64[E + np] (pattern q's tables start at poff[q] + q and hold its m + 1 prefixes); scans u64[2 total + 2] (cs, scan); longlist
// unsigned[total]; DsCounters.  c->ds_raw, ONE Carve behind the first read-back: rpts int2[R], rdid unsigned[R], dpath int[Q], alive unsigned[Q], scans
// u64[2 R + 2] (cs2, scan2).  Output: the record c->ds, sized by R and Q (gc_cut.h states the frame, orip_ctx.h the contract).
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>
#include <vector>

#ifndef DS_THREAD_CUTS
#define DS_THREAD_CUTS 24             // cut points one thread writes before the segment goes to a wave: by measurement, DESIGN 6 "dash" has the runs on both sides
#endif

namespace {
typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;
constexpr int DS_LONG_BLOCKS = 1024, DS_WAVES = 4;
constexpr unsigned DS_START = 1u << 31;
constexpr unsigned DS_BAD_REPEAT = 1, DS_BAD_LENGTH = 2, DS_BAD_MANY = 4, DS_BAD_PLACE = 8, DS_BAD_LIST = 16, DS_BAD_ORDER = 32;
constexpr u64 DS_LENGTH_MAX = 1ull << 62;
struct DsLen { u64 lo, hi; };                                                         // a length and its high part, summed side by side
struct DsAdd { __device__ DsLen operator()(const DsLen& a, const DsLen& b) const { return DsLen{a.lo + b.lo, a.hi + b.hi}; } };
struct DsCounters { u64 dashed, dashes, length_in, length_on, raw_points, tot; unsigned n_long, bad; };
struct DsTab { const int* pat; const u64* ph; const int* poff; const u64* A; const u64* On; };
struct DsPat { const u64* A; const u64* On; unsigned m; u64 P, ph; };                 // one stroke's pattern; m == 0: solid
struct DsPos { u64 r, rem; unsigned t; bool at; };                                    // of an arc position: period, place in it, boundaries of the period at or before it, on one
struct DsSeg { bool head, head_start, closing; u64 c, r0, x0, len; unsigned t0, ns; };
struct DsRaw { int2* pts; unsigned* did; int* dpath; long long R, Q; };

// floor(256 sqrt(D)), D <= 2^61: the double's estimate is within one of it, the two loops make it exact on the radicand D 2^16
__device__ __forceinline__ u64 ds_isqrt(u64 D) {
    const u128 R = (u128)D << 16;
    u64 r = (u64)(sqrt((double)D) * 256.0);
    while ((u128)r * r > R) r--;
    while ((u128)(r + 1) * (r + 1) <= R) r++;
    return r;
}
// floor((2 d t + l) / (2 l)), |d| <= 2^30, 0 < t < l < 2^39: the nearest step to d t / l, halves toward +infinity
__device__ __forceinline__ long long ds_round_div(long long d, u64 t, u64 l) {
    const i128 num = (i128)(2 * d) * (i128)t + (i128)l, den = (i128)(2 * l);
    long long q = (long long)floor((double)d * (double)t / (double)l + 0.5);
    i128 rem = num - (i128)q * den;
    while (rem < 0) { q--; rem += den; }
    while (rem >= den) { q++; rem -= den; }
    return q;
}
__device__ __forceinline__ DsPat ds_pattern(const DsTab& T, int64_t p) {
    const int q = T.pat[p];
    if (q < 0) return DsPat{nullptr, nullptr, 0, 1, 0};
    const int a = T.poff[q], m = T.poff[q + 1] - a;
    return DsPat{T.A + a + q, T.On + a + q, (unsigned)m, T.A[a + q + m], T.ph[p]};
}
__device__ __forceinline__ DsPos ds_pos(const DsPat& p, u64 x) {
    const u64 y = x + p.ph, r = y / p.P, rem = y - r * p.P;
    unsigned a = 0, b = p.m;                                                          // A[a] <= rem < A[b]
    while (b - a > 1) { const unsigned mid = (a + b) >> 1; if (p.A[mid] <= rem) a = mid; else b = mid; }
    return DsPos{r, rem, a + 1, p.A[a] == rem};
}
// the on-length of the pattern positions [0, x + phase]
__device__ __forceinline__ u64 ds_on(const DsPat& p, const DsPos& q) {
    const unsigned a = q.t - 1;
    return q.r * p.On[p.m] + p.On[a] + ((a & 1u) ? 0 : q.rem - p.A[a]);
}
// what segment [x0, x1] of a stroke emits: its head vertex, its cut points, the closing vertex
__device__ __forceinline__ bool ds_segment(const DsPat& p, u64 x0, u64 x1, bool first, bool last, DsSeg& s) {
    s.x0 = x0; s.len = x1 - x0;
    if (p.m == 0) { s.head = true; s.head_start = first; s.closing = last; s.c = 0; s.r0 = 0; s.t0 = 0; s.ns = first ? 1u : 0u; return true; }
    if (x1 <= x0) return false;
    const DsPos a = ds_pos(p, x0), b = ds_pos(p, x1);
    const bool on0 = (a.t & 1u) != 0, on1 = (b.t & 1u) != 0;
    s.head = on0 && (first || !a.at); s.head_start = s.head && first;
    s.c = (b.r - a.r) * p.m + b.t - a.t;
    if (last && on1 && b.at) s.c--;                                                   // a dash that would begin at the stroke's end
    s.closing = last && on1 && !b.at;
    s.r0 = a.r; s.t0 = a.t;
    if (s.c >= (1ull << 30)) return false;
    const unsigned g = s.t0 + (unsigned)s.c;
    s.ns = (s.head_start ? 1u : 0u) + ((g + 1) >> 1) - ((s.t0 + 1) >> 1);
    return true;
}
__device__ __forceinline__ void ds_put(const DsRaw& o, long long at, unsigned did, bool start, int2 pt, int path, DsCounters* cn) {
    if (at < 0 || at >= o.R || (long long)did >= o.Q) { atomicOr(&cn->bad, DS_BAD_PLACE); return; }
    o.pts[at] = pt; o.did[at] = did | (start ? DS_START : 0u);
    if (start) o.dpath[did] = path;
}
// cut e of the segment a -> b
__device__ __forceinline__ void ds_cut(const DsPat& p, const DsSeg& s, unsigned e, int2 a, int2 b, long long pbase, unsigned sbase, int path, const DsRaw& o, DsCounters* cn) {
    const unsigned g = s.t0 + e, k = g / p.m, ti = g - k * p.m;
    const u64 t = (s.r0 + k) * p.P + p.A[ti] - p.ph - s.x0;                           // in (0, len]
    if (t == 0 || t > s.len) { atomicOr(&cn->bad, DS_BAD_ORDER); return; }
    const int2 pt = t == s.len ? b : make_int2(a.x + (int)ds_round_div((long long)b.x - a.x, t, s.len), a.y + (int)ds_round_div((long long)b.y - a.y, t, s.len));
    const bool start = (g & 1u) == 0;
    const unsigned before = (s.head_start ? 1u : 0u) + ((g + 1) >> 1) - ((s.t0 + 1) >> 1);      // dashes begun in front of this cut
    if (!start && sbase + before == 0) { atomicOr(&cn->bad, DS_BAD_ORDER); return; }
    ds_put(o, pbase + (s.head ? 1 : 0) + e, start ? sbase + before : sbase + before - 1, start, pt, path, cn);
}

__global__ __launch_bounds__(256) void k_ds_len(const long long* __restrict__ off, int64_t n, const int2* __restrict__ pts, int64_t total, const int* __restrict__ pat,
                                                DsLen* __restrict__ len, DsCounters* cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > total) return;
    DsLen v = {0, 0};
    if (i < total) {
        const int64_t p = gc_path_of(off, n, i);
        if (i + 1 < off[p + 1]) {
            const int2 a = pts[i], b = pts[i + 1];
            const long long dx = (long long)b.x - a.x, dy = (long long)b.y - a.y;
            if (dx == 0 && dy == 0) atomicOr(&cn->bad, DS_BAD_REPEAT);
            else if (pat[p] >= 0) { v.lo = ds_isqrt((u64)(dx * dx) + (u64)(dy * dy)); v.hi = v.lo >> 20; }
        }
    }
    len[i] = v;
}

// what a thread knows of the segment point i heads; false: the point ends its stroke
__device__ __forceinline__ bool ds_load(const long long* __restrict__ off, int64_t n, int64_t i, const DsLen* __restrict__ X, const DsTab& T, int64_t& p, DsPat& pt, DsSeg& s,
                                        bool& first, DsCounters* cn) {
    p = gc_path_of(off, n, i);
    const int64_t h = off[p], e = off[p + 1];
    if (i + 1 >= e) return false;
    pt = ds_pattern(T, p);
    first = i == h;
    if (!ds_segment(pt, X[i].lo - X[h].lo, X[i + 1].lo - X[h].lo, first, i + 2 == e, s)) {
        atomicOr(&cn->bad, DS_BAD_MANY);
        s.head = s.head_start = s.closing = false; s.c = 0; s.ns = 0;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_ds_count(const long long* __restrict__ off, int64_t n, int64_t total, const DsLen* __restrict__ X, DsTab T, u64* __restrict__ cs,
                                                  unsigned* __restrict__ longlist, DsCounters* cn) {
    __shared__ u64 s_cnt[5];                                                      // dashed, dashes, length_in, length_on, raw points
    if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    u64 mine[5] = {0, 0, 0, 0, 0};                                                // this thread's share of the five sums
    if (i <= total) {
        u64 out = 0;
        int64_t p; DsPat pt; DsSeg s; bool first;
        if (i < total && ds_load(off, n, i, X, T, p, pt, s, first, cn)) {
            const u64 np = (s.head ? 1u : 0u) + s.c + (s.closing ? 1u : 0u);
            out = (np << 32) | s.ns;
            mine[4] = np;
            if (pt.m) mine[1] = s.ns;
            if (s.c > (u64)DS_THREAD_CUTS) {
                const unsigned at = atomicAdd(&cn->n_long, 1u);
                if (at < (unsigned)total) longlist[at] = (unsigned)i; else atomicOr(&cn->bad, DS_BAD_LIST);
            }
            if (first && pt.m) {                                                  // the stroke's own figures
                const int64_t e = off[p + 1] - 1;
                const u64 hi = X[e].hi - X[i].hi, S = X[e].lo - X[i].lo;
                if (hi >= (1ull << 42) || S >= DS_LENGTH_MAX) atomicOr(&cn->bad, DS_BAD_LENGTH);
                else {
                    mine[0] = 1; mine[2] = S;
                    mine[3] = ds_on(pt, ds_pos(pt, S)) - ds_on(pt, ds_pos(pt, 0));
                }
            }
        }
        cs[i] = out;
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {                                                 // summed over the wave first: one LDS atomic per wave and sum, one global per block
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mine[k] += __shfl_xor(mine[k], m, 64);
        if ((threadIdx.x & 63) == 0 && mine[k]) atomicAdd(&s_cnt[k], mine[k]);
    }
    __syncthreads();
    if (threadIdx.x < 5 && s_cnt[threadIdx.x]) {
        u64* const dst = threadIdx.x == 0 ? &cn->dashed : threadIdx.x == 1 ? &cn->dashes : threadIdx.x == 2 ? &cn->length_in : threadIdx.x == 3 ? &cn->length_on : &cn->raw_points;
        atomicAdd(dst, s_cnt[threadIdx.x]);
    }
}

__global__ __launch_bounds__(256) void k_ds_emit(const long long* __restrict__ off, int64_t n, const int2* __restrict__ pts, int64_t total, const DsLen* __restrict__ X, DsTab T,
                                                 const u64* __restrict__ scan, DsRaw o, DsCounters* cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int64_t p; DsPat pt; DsSeg s; bool first;
    if (!ds_load(off, n, i, X, T, p, pt, s, first, cn)) return;
    const long long pbase = (long long)(scan[i] >> 32); const unsigned sbase = (unsigned)scan[i];
    const int2 a = pts[i], b = pts[i + 1];
    if (s.head) {
        if (!s.head_start && sbase == 0) atomicOr(&cn->bad, DS_BAD_ORDER);
        else ds_put(o, pbase, s.head_start ? sbase : sbase - 1, s.head_start, a, (int)p, cn);
    }
    if (s.c <= (u64)DS_THREAD_CUTS)
        for (unsigned e = 0; e < (unsigned)s.c; e++) ds_cut(pt, s, e, a, b, pbase, sbase, (int)p, o, cn);
    if (s.closing) {
        if (sbase + s.ns == 0) atomicOr(&cn->bad, DS_BAD_ORDER);
        else ds_put(o, pbase + (s.head ? 1 : 0) + (long long)s.c, sbase + s.ns - 1, false, b, (int)p, cn);
    }
}

__global__ __launch_bounds__(256) void k_ds_emit_long(const long long* __restrict__ off, int64_t n, const int2* __restrict__ pts, int64_t total, const DsLen* __restrict__ X, DsTab T,
                                                      const u64* __restrict__ scan, const unsigned* __restrict__ longlist, DsRaw o, DsCounters* cn) {
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned count = cn->n_long < (unsigned)total ? cn->n_long : (unsigned)total;
    for (unsigned q = blockIdx.x * DS_WAVES + w; q < count; q += gridDim.x * DS_WAVES) {       // q, and with it the segment, is the same in the whole wave
        const int64_t i = longlist[q];
        int64_t p; DsPat pt; DsSeg s; bool first;
        if (i >= total || !ds_load(off, n, i, X, T, p, pt, s, first, cn) || s.c <= (u64)DS_THREAD_CUTS) { if (lane == 0) atomicOr(&cn->bad, DS_BAD_LIST); continue; }
        const long long pbase = (long long)(scan[i] >> 32); const unsigned sbase = (unsigned)scan[i];
        const int2 a = pts[i], b = pts[i + 1];
        for (unsigned e = lane; e < (unsigned)s.c; e += 64) ds_cut(pt, s, e, a, b, pbase, sbase, (int)p, o, cn);
    }
}

__device__ __forceinline__ bool ds_differs(const int2* __restrict__ pts, int64_t i) { const int2 a = pts[i - 1], b = pts[i]; return a.x != b.x || a.y != b.y; }

__global__ __launch_bounds__(256) void k_ds_alive(DsRaw o, unsigned* __restrict__ alive, DsCounters* cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= o.R) return;
    const unsigned w = o.did[i];
    if (w == ~0u) atomicOr(&cn->bad, DS_BAD_PLACE);                               // nobody wrote it
    if (w & DS_START) return;
    if (i == 0 || (long long)w >= o.Q) { atomicOr(&cn->bad, DS_BAD_ORDER); return; }
    if (ds_differs(o.pts, i)) alive[w] = 1u;
}
__device__ __forceinline__ bool ds_kept(const DsRaw& o, const unsigned* __restrict__ alive, int64_t i, bool& start) {
    const unsigned w = o.did[i], d = w & ~DS_START;
    start = (w & DS_START) != 0;
    if ((long long)d >= o.Q || (!start && i == 0)) return false;
    return alive[d] && (start || ds_differs(o.pts, i));
}
__global__ __launch_bounds__(256) void k_ds_flag(DsRaw o, const unsigned* __restrict__ alive, u64* __restrict__ cs2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > o.R) return;
    bool start = false;
    cs2[i] = i < o.R && ds_kept(o, alive, i, start) ? (1ull << 32) | (start ? 1u : 0u) : 0;
}
__global__ __launch_bounds__(256) void k_ds_out(DsRaw o, const unsigned* __restrict__ alive, const u64* __restrict__ scan2, GcCutOut out, DsCounters* cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= o.R) return;
    if (i == 0) {                                                                 // the closing offset, and the totals for the read-back
        const u64 tot = scan2[o.R];
        cn->tot = tot;
        gc_cut_close(out, tot);
    }
    bool start = false;
    if (!ds_kept(o, alive, i, start)) return;
    const long long at = (long long)(scan2[i] >> 32), sid = (long long)(unsigned)scan2[i] - (start ? 0 : 1);
    if (at >= out.cap_pts || sid < 0 || sid >= out.cap_paths) { atomicOr(&cn->bad, DS_BAD_PLACE); return; }
    out.pts[at] = o.pts[i];
    if (start) gc_cut_start(out, sid, at, o.dpath[o.did[i] & ~DS_START]);
}

// the pattern table, checked, as prefix sums: hA / hOn, pattern q at pat_off[q] + q
int ds_tables(orip_ctx* c, const char* who, const int32_t* pat_off, const int64_t* pat_val, int64_t np, std::vector<u64>& hA, std::vector<u64>& hOn) {
    if (pat_off[0] != 0) ORIP_FAIL_AS(c, who, "pat_off must start at 0");
    for (int64_t q = 0; q < np; q++) {
        const int64_t m = (int64_t)pat_off[q + 1] - pat_off[q];
        if (m < 2 || m > ORIP_DASH_MAX_ENTRIES || (m & 1)) ORIP_FAIL_AS(c, who, "pattern %lld has %lld entries: an even number in 2..%d", (long long)q, (long long)m, ORIP_DASH_MAX_ENTRIES);
    }
    if (np && !pat_val) ORIP_FAIL_AS(c, who, "bad arguments");
    hA.assign((size_t)pat_off[np] + (size_t)np, 0); hOn.assign(hA.size(), 0);
    for (int64_t q = 0; q < np; q++) {
        const size_t base = (size_t)pat_off[q] + (size_t)q; const int m = pat_off[q + 1] - pat_off[q];
        for (int t = 0; t < m; t++) {
            const int64_t v = pat_val[pat_off[q] + t];
            if (v < ORIP_DASH_UNIT || v > ((int64_t)1 << 40)) ORIP_FAIL_AS(c, who, "pattern %lld, entry %d: %lld outside %d..2^40 (1/%d step)", (long long)q, t, (long long)v, ORIP_DASH_UNIT, ORIP_DASH_UNIT);
            hA[base + t + 1] = hA[base + t] + (u64)v; hOn[base + t + 1] = hOn[base + t] + ((t & 1) ? 0 : (u64)v);
        }
    }
    return 0;
}
}  // namespace

// include/orip.h states the rule; the dashes become the resident step polylines
extern "C" int orip_gcode_dash(orip_ctx* c, const int64_t* off, const int32_t* pts, const int32_t* pattern, const int64_t* phase, int64_t n, const int32_t* pat_off,
                               const int64_t* pat_val, int32_t n_patterns, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats) ORIP_FAIL(c, "bad arguments");
    int64_t total;
    ORIP_TRY(gc_steps_check(c, __func__, off, pts, n, true, total, 28));
    const int64_t np = n_patterns;
    if (np < 0 || np > (1 << 20)) ORIP_FAIL(c, "%lld patterns: 0..2^20", (long long)np);
    if (!pat_off || (n > 0 && (!pattern || !phase))) ORIP_FAIL(c, "bad arguments");
    std::vector<u64> hA, hOn;
    ORIP_TRY(ds_tables(c, __func__, pat_off, pat_val, np, hA, hOn));
    for (int64_t k = 0; k < n; k++) {
        if (pattern[k] < -1 || pattern[k] >= np) ORIP_FAIL(c, "stroke %lld: pattern %d of %lld", (long long)k, pattern[k], (long long)np);
        if (pattern[k] >= 0) {
            const u64 P = hA[(size_t)pat_off[pattern[k] + 1] + (size_t)pattern[k]];
            if (phase[k] < 0 || (u64)phase[k] >= P) ORIP_FAIL(c, "stroke %lld: phase %lld outside [0, %llu)", (long long)k, (long long)phase[k], P);
        }
    }
    hipStream_t s = LN(c).stream;
    for (int k = 0; k < ORIP_DASH_STATS; k++) stats[k] = 0;
    if (n == 0) return gc_cut_empty(c, __func__, c->ds, off != nullptr);
    const size_t Z = (size_t)total, E = hA.size();
    DsLen *len, *X; int *d_pat, *d_poff; u64 *d_ph, *d_A, *d_On, *scans; unsigned* longlist; DsCounters* cn;
    { Carve L; L.each(Z + 1, len, X); L.take(d_pat, (size_t)n); L.take(d_ph, (size_t)n); L.take(d_poff, (size_t)np + 1); L.each(E + 1, d_A, d_On); L.take(scans, 2 * Z + 2);
      L.take(longlist, Z); L.take(cn, 1); HIPC(c, L.commit(c->ds_tmp, 64)); }
    u64 *cs = scans, *scan = scans + Z + 1;
    bool sources;
    ORIP_TRY(gc_cut_intake(c, __func__, c->ds, off, pts, n, total, sources));
    HIPC(c, hipMemcpyAsync(d_pat, pattern, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(d_ph, phase, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(d_poff, pat_off, ((size_t)np + 1) * 4, hipMemcpyHostToDevice, s));
    if (E) { HIPC(c, hipMemcpyAsync(d_A, hA.data(), E * 8, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_On, hOn.data(), E * 8, hipMemcpyHostToDevice, s)); }
    HIPC(c, hipMemsetAsync(cn, 0, sizeof(DsCounters), s));
    const long long* d_off = c->gc_off.as<long long>(); const int2* d_pts = c->gc_pts.as<int2>();
    const DsTab T = {d_pat, d_ph, d_poff, d_A, d_On};
    const dim3 b(256), gp(cdiv(total, 256)), gp1(cdiv(total + 1, 256));
    { ProfScope ps(c, "ds_len");
      hipLaunchKernelGGL(k_ds_len, gp1, b, 0, s, d_off, n, d_pts, total, d_pat, len, cn);
      HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, len, X, DsLen{0, 0}, Z + 1, DsAdd(), s); })); }
    { ProfScope ps(c, "ds_count");
      hipLaunchKernelGGL(k_ds_count, gp1, b, 0, s, d_off, n, total, X, T, cs, longlist, cn);
      HIPC(c, gc_scan_u64(c, cs, scan, Z + 1)); }
    HIPC(c, hipGetLastError());
    struct { u64 tot; DsCounters cn; } h1;                                    // first read-back: the size of the raw arrays, and what the count found
    HIPC(c, hipMemcpyAsync(&h1.tot, scan + Z, 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h1.cn, cn, sizeof(DsCounters), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (h1.cn.bad & DS_BAD_REPEAT) { gc_drop(c); ORIP_FAIL(c, "a resident polyline holds a point equal to the one before it"); }
    if (h1.cn.bad & DS_BAD_LENGTH) { gc_drop(c); ORIP_FAIL(c, "a dashed stroke is 2^62 units (2^54 steps) long or longer"); }
    if ((h1.cn.bad & DS_BAD_MANY) || h1.cn.raw_points >= (1ull << 30)) { gc_drop(c); ORIP_FAIL(c, "%llu output points or more: fewer than 2^30", h1.cn.raw_points); }
    const int64_t R = (int64_t)(h1.tot >> 32), Q = (int64_t)(h1.tot & 0xFFFFFFFFu);
    if (h1.cn.bad || (u64)R != h1.cn.raw_points || Q > R || h1.cn.dashed > (u64)n || h1.cn.length_on > h1.cn.length_in || Q - (n - (int64_t)h1.cn.dashed) != (int64_t)h1.cn.dashes) {
        gc_drop(c); ORIP_FAIL(c, "the count does not add up (internal error %u)", h1.cn.bad);
    }
    ORIP_TRY(gc_cut_ensure(c, __func__, c->ds, Q, R));
    int64_t paths = 0, points = 0;
    if (R == 0) HIPC(c, hipMemsetAsync(c->ds.off.p, 0, 8, s));                // every stroke lies in a gap: the list of no polylines
    else {
        DsRaw o = {nullptr, nullptr, nullptr, R, Q}; unsigned* alive; u64* scans2;
        { Carve L; L.take(o.pts, (size_t)R); L.take(o.did, (size_t)R); L.take(o.dpath, (size_t)Q); L.take(alive, (size_t)Q); L.take(scans2, 2 * (size_t)R + 2);
          HIPC(c, L.commit(c->ds_raw, 64)); }
        u64 *cs2 = scans2, *scan2 = scans2 + R + 1;
        HIPC(c, hipMemsetAsync(alive, 0, (size_t)Q * 4, s));
        HIPC(c, hipMemsetAsync(o.did, 0xFF, (size_t)R * 4, s));               // a raw point nobody writes fails every bound check
        const dim3 gr(cdiv(R, 256)), gr1(cdiv(R + 1, 256));
        { ProfScope ps(c, "ds_emit");
          hipLaunchKernelGGL(k_ds_emit, gp, b, 0, s, d_off, n, d_pts, total, X, T, scan, o, cn);
          if (h1.cn.n_long) hipLaunchKernelGGL(k_ds_emit_long, dim3((unsigned)std::min<u64>(DS_LONG_BLOCKS, cdiv(h1.cn.n_long, DS_WAVES))), b, 0, s, d_off, n, d_pts, total, X, T, scan, longlist, o, cn); }
        { ProfScope ps(c, "ds_compact");
          hipLaunchKernelGGL(k_ds_alive, gr, b, 0, s, o, alive, cn);
          hipLaunchKernelGGL(k_ds_flag, gr1, b, 0, s, o, alive, cs2);
          HIPC(c, gc_scan_u64(c, cs2, scan2, (size_t)R + 1));
          const GcCutOut out = gc_cut_out(c, c->ds, sources, R, Q);
          hipLaunchKernelGGL(k_ds_out, gr, b, 0, s, o, alive, scan2, out, cn); }
        HIPC(c, hipGetLastError());
        DsCounters h;                                                         // second read-back: the output's size, and what the emit found
        HIPC(c, hipMemcpyAsync(&h, cn, sizeof(DsCounters), hipMemcpyDeviceToHost, s));
        HIPC(c, hipStreamSynchronize(s));
        gc_cut_totals(h.tot, paths, points);
        if (h.bad || paths > Q || points > R || 2 * paths > points) { gc_drop(c); ORIP_FAIL(c, "the dashes do not add up (internal error %u)", h.bad); }
    }
    gc_cut_publish(c, c->ds, sources, paths, points);
    stats[0] = n; stats[1] = (int64_t)h1.cn.dashed; stats[2] = (int64_t)h1.cn.dashes; stats[3] = Q - paths; stats[4] = paths; stats[5] = points;
    stats[6] = (int64_t)h1.cn.length_in; stats[7] = (int64_t)h1.cn.length_on;
    return 0;
}

extern "C" int orip_gcode_dash_fetch(orip_ctx* c, int32_t* origin) { return gc_cut_fetch(c, __func__, c->ds, "orip_gcode_dash", origin); }
