// csrc/gcode_dedup.hip -- --dedup of gcode2stream.py / svg2stream.py: overlapping collinear segments of one pen are drawn once, the first drawn copy stays
// (orip_gcode_dedup; the rule is stated in include/orip.h, is exact in integers on the step grid and has one answer for every input).  Ours: the reference
// has no such pass on its vector front doors.
//
// A point ON A LINE is carried as one 64-bit word, (tau << 32) | other coordinate: words compare as tau compares, and a word unpacks into the grid point
// it came from, so a piece end is never computed, only copied.  SEGMENT g is the g-th segment of the drawing, strokes in order, S = points - strokes of them.
//
// 1. k_dd_keys, one thread per point (the point ends segment g unless it starts its stroke): the gcd, the LINE, the two end words in tau order, and the
//    three sort words  w0 = (group << 31) | lo   w1 = (ux << 32) | (uy + 2^30)   w2 = c + 2^62.
// 2. Three stable LSD passes of rocprim::radix_sort_pairs over the segment indices, w0 first, the next word gathered through the order so far: segments
//    sorted by (c, direction, group, lo, g); equal LINEs are contiguous and inside one the order is (lo, g).
// 3. k_dd_groups: the end words in sorted order, a head flag where the LINE changes; a scan numbers the lines, k_dd_lstart scatters where each begins, and
//    an inclusive scan by line number leaves pmax = the largest hi so far inside the line, whoever drew it.
// 4. Reach.  The positions of the line in front of k begin at or before lo, so of those only the earlier drawn count and only how far they reach:
//    k_dd_reach leaves reach[k] = max(lo, their largest hi).  One thread per segment walks backwards from k; it stops at hi, or where pmax says nothing
//    further reaches beyond what it has; and it steps over a whole block of 64 positions, or of 64 blocks (k_dd_blocks, k_dd_superblocks: largest hi and
//    lowest g of each), whose largest hi adds nothing or which was drawn later altogether.  pmax alone must not bound the search: it counts segments
//    drawn LATER, which cover nothing, and one long wall drawn behind m short ones on its line would send every short one over all the others, m^2 / 2
//    visits.  With the blocks that drawing costs each short one some 280 steps.  What stays quadratic: blocks that hold a far-reaching later segment
//    next to an earlier drawn one that reaches nowhere are walked position by position, and the forward sweep below over nested segments.
// 5. Survival, the same sweep run twice: COUNT (pieces, the two "still reaches its vertex" flags, pen-down steps) and, behind the compaction, EMIT.
//    For the segment at sorted position k the cover starts at reach[k] and the candidates are the positions (k, end) of its line, end = the first one
//    whose lo is not below hi (binary search).  Those with a lower g are taken in order, the running cover end kept; a candidate that begins beyond the
//    cover leaves a PIECE (cover, its lo); the sweep stops when the cover reaches hi, and what is left behind the last candidate is the last piece.
//    10^4 copies of one segment cost one look back each: the lowest g sorts first.
//      k_dd_survive, one THREAD per segment, looks at DD_THREAD_STEPS positions at most.  A segment it cannot finish within them is put on a list (count
//      pass; the emit pass finds the mark in its record) and left to
//      k_dd_long, one WAVE per listed segment: 64 positions per turn, the next turn's loads in flight, a wave prefix maximum of the candidates' hi, a
//      ballot of the gaps, the pieces numbered by the ballot's prefix count.
//    32 was chosen by measurement, on a long stroke over 10^5 earlier dashes and on 2 x 10^4 nested segments against a grid of squares; DESIGN 6 "dedup"
//    has the timings.
// 6. The cutting passes' compaction (gc_cut.h: k_gc_cut_compact, gc_scan_u64) places the points and numbers the strokes; the emit sweep writes every
//    piece where the scan says (gc_cut_piece): points, offsets, origin and the gathered sources.
// Everything on the calling lane's stream; one read-back (the counters, the scan's last word among them) and one host synchronisation, behind the last launch.
//
// Scratch in c->dd_tmp, free between calls, ONE Carve (orip_gcode_dedup): w0, w1, w2 u64[S]; ka u64[S] and kb u64[max(S, 2 (nb + nsb))], the sort's two key
// buffers and, once it is done, reach u64[S] and the DdSum[nb + nsb] of the blocks; idx unsigned[2 S] (the two index buffers of the sort); ends
// ulonglong2[S] (lo, hi words by g); sinfo int2[S] (forward, stroke); se ulonglong2[S] (the end words in sorted order); pmax u64[S]; lineid unsigned[S];
// lists unsigned[2 S + 1] (lstart[S + 1], then the long list); rec unsigned[S] (pieces | long << 29 | first piece starts at the first vertex << 30 | last
// piece ends at the second << 31; the head flags before that); grp int[n]; scans u64[2 S + 2] (cs, scan); DdCounters.  About 130 bytes per segment.
// Output: the record c->dd (gc_cut.h states the frame, orip_ctx.h the contract).
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>

#ifndef DD_THREAD_STEPS
#define DD_THREAD_STEPS 32            // positions one thread looks at before the segment goes to a wave
#endif

namespace {
typedef unsigned long long u64;
constexpr int DD_LONG_BLOCKS = 1024, DD_WAVES = 4;
constexpr unsigned DD_NP = GC_CUT_NP, DD_LONG = GC_CUT_OWN, DD_FA = GC_CUT_FA, DD_FB = GC_CUT_FB;        // the pass's own bit: a wave took the segment
constexpr unsigned DD_BAD_REPEAT = 1, DD_BAD_LINE = 2, DD_BAD_PLACE = 4, DD_BAD_LIST = 8;
struct DdCounters { u64 whole, cut, covered, pieces, steps_in, steps_out, tot; unsigned n_long, bad; };
struct DdSum { u64 maxhi; unsigned ming, pad; };                                      // of 64 sorted positions, or of 64 such blocks

__device__ __forceinline__ u64 dd_max(u64 a, u64 b) { return a > b ? a : b; }
// pen-down steps between two points of one line: max(|dx|, |dy|)
__device__ __forceinline__ u64 dd_steps(u64 s, u64 t) {
    const long long dt = (long long)(t >> 32) - (long long)(s >> 32), dv = (long long)(unsigned)t - (long long)(unsigned)s;
    const long long a = dt < 0 ? -dt : dt, b = dv < 0 ? -dv : dv;
    return (u64)(a > b ? a : b);
}
__device__ __forceinline__ int2 dd_point(u64 w, bool tau_is_x) { return tau_is_x ? make_int2((int)(w >> 32), (int)(unsigned)w) : make_int2((int)(unsigned)w, (int)(w >> 32)); }

__global__ __launch_bounds__(256) void k_dd_keys(const long long* __restrict__ off, int64_t n, const int2* __restrict__ pts, int64_t total, const int* __restrict__ grp,
                                                 u64* __restrict__ w0, u64* __restrict__ w1, u64* __restrict__ w2, unsigned* __restrict__ iota, ulonglong2* __restrict__ ends,
                                                 int2* __restrict__ sinfo, DdCounters* cn) {
    __shared__ u64 s_steps;
    if (threadIdx.x == 0) s_steps = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        const int64_t p = gc_path_of(off, n, i);
        if (i > off[p]) {                                                         // segment g: point i - 1 -> point i
            const int64_t g = i - 1 - p;
            const int2 a = pts[i - 1], b = pts[i];
            const long long dx = (long long)b.x - a.x, dy = (long long)b.y - a.y;
            unsigned m = (unsigned)(dx < 0 ? -dx : dx), r = (unsigned)(dy < 0 ? -dy : dy);
            const unsigned len = m > r ? m : r;
            while (r) { const unsigned t = m % r; m = r; r = t; }                 // m = gcd(|dx|, |dy|); 0 only for a repeated point
            long long ux = 0, uy = 0;
            if (m == 0) atomicOr(&cn->bad, DD_BAD_REPEAT);
            else { ux = dx / (long long)m; uy = dy / (long long)m; }
            if (ux < 0 || (ux == 0 && uy < 0)) { ux = -ux; uy = -uy; }
            const long long c = ux * a.y - uy * a.x;                              // |c| <= 2^61
            const bool tx = ux > 0;
            const u64 wa = tx ? ((u64)(unsigned)a.x << 32) | (unsigned)a.y : ((u64)(unsigned)a.y << 32) | (unsigned)a.x;
            const u64 wb = tx ? ((u64)(unsigned)b.x << 32) | (unsigned)b.y : ((u64)(unsigned)b.y << 32) | (unsigned)b.x;
            const bool fwd = wa < wb;
            const u64 lo = fwd ? wa : wb, hi = fwd ? wb : wa;
            w0[g] = ((u64)(unsigned)grp[p] << 31) | (lo >> 32);
            w1[g] = ((u64)ux << 32) | (u64)(uy + (1ll << 30));
            w2[g] = (u64)(c + (1ll << 62));
            iota[g] = (unsigned)g;
            ends[g] = make_ulonglong2(lo, hi);
            sinfo[g] = make_int2(fwd ? 1 : 0, (int)p);
            atomicAdd(&s_steps, (u64)len);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_steps) atomicAdd(&cn->steps_in, s_steps);
}

__global__ __launch_bounds__(256) void k_dd_gather(const u64* __restrict__ w, const unsigned* __restrict__ ord, int64_t S, u64* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < S) { const unsigned g = ord[k]; out[k] = g < (unsigned)S ? w[g] : 0; }
}

__global__ __launch_bounds__(256) void k_dd_groups(const u64* __restrict__ w0, const u64* __restrict__ w1, const u64* __restrict__ w2, const unsigned* __restrict__ ord, int64_t S,
                                                   const ulonglong2* __restrict__ ends, ulonglong2* __restrict__ se, unsigned* __restrict__ head, DdCounters* cn) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= S) return;
    const unsigned g = ord[k], gp = k ? ord[k - 1] : 0;
    if (g >= (unsigned)S || gp >= (unsigned)S) { atomicOr(&cn->bad, DD_BAD_LINE); se[k] = make_ulonglong2(0, 0); head[k] = 1; return; }
    se[k] = ends[g];
    head[k] = (k == 0 || w2[g] != w2[gp] || w1[g] != w1[gp] || (w0[g] >> 31) != (w0[gp] >> 31)) ? 1u : 0u;
}
// lstart[l] = the sorted position at which line l (0-based) begins; lstart[lines] = S
__global__ __launch_bounds__(256) void k_dd_lstart(const unsigned* __restrict__ head, const unsigned* __restrict__ lineid, int64_t S, unsigned* __restrict__ lstart) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= S) return;
    const unsigned l = lineid[k];
    if (l < 1 || l > (unsigned)S) return;
    if (head[k]) lstart[l - 1] = (unsigned)k;
    if (k == S - 1) lstart[l] = (unsigned)S;
}
struct DdHi { __device__ u64 operator()(const ulonglong2& e) const { return e.y; } };

// sum[b] = (largest hi, lowest g) of the sorted positions [64 b, 64 b + 64); behind the nb blocks, the same of 64 blocks each
__global__ __launch_bounds__(256) void k_dd_blocks(int64_t S, const unsigned* __restrict__ ord, const ulonglong2* __restrict__ se, DdSum* __restrict__ sum, int64_t nb) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    DdSum r = {0, ~0u, 0};
    const int64_t top = (b + 1) * 64 < S ? (b + 1) * 64 : S;
    for (int64_t j = b * 64; j < top; j++) { r.maxhi = dd_max(r.maxhi, se[j].y); r.ming = ord[j] < r.ming ? ord[j] : r.ming; }
    sum[b] = r;
}
__global__ __launch_bounds__(256) void k_dd_superblocks(DdSum* __restrict__ sum, int64_t nb, int64_t nsb) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nsb) return;
    DdSum r = {0, ~0u, 0};
    const int64_t top = (b + 1) * 64 < nb ? (b + 1) * 64 : nb;
    for (int64_t j = b * 64; j < top; j++) { r.maxhi = dd_max(r.maxhi, sum[j].maxhi); r.ming = sum[j].ming < r.ming ? sum[j].ming : r.ming; }
    sum[nb + b] = r;
}
// reach[k] = max(lo, the largest hi among the positions of the line in front of k that were drawn earlier): they begin at or before lo, so only how far they
// reach matters.  One thread per segment walks backwards from k and stops where the prefix maximum says that nothing further reaches beyond what it has, or
// at hi; a whole block of 64 positions, or of 64 blocks, is stepped over when its largest hi adds nothing or all of it was drawn later.  pmax alone would
// not do: it counts segments drawn LATER, which cover nothing, and one long wall drawn behind many short ones on its line would hold every search open.
__global__ __launch_bounds__(256) void k_dd_reach(int64_t S, const unsigned* __restrict__ ord, const ulonglong2* __restrict__ se, const u64* __restrict__ pmax,
                                                  const unsigned* __restrict__ lineid, const unsigned* __restrict__ lstart, const DdSum* __restrict__ sum, int64_t nb,
                                                  u64* __restrict__ reach, DdCounters* cn) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= S) return;
    const unsigned g = ord[k], l = lineid[k];
    const ulonglong2 e = se[k];
    u64 cover = e.x;
    const unsigned a = l >= 1 && l <= (unsigned)S ? lstart[l - 1] : ~0u;
    if (a > (unsigned)k) { atomicOr(&cn->bad, DD_BAD_LINE); reach[k] = cover; return; }
    unsigned j = (unsigned)k;                                                     // positions [a, j) are still to be looked at
    while (j > a && cover < e.y && pmax[j - 1] > cover) {
        if ((j & 63u) == 0 && j - a >= 64) {
            if ((j & 4095u) == 0 && j - a >= 4096) { const DdSum q = sum[nb + (j >> 12) - 1]; if (q.maxhi <= cover || q.ming > g) { j -= 4096; continue; } }
            const DdSum q = sum[(j >> 6) - 1];
            if (q.maxhi <= cover || q.ming > g) { j -= 64; continue; }
        }
        j--;
        if (ord[j] < g) cover = dd_max(cover, se[j].y);
    }
    reach[k] = cover;
}

// what both sweeps know of the segment at sorted position k
struct DdSeg { unsigned g, first, end, np_all, sbase; u64 lo, hi, cover0, pbase; bool fwd, tx, cont; int path; };
__device__ __forceinline__ bool dd_segment(int64_t k, int64_t S, const unsigned* __restrict__ ord, const ulonglong2* __restrict__ se, const u64* __restrict__ reach,
                                           const unsigned* __restrict__ lineid, const unsigned* __restrict__ lstart, const int2* __restrict__ sinfo, const u64* __restrict__ w1,
                                           DdSeg& s) {
    s.g = ord[k];
    const unsigned l = lineid[k];
    if (s.g >= (unsigned)S || l < 1 || l > (unsigned)S) return false;
    const unsigned a = lstart[l - 1], b = lstart[l];
    if (a > k || b <= k || b > (unsigned)S) return false;
    const ulonglong2 e = se[k];
    s.lo = e.x; s.hi = e.y;
    s.cover0 = reach[k];                                                          // what the line's positions in front of k cover of it (k_dd_reach)
    s.first = (unsigned)k + 1;
    unsigned x = s.first, y = b;
    while (x < y) { const unsigned mid = (x + y) >> 1; if (se[mid].x >= s.hi) y = mid; else x = mid + 1; }
    s.end = x;
    const int2 si = sinfo[s.g];
    s.fwd = si.x != 0; s.path = si.y; s.tx = (w1[s.g] >> 32) != 0;
    return true;
}
// where the emit sweep writes: the scan's word of the segment, and whether its first drawn piece continues the stroke of the segment before it
__device__ __forceinline__ void dd_place(DdSeg& s, const unsigned* __restrict__ rec, const u64* __restrict__ cs, const u64* __restrict__ scan) {
    s.np_all = rec[s.g] & DD_NP;
    s.cont = s.np_all > 0 && (unsigned)cs[s.g] == s.np_all - 1;
    s.pbase = scan[s.g] >> 32; s.sbase = (unsigned)scan[s.g];
}
// piece u of the segment in tau order, from word a to word b
__device__ __forceinline__ void dd_emit(const DdSeg& s, unsigned u, u64 a, u64 b, const GcCutOut& o, DdCounters* cn) {
    const unsigned t = s.fwd ? u : s.np_all - 1 - u;                              // its place in drawing order; beyond np_all when u is
    if (!gc_cut_piece(o, (long long)s.pbase, (long long)s.sbase, s.cont, t, s.np_all, s.path, dd_point(s.fwd ? a : b, s.tx), dd_point(s.fwd ? b : a, s.tx)))
        atomicOr(&cn->bad, DD_BAD_PLACE);
}
__device__ __forceinline__ unsigned dd_record(const DdSeg& s, unsigned np, bool flo, bool fhi) {
    const bool fa = s.fwd ? flo : fhi, fb = s.fwd ? fhi : flo;
    return np | (np && fa ? DD_FA : 0u) | (np && fb ? DD_FB : 0u);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_dd_survive(int64_t S, const unsigned* __restrict__ ord, const ulonglong2* __restrict__ se, const u64* __restrict__ reach,
                                                    const unsigned* __restrict__ lineid, const unsigned* __restrict__ lstart, const int2* __restrict__ sinfo, const u64* __restrict__ w1,
                                                    unsigned* __restrict__ rec, unsigned* __restrict__ longlist, const u64* __restrict__ cs, const u64* __restrict__ scan, GcCutOut o,
                                                    DdCounters* cn) {
    __shared__ u64 s_cnt[5];                                                      // whole, cut, covered, pieces, steps_out
    if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < S) {
        if (EMIT && k == 0) {                                                     // the closing offset, and the totals for the one read-back
            cn->tot = scan[S];
            gc_cut_close(o, scan[S]);
        }
        DdSeg s;
        if (!dd_segment(k, S, ord, se, reach, lineid, lstart, sinfo, w1, s)) atomicOr(&cn->bad, DD_BAD_LINE);
        else if (!EMIT || !(rec[s.g] & DD_LONG)) {
            if (EMIT) dd_place(s, rec, cs, scan);
            u64 cover = s.cover0, steps = 0;
            unsigned np = 0, j = s.first;
            bool flo = false;
            const unsigned stop = s.end - s.first > (unsigned)DD_THREAD_STEPS ? s.first + DD_THREAD_STEPS : s.end;
            for (; j < stop && cover < s.hi; j++) {
                if (ord[j] >= s.g) continue;                                      // drawn later
                const ulonglong2 e = se[j];
                if (e.x > cover) {
                    if (EMIT) dd_emit(s, np, cover, e.x, o, cn); else { steps += dd_steps(cover, e.x); flo |= cover == s.lo; }
                    np++;
                }
                cover = dd_max(cover, e.y);
            }
            if (cover < s.hi && j < s.end) {                                      // not finished within the thread's share: a wave takes it from the start
                if (!EMIT) {
                    const unsigned at = atomicAdd(&cn->n_long, 1u);
                    if (at < (unsigned)S) longlist[at] = (unsigned)k; else atomicOr(&cn->bad, DD_BAD_LIST);
                    rec[s.g] = DD_LONG;
                } else atomicOr(&cn->bad, DD_BAD_PLACE);                          // the count pass finished it and this one does not
            } else {
                const bool fhi = cover < s.hi;
                if (fhi) {
                    if (EMIT) dd_emit(s, np, cover, s.hi, o, cn); else { steps += dd_steps(cover, s.hi); flo |= cover == s.lo; }
                    np++;
                }
                if (!EMIT) {
                    rec[s.g] = dd_record(s, np, flo, fhi);
                    atomicAdd(&s_cnt[np == 0 ? 2 : (np == 1 && flo && fhi) ? 0 : 1], 1ull);
                    if (np) { atomicAdd(&s_cnt[3], (u64)np); atomicAdd(&s_cnt[4], steps); }
                } else if (np != s.np_all) atomicOr(&cn->bad, DD_BAD_PLACE);
            }
        }
    }
    __syncthreads();
    if (!EMIT && threadIdx.x < 5 && s_cnt[threadIdx.x]) {
        u64* const dst = threadIdx.x == 0 ? &cn->whole : threadIdx.x == 1 ? &cn->cut : threadIdx.x == 2 ? &cn->covered : threadIdx.x == 3 ? &cn->pieces : &cn->steps_out;
        atomicAdd(dst, s_cnt[threadIdx.x]);
    }
}

// the inclusive prefix maximum over the 64 lanes
__device__ __forceinline__ u64 dd_wave_prefix_max(u64 v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u64 o = __shfl_up(v, d, 64); if (lane >= d) v = dd_max(v, o); }
    return v;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_dd_long(int64_t S, const unsigned* __restrict__ ord, const ulonglong2* __restrict__ se, const u64* __restrict__ reach,
                                                 const unsigned* __restrict__ lineid, const unsigned* __restrict__ lstart, const int2* __restrict__ sinfo, const u64* __restrict__ w1,
                                                 unsigned* __restrict__ rec, const unsigned* __restrict__ longlist, const u64* __restrict__ cs, const u64* __restrict__ scan, GcCutOut o,
                                                 DdCounters* cn) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned count = cn->n_long < (unsigned)S ? cn->n_long : (unsigned)S;
    for (unsigned q = blockIdx.x * DD_WAVES + w; q < count; q += gridDim.x * DD_WAVES) {       // q, and with it the segment, is the same in the whole wave
        const unsigned k = longlist[q];
        DdSeg s;
        if (k >= (unsigned)S || !dd_segment(k, S, ord, se, reach, lineid, lstart, sinfo, w1, s)) { if (lane == 0) atomicOr(&cn->bad, DD_BAD_LIST); continue; }
        if (EMIT) dd_place(s, rec, cs, scan);
        u64 cover = s.cover0, steps = 0;
        unsigned np = 0;
        bool flo = false;
        // a turn's two loads do not wait for each other, and the next turn's are in flight while this one is worked on
        unsigned og = ~0u; ulonglong2 el = make_ulonglong2(~0ull, 0);
        if (s.first + lane < s.end) { og = ord[s.first + lane]; el = se[s.first + lane]; }
        for (unsigned base = s.first; base < s.end && cover < s.hi; base += 64) {
            const bool valid = og < s.g;
            const ulonglong2 e = valid ? el : make_ulonglong2(~0ull, 0);
            og = ~0u;
            if (base + 64 + lane < s.end) { og = ord[base + 64 + lane]; el = se[base + 64 + lane]; }
            const u64 pm = dd_wave_prefix_max(e.y, lane);
            u64 before = __shfl_up(pm, 1, 64);
            before = lane ? dd_max(cover, before) : cover;                        // the cover end in front of this lane's candidate
            const bool gap = valid && e.x > before;
            const u64 mask = __ballot(gap);
            if (gap) {
                const unsigned u = np + (unsigned)__popcll(mask & ((1ull << lane) - 1));
                if (EMIT) dd_emit(s, u, before, e.x, o, cn); else steps += dd_steps(before, e.x);
            }
            flo |= __ballot(gap && before == s.lo) != 0;
            np += (unsigned)__popcll(mask);
            cover = dd_max(cover, __shfl(pm, 63, 64));
        }
        const bool fhi = cover < s.hi;
        if (fhi) {
            if (lane == 0) { if (EMIT) dd_emit(s, np, cover, s.hi, o, cn); else steps += dd_steps(cover, s.hi); }
            flo |= cover == s.lo;
            np++;
        }
        if (!EMIT) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) steps += __shfl_xor(steps, m, 64);
            if (lane == 0) {
                rec[s.g] = dd_record(s, np, flo, fhi) | DD_LONG;
                atomicAdd(np == 0 ? &cn->covered : (np == 1 && flo && fhi) ? &cn->whole : &cn->cut, 1ull);
                atomicAdd(&cn->pieces, (u64)np); atomicAdd(&cn->steps_out, steps);
            }
        } else if (lane == 0 && np != s.np_all) atomicOr(&cn->bad, DD_BAD_PLACE);
    }
}

}  // namespace

// include/orip.h states the rule; the surviving strokes become the resident step polylines
extern "C" int orip_gcode_dedup(orip_ctx* c, const int64_t* off, const int32_t* pts, const int32_t* group, int64_t n, int32_t n_groups, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats) ORIP_FAIL(c, "bad arguments");
    int64_t total;
    ORIP_TRY(gc_steps_check(c, __func__, off, pts, n, true, total, 28));      // 2^28: a segment can leave two pieces, four points, and the output stays under 2^30
    ORIP_TRY(gc_check_groups(c, __func__, group, n, n_groups, nullptr));
    hipStream_t s = LN(c).stream;
    for (int k = 0; k < 9; k++) stats[k] = 0;
    if (n == 0) return gc_cut_empty(c, __func__, c->dd, off != nullptr);
    const int64_t S = total - n;                                              // segments: every path has two points or more, so n <= S
    const size_t Z = (size_t)S;
    const int64_t nb = (S + 63) / 64, nsb = (nb + 63) / 64;                   // blocks of 64 sorted positions, and of 64 blocks
    u64 *w0, *w1, *w2, *ka, *kb, *pmax, *scans; unsigned *idx, *lineid, *lists, *rec; ulonglong2 *ends, *se; int2* sinfo; int* grp; DdCounters* cn;
    { Carve L; L.each(Z, w0, w1, w2, ka); L.take(kb, std::max(Z, 2 * (size_t)(nb + nsb))); L.take(idx, 2 * Z); L.take(ends, Z); L.take(sinfo, Z); L.take(se, Z); L.take(pmax, Z); L.take(lineid, Z); L.take(lists, 2 * Z + 1);
      L.take(rec, Z); L.take(grp, (size_t)n); L.take(scans, 2 * Z + 2); L.take(cn, 1); HIPC(c, L.commit(c->dd_tmp, 64)); }
    unsigned *ia = idx, *ib = idx + Z, *lstart = lists, *longlist = lists + Z + 1; u64 *cs = scans, *scan = scans + Z + 1;
    const long long cap_paths = 2 * S, cap_pts = 4 * S;                       // pieces <= 2 segments: an end point cuts one later segment at most
    ORIP_TRY(gc_cut_ensure(c, __func__, c->dd, cap_paths, cap_pts));
    bool sources;
    ORIP_TRY(gc_cut_intake(c, __func__, c->dd, off, pts, n, total, sources));
    if (group) HIPC(c, hipMemcpyAsync(grp, group, (size_t)n * 4, hipMemcpyHostToDevice, s));
    else HIPC(c, hipMemsetAsync(grp, 0, (size_t)n * 4, s));
    HIPC(c, hipMemsetAsync(cn, 0, sizeof(DdCounters), s));
    HIPC(c, hipMemsetAsync(lstart, 0xFF, (Z + 1) * 4, s));                    // an entry nobody writes fails every bound check
    const long long* d_off = c->gc_off.as<long long>(); const int2* d_pts = c->gc_pts.as<int2>();
    const dim3 b(256), gs(cdiv(S, 256)), gs1(cdiv(S + 1, 256));
    { ProfScope ps(c, "dd_keys");
      hipLaunchKernelGGL(k_dd_keys, dim3(cdiv(total, 256)), b, 0, s, d_off, n, d_pts, total, grp, w0, w1, w2, ia, ends, sinfo, cn); }
    { ProfScope ps(c, "dd_sort");
      HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, w0, ka, ia, ib, Z, 0, 37, s); }));
      hipLaunchKernelGGL(k_dd_gather, gs, b, 0, s, w1, ib, S, kb);
      HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, kb, ka, ib, ia, Z, 0, 63, s); }));
      hipLaunchKernelGGL(k_dd_gather, gs, b, 0, s, w2, ia, S, kb);
      HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, kb, ka, ia, ib, Z, 0, 64, s); })); }
    const unsigned* ord = ib;
    { ProfScope ps(c, "dd_groups");
      hipLaunchKernelGGL(k_dd_groups, gs, b, 0, s, w0, w1, w2, ord, S, ends, se, rec, cn);
      HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::inclusive_scan(tmp, bytes, rec, lineid, Z, rocprim::plus<unsigned>(), s); }));
      hipLaunchKernelGGL(k_dd_lstart, gs, b, 0, s, rec, lineid, S, lstart);
      HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) {
          return rocprim::inclusive_scan_by_key(tmp, bytes, lineid, rocprim::make_transform_iterator(se, DdHi()), pmax, Z, rocprim::maximum<u64>(), rocprim::equal_to<unsigned>(), s); })); }
    u64* reach = ka; DdSum* sum = (DdSum*)kb;                                 // the sort is done with its two key buffers: their next roles
    { ProfScope ps(c, "dd_reach");
      hipLaunchKernelGGL(k_dd_blocks, dim3(cdiv(nb, 256)), b, 0, s, S, ord, se, sum, nb);
      hipLaunchKernelGGL(k_dd_superblocks, dim3(cdiv(nsb, 256)), b, 0, s, sum, nb, nsb);
      hipLaunchKernelGGL(k_dd_reach, gs, b, 0, s, S, ord, se, pmax, lineid, lstart, sum, nb, reach, cn); }
    const GcCutOut o = gc_cut_out(c, c->dd, sources, cap_pts, cap_paths);
    { ProfScope ps(c, "dd_survive");
      hipLaunchKernelGGL(k_dd_survive<false>, gs, b, 0, s, S, ord, se, reach, lineid, lstart, sinfo, w1, rec, longlist, cs, scan, o, cn);
      hipLaunchKernelGGL(k_dd_long<false>, dim3(DD_LONG_BLOCKS), b, 0, s, S, ord, se, reach, lineid, lstart, sinfo, w1, rec, longlist, cs, scan, o, cn); }
    { ProfScope ps(c, "dd_compact");
      hipLaunchKernelGGL(k_gc_cut_compact, gs1, b, 0, s, S, rec, sinfo, cs);
      HIPC(c, gc_scan_u64(c, cs, scan, Z + 1)); }
    { ProfScope ps(c, "dd_emit");
      hipLaunchKernelGGL(k_dd_survive<true>, gs, b, 0, s, S, ord, se, reach, lineid, lstart, sinfo, w1, rec, longlist, cs, scan, o, cn);
      hipLaunchKernelGGL(k_dd_long<true>, dim3(DD_LONG_BLOCKS), b, 0, s, S, ord, se, reach, lineid, lstart, sinfo, w1, rec, longlist, cs, scan, o, cn); }
    HIPC(c, hipGetLastError());
    DdCounters h;                                                             // the emit pass adds to nothing but `bad` and `tot`
    HIPC(c, hipMemcpyAsync(&h, cn, sizeof(DdCounters), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));                                         // the one read-back and the one sync, behind the last launch
    int64_t paths, points;
    gc_cut_totals(h.tot, paths, points);
    if (h.bad & DD_BAD_REPEAT) { gc_drop(c); ORIP_FAIL(c, "a resident polyline holds a point equal to the one before it"); }
    if (h.bad || h.whole + h.cut + h.covered != (u64)S || h.pieces > 2 * (u64)S || paths < 1 || paths > (int64_t)h.pieces || points != (int64_t)h.pieces + paths ||
        h.steps_out > h.steps_in) {
        gc_drop(c); ORIP_FAIL(c, "the pieces do not add up (internal error %u)", h.bad);
    }
    gc_cut_publish(c, c->dd, sources, paths, points);
    stats[0] = S; stats[1] = (int64_t)h.whole; stats[2] = (int64_t)h.cut; stats[3] = (int64_t)h.covered; stats[4] = (int64_t)h.pieces; stats[5] = paths; stats[6] = points;
    stats[7] = (int64_t)h.steps_in; stats[8] = (int64_t)h.steps_out;
    return 0;
}

extern "C" int orip_gcode_dedup_fetch(orip_ctx* c, int32_t* origin) { return gc_cut_fetch(c, __func__, c->dd, "orip_gcode_dedup", origin); }
