// csrc/gcode_link.hip -- --hatch-connect of svg2stream.py: the lines of a hatch are drawn as zigzags, the links kept inside the shape (orip_gcode_hatch_link,
// orip_svg_hatch_link; the rule is stated in include/orip.h, is exact in integers on the step grid and has one answer for every input).  Ours: the
// reference has no such pass.
//
// A LINE is a stroke of exactly two points with cls >= 0; line j (0 .. nl - 1, in stroke order, so j ascends with the stroke) runs START -> END.  SHAPE s
// is the s-th distinct ring group, ascending: its rings, and with them its EDGES (edge i runs from ring point i to the next point of its ring, the first
// one behind the last), are contiguous because ring_group is sorted; a class finds its shape by binary search on the groups.
//
// 1. Rings, as the occlusion takes them: orip_svg_hatch_link gathers ring r from the resident fitted path ring_sub[r] and converts every point with
//    gc_ring_step (gc_convert.h); the offsets of the fitted paths are read back once for the ring sizes.  k_hl_edges, one thread per ring point: the edge.
// 2. Lines.  k_hl_flag marks them, a scan numbers them, the host reads nl (first read-back); k_hl_lines writes (START, END), class and stroke of every line
//    and the BUCKET KEY of its START: a 64-bit hash of (class, cell x, cell y) on a grid `reach` wide.  (class, cell) itself needs 91 bits, so the buckets
//    are sorted by the hash (rocPRIM radix sort, stable: a bucket lists its lines ascending) and a reader compares the whole triple, never the hash alone.
// 3. Pairs in reach.  One thread per END probes the 3 x 3 cells around its own: per cell a binary search for the hash, then the bucket's entries, each
//    tested for its own cell (two of the nine cells may share a hash: an entry counts only in the cell it lies in), the class, a < b and the distance.
//    k_hl_count counts, a scan places, the host reads the total P (second read-back; 2^30 pairs or more is refused) and sizes the pair list; k_hl_fill
//    runs the same probe again and writes (a, b).  A bucket of K lines costs every END near it K tests: nothing bounds K.
// 4. k_hl_elig, one WAVE per pair: the lanes stride over the edges of the pair's shape, each behind a box test; the inside parity of E is a ballot and a
//    popcount of the edges that cross the ray from E towards +x (half-open in y, so a vertex on the ray counts once), "meets an edge" is a wave-wide OR of
//    the closed segment test, which ends the stride early.  E on an edge meets that edge, so the parity only decides where E lies on none.  Orientations
//    are 128-bit.  Every shape takes this one path, a square of four edges as well: a thread per pair would be a second path to keep right.
// 5. Best and mutual.  (d^2, index) needs 41 + 26 bits, so it is TWO words and two passes: k_hl_elig takes atomicMin of d^2 per END and per START over its
//    eligible pairs, k_hl_best then atomicMin of the partner's index over the eligible pairs whose d^2 is that minimum.  Both are minima over a set, so
//    no order of the threads shows.  k_hl_mutual, one thread per END: a -> b is a link iff best(END a) = b and best(START b) = a.
// 6. Chains.  Links ascend, so chains are open and a chain's head is its lowest member.  Pointer jumping over prev, R rounds with 2^R >= nl fixed on the
//    host, ping-pong between two arrays of (pointer, head, members up to here, points up to here) as gcode_merge.hip jumps; a pointer still alive after R
//    rounds is an internal error.  The tail of a chain hands the totals to its head.
// 7. Emit.  Per stroke (points << 32 | 1, members) for a stroke that takes no part and for a head, zeros for any other line; two scans over the stroke
//    index number the output strokes, place their points and their member slots.  k_hl_emit, one thread per input point and per stroke, writes them through
//    the cutting passes' frame (gc_cut.h; origin = the first member, through which the sources are gathered).  The output is never larger than the input.
// Everything on the calling lane's stream; the third read-back fetches the totals and the counters behind the last launch.  Every index computed from device
// data is checked against its array before it is used; a miss sets HlCounters::bad and fails the call.
//
// Scratch, free between calls.  c->hl_tmp, ONE Carve: cls int[n]; roff long long[m + 1]; rsub int[m]; rpts int2[R]; edges int4[R]; gspt long long[ng + 1]
// (first ring point of every shape); ggrp int[ng]; flag, lidx u64[n + 1] (is a line, lines in front); cs u64[2][n + 1] (points << 32 | strokes, members) and
// sc u64[2][n + 1], their scans; HlCounters.  c->hl_ln, one Carve behind the first read-back: lp int4[nl] (START, END); lc, ls int[nl] (class, stroke); keys
// u64[2][nl], vals unsigned[2][nl] (unsorted, sorted); cnts u64[2][nl + 1] (pairs per END, their scan); bestd u64[2][nl], besti unsigned[2][nl] (per END, per
// START); link int[2][nl] (next, prev); J int4[2][nl]; tot int2[nl] (members, points of the chain, at its head).  c->hl_pair, one Carve behind the second:
// pairs uint2[P]; elig u8[P].  Resident: the record c->hl (orip_ctx.h states the contract), member_off / member in c->hl_res until the next call.
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <vector>

namespace {
typedef unsigned long long u64;
typedef __int128 i128;
constexpr int HL_BLOCKS = 16384;                                                      // one wave each; they stride over the pairs
constexpr unsigned HL_BAD_NOT_FINITE = 1, HL_BAD_RANGE = 2, HL_BAD_LIST = 4, HL_BAD_CHAIN = 8, HL_BAD_PLACE = 16;
struct HlCounters { u64 eligible, links, coincident, link_steps; unsigned bad; };
struct HlShapes { const long long* gspt; const int* ggrp; const int4* edges; int64_t ng; };
struct HlLines { const int4* lp; const int* lc; const u64* skey; const unsigned* sval; int nl; int reach; };

__device__ __forceinline__ u64 hl_hash(int cls, int gx, int gy) {
    u64 k = (((u64)(unsigned)gx << 32) | (unsigned)gy) * 0x9E3779B97F4A7C15ull + (u64)(unsigned)cls * 0xC2B2AE3D27D4EB4Full;
    k ^= k >> 32; k *= 0xD6E8FEB86659FD93ull; k ^= k >> 32;
    return k;
}
__device__ __forceinline__ int hl_sign(const int2 A, const int2 B, const int2 C) {   // of (B - A) x (C - A): up to 2^63 in magnitude
    const i128 v = (i128)((long long)B.x - A.x) * ((long long)C.y - A.y) - (i128)((long long)B.y - A.y) * ((long long)C.x - A.x);
    return v > 0 ? 1 : (v < 0 ? -1 : 0);
}
__device__ __forceinline__ bool hl_in_box(const int2 A, const int2 B, const int2 C) {  // C in the box of A and B
    return C.x >= min(A.x, B.x) && C.x <= max(A.x, B.x) && C.y >= min(A.y, B.y) && C.y <= max(A.y, B.y);
}
// the edge P -> Q crosses the ray from E towards +x; an end ON the ray's line counts as below it, so a vertex is counted once
__device__ __forceinline__ bool hl_crosses_ray(const int2 P, const int2 Q, const int2 E) {
    if ((P.y > E.y) == (Q.y > E.y)) return false;
    const int s = hl_sign(P, Q, E);
    return Q.y > P.y ? s > 0 : s < 0;
}
// the closed segments E S and P Q share a point; E == S is a segment of one point
__device__ __forceinline__ bool hl_meets(const int2 P, const int2 Q, const int2 E, const int2 S) {
    if (max(P.x, Q.x) < min(E.x, S.x) || min(P.x, Q.x) > max(E.x, S.x) || max(P.y, Q.y) < min(E.y, S.y) || min(P.y, Q.y) > max(E.y, S.y)) return false;
    const int d1 = hl_sign(P, Q, E), d2 = hl_sign(P, Q, S), d3 = hl_sign(E, S, P), d4 = hl_sign(E, S, Q);
    if (d1 * d2 < 0 && d3 * d4 < 0) return true;
    return (d1 == 0 && hl_in_box(P, Q, E)) || (d2 == 0 && hl_in_box(P, Q, S)) || (d3 == 0 && hl_in_box(E, S, P)) || (d4 == 0 && hl_in_box(E, S, Q));
}
__device__ __forceinline__ u64 hl_d2(const int4 a, const int4 b) {                    // END of a to START of b; in reach, so at most 2^41
    const long long dx = (long long)b.x - a.z, dy = (long long)b.y - a.w;
    return (u64)(dx * dx + dy * dy);
}

// ------------------------------------------------------------------------------------------------ 1. rings
__global__ __launch_bounds__(256) void k_hl_rings(const long long* __restrict__ roff, int64_t m, int64_t R, const int* __restrict__ rsub, const long long* __restrict__ sv_off,
                                                  const double2* __restrict__ sv_pts, orip_gcode_map g, int clamp, int2* __restrict__ rpts, HlCounters* cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int64_t r = gc_path_of(roff, m, i);
    int2 o;
    const unsigned why = gc_ring_step(g, sv_pts[sv_off[rsub[r]] + (i - roff[r])], clamp, o);
    if (why) atomicOr(&cn->bad, why == GC_RING_NOT_FINITE ? HL_BAD_NOT_FINITE : HL_BAD_RANGE);
    rpts[i] = o;
}
__global__ __launch_bounds__(256) void k_hl_edges(const long long* __restrict__ roff, int64_t m, int64_t R, const int2* __restrict__ rpts, int4* __restrict__ edges) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int64_t r = gc_path_of(roff, m, i);
    const int2 P = rpts[i], Q = rpts[i + 1 < roff[r + 1] ? i + 1 : roff[r]];
    edges[i] = make_int4(P.x, P.y, Q.x, Q.y);
}

// ------------------------------------------------------------------------------------------------ 2. lines
__global__ __launch_bounds__(256) void k_hl_flag(const long long* __restrict__ off, int64_t n, const int* __restrict__ cls, u64* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    flag[p] = p < n && off[p + 1] - off[p] == 2 && cls[p] >= 0 ? 1ull : 0ull;
}
__global__ __launch_bounds__(256) void k_hl_lines(const long long* __restrict__ off, const int2* __restrict__ pts, int64_t n, const int* __restrict__ cls, const u64* __restrict__ flag,
                                                  const u64* __restrict__ lidx, int nl, int reach, int4* __restrict__ lp, int* __restrict__ lc, int* __restrict__ ls,
                                                  u64* __restrict__ key, unsigned* __restrict__ val, HlCounters* cn) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n || !flag[p]) return;
    const u64 j = lidx[p];
    if (j >= (u64)nl) { atomicOr(&cn->bad, HL_BAD_LIST); return; }
    const int2 S = pts[off[p]], E = pts[off[p] + 1];
    lp[j] = make_int4(S.x, S.y, E.x, E.y); lc[j] = cls[p]; ls[j] = (int)p;
    key[j] = hl_hash(cls[p], S.x / reach, S.y / reach); val[j] = (unsigned)j;
}

// ------------------------------------------------------------------------------------------------ 3. pairs in reach
// found(b) for every line b whose START is in reach of the END of line a, b > a, of a's class: each once, in a fixed order
template <class F> __device__ __forceinline__ void hl_probe(const HlLines& L, int a, F&& found) {
    const int4 me = L.lp[a];
    const int c = L.lc[a], cx = me.z / L.reach, cy = me.w / L.reach;
    const long long reach = L.reach;
    for (int gy = cy - 1; gy <= cy + 1; gy++)
        for (int gx = cx - 1; gx <= cx + 1; gx++) {
            if (gx < 0 || gy < 0) continue;
            const u64 h = hl_hash(c, gx, gy);
            int lo = 0, hi = L.nl;
            while (lo < hi) { const int mid = (int)(((long long)lo + hi) >> 1); if (L.skey[mid] < h) lo = mid + 1; else hi = mid; }
            for (int k = lo; k < L.nl && L.skey[k] == h; k++) {
                const unsigned b = L.sval[k];
                if (b >= (unsigned)L.nl || (int)b <= a) continue;
                const int4 o = L.lp[b];
                if (L.lc[b] != c || o.x / L.reach != gx || o.y / L.reach != gy) continue;      // the whole triple, never a hash of it
                const long long dx = (long long)o.x - me.z, dy = (long long)o.y - me.w;
                if (dx > reach || dx < -reach || dy > reach || dy < -reach || dx * dx + dy * dy > reach * reach) continue;
                found(b);
            }
        }
}
__global__ __launch_bounds__(256) void k_hl_count(HlLines L, u64* __restrict__ cnt) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a > L.nl) return;
    u64 k = 0;
    if (a < L.nl) hl_probe(L, a, [&](unsigned) { k++; });
    cnt[a] = k;
}
__global__ __launch_bounds__(256) void k_hl_fill(HlLines L, const u64* __restrict__ cnt, const u64* __restrict__ base, u64 P, uint2* __restrict__ pairs, HlCounters* cn) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= L.nl) return;
    const u64 at = base[a], k1 = cnt[a];
    if (at > P || k1 > P - at) { atomicOr(&cn->bad, HL_BAD_LIST); return; }
    u64 k = 0;
    hl_probe(L, a, [&](unsigned b) { if (k < k1) pairs[at + k] = make_uint2((unsigned)a, b); k++; });
    if (k != k1) atomicOr(&cn->bad, HL_BAD_LIST);
}

// ------------------------------------------------------------------------------------------------ 4. eligibility, and the least d^2 per END and per START
__global__ __launch_bounds__(64) void k_hl_elig(u64 P, const uint2* __restrict__ pairs, int nl, const int4* __restrict__ lp, const int* __restrict__ lc, HlShapes sh,
                                                uint8_t* __restrict__ elig, u64* bestd, HlCounters* cn) {
    const int lane = threadIdx.x;
    for (u64 q = blockIdx.x; q < P; q += gridDim.x) {                             // q, and with it the pair, is the same in the whole block of one wave
        const uint2 pr = pairs[q];
        if (pr.x >= (unsigned)nl || pr.y >= (unsigned)nl) { if (lane == 0) { atomicOr(&cn->bad, HL_BAD_LIST); elig[q] = 0; } continue; }
        const int4 la = lp[pr.x], lb = lp[pr.y];
        const int2 E = make_int2(la.z, la.w), S = make_int2(lb.x, lb.y);
        const int g = lc[pr.x] >> 1;
        int64_t lo = 0, hi = sh.ng;                                               // the shape of the class: the first group not below g
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (sh.ggrp[mid] < g) lo = mid + 1; else hi = mid; }
        const bool shape = lo < sh.ng && sh.ggrp[lo] == g;
        bool par = false, meets = false;
        if (shape) {
            const int64_t e1 = sh.gspt[lo + 1];
            for (int64_t eb = sh.gspt[lo]; eb < e1; eb += 64) {
                if (eb + lane < e1) {
                    const int4 e = sh.edges[eb + lane];
                    const int2 A = make_int2(e.x, e.y), B = make_int2(e.z, e.w);
                    if (A.x != B.x || A.y != B.y) { par ^= hl_crosses_ray(A, B, E); meets = meets || hl_meets(A, B, E, S); }
                }
                if (__ballot(meets)) break;
            }
        }
        const bool any = __ballot(meets) != 0, inside = (__popcll(__ballot(par)) & 1) != 0;
        if (lane == 0) {
            const bool ok = shape && inside && !any;
            elig[q] = ok ? 1 : 0;
            if (ok) { const u64 d2 = hl_d2(la, lb); atomicMin(&bestd[pr.x], d2); atomicMin(&bestd[(size_t)nl + pr.y], d2); atomicAdd(&cn->eligible, 1ull); }
        }
    }
}

// ------------------------------------------------------------------------------------------------ 5. best and mutual
__global__ __launch_bounds__(256) void k_hl_best(u64 P, const uint2* __restrict__ pairs, const uint8_t* __restrict__ elig, int nl, const int4* __restrict__ lp,
                                                 const u64* __restrict__ bestd, unsigned* besti) {
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q >= P || !elig[q]) return;
    const uint2 pr = pairs[q];                                                    // k_hl_elig has checked it: an eligible pair names two lines
    const u64 d2 = hl_d2(lp[pr.x], lp[pr.y]);
    if (d2 == bestd[pr.x]) atomicMin(&besti[pr.x], pr.y);
    if (d2 == bestd[(size_t)nl + pr.y]) atomicMin(&besti[(size_t)nl + pr.y], pr.x);
}
__global__ __launch_bounds__(256) void k_hl_mutual(int nl, const int4* __restrict__ lp, const unsigned* __restrict__ besti, int* __restrict__ link, HlCounters* cn) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= nl) return;
    const unsigned b = besti[a];
    if (b >= (unsigned)nl || (int)b <= a || besti[(size_t)nl + b] != (unsigned)a) return;
    link[a] = (int)b; link[(size_t)nl + b] = a;                                   // next, prev: only a is b's best, so nobody else writes prev[b]
    const int4 la = lp[a], lb = lp[b];
    const long long dx = (long long)lb.x - la.z, dy = (long long)lb.y - la.w, x = dx < 0 ? -dx : dx, y = dy < 0 ? -dy : dy;
    atomicAdd(&cn->links, 1ull);
    if (x == 0 && y == 0) atomicAdd(&cn->coincident, 1ull);
    else atomicAdd(&cn->link_steps, (u64)(x > y ? x : y));
}

// ------------------------------------------------------------------------------------------------ 6. chains
// the START of line j equals the END of the line linked in front of it: the point is written once
__device__ __forceinline__ bool hl_coincident(const int4* __restrict__ lp, int p, int j) { return p >= 0 && lp[p].z == lp[j].x && lp[p].w == lp[j].y; }

__global__ __launch_bounds__(256) void k_hl_chain0(int nl, const int4* __restrict__ lp, const int* __restrict__ link, int4* __restrict__ J, HlCounters* cn) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nl) return;
    int p = link[(size_t)nl + j];
    if (p >= j) { atomicOr(&cn->bad, HL_BAD_CHAIN); p = -1; }                     // links ascend
    J[j] = make_int4(p, j, 1, hl_coincident(lp, p, j) ? 1 : 2);
}
__global__ __launch_bounds__(256) void k_hl_jump(const int4* __restrict__ A, int4* __restrict__ B, int nl) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nl) return;
    int4 a = A[t];
    if ((unsigned)a.x < (unsigned)nl) {
        const int4 b = A[a.x];
        a.x = b.x; a.y = min(a.y, b.y); a.z = (int)((unsigned)a.z + (unsigned)b.z); a.w = (int)((unsigned)a.w + (unsigned)b.w);
    }
    B[t] = a;
}
__global__ __launch_bounds__(256) void k_hl_tails(int nl, const int* __restrict__ link, const int4* __restrict__ J, int2* __restrict__ tot, HlCounters* cn) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nl) return;
    const int4 a = J[j];
    if (a.x != -1 || (unsigned)a.y >= (unsigned)nl) { atomicOr(&cn->bad, HL_BAD_CHAIN); return; }
    if (link[j] < 0) tot[a.y] = make_int2(a.z, a.w);                              // one tail per chain
}

// ------------------------------------------------------------------------------------------------ 7. emit
__global__ __launch_bounds__(256) void k_hl_heads(const long long* __restrict__ off, int64_t n, const u64* __restrict__ flag, const u64* __restrict__ lidx, int nl,
                                                  const int* __restrict__ link, const int2* __restrict__ tot, u64* __restrict__ cs, HlCounters* cn) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    u64 a = 0, b = 0;
    if (p < n && !flag[p]) { a = ((u64)(off[p + 1] - off[p]) << 32) | 1ull; b = 1; }
    else if (p < n) {
        const u64 j = lidx[p];
        if (j >= (u64)nl) atomicOr(&cn->bad, HL_BAD_LIST);
        else if (link[(size_t)nl + j] < 0) {
            const int2 t = tot[j];
            if (t.x < 1 || t.y < 2) atomicOr(&cn->bad, HL_BAD_CHAIN);
            else { a = ((u64)(unsigned)t.y << 32) | 1ull; b = (u64)(unsigned)t.x; }
        }
    }
    cs[p] = a; cs[(size_t)(n + 1) + p] = b;
}
__global__ __launch_bounds__(256) void k_hl_emit(const long long* __restrict__ off, const int2* __restrict__ pts, int64_t n, int64_t total, const u64* __restrict__ flag,
                                                 const u64* __restrict__ lidx, int nl, const int4* __restrict__ lp, const int* __restrict__ ls, const int* __restrict__ link,
                                                 const int4* __restrict__ J, const u64* __restrict__ sc, GcCutOut o, long long* __restrict__ member_off, int* __restrict__ member,
                                                 HlCounters* cn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const u64* sc1 = sc; const u64* sc2 = sc + (size_t)(n + 1);
    if (i == n) {                                                                 // the closing offsets
        gc_cut_close(o, sc1[n]);
        if ((long long)(unsigned)sc1[n] <= o.cap_paths) member_off[(unsigned)sc1[n]] = (long long)sc2[n]; else atomicOr(&cn->bad, HL_BAD_PLACE);
    }
    if (i < n) {                                                                  // stroke i: its member slot, and its output stroke when it starts one
        const int64_t p = i;
        int64_t first = p; u64 rank = 0; bool starts = true;
        if (flag[p]) {
            const u64 j = lidx[p];
            if (j >= (u64)nl) { atomicOr(&cn->bad, HL_BAD_LIST); first = -1; }
            else { const int4 a = J[j]; first = (unsigned)a.y < (unsigned)nl ? ls[a.y] : -1; rank = (u64)(unsigned)a.z - 1; starts = link[(size_t)nl + j] < 0; }
        }
        if (first < 0 || first >= n || sc2[first] + rank >= (u64)n) atomicOr(&cn->bad, HL_BAD_PLACE);
        else {
            member[sc2[first] + rank] = (int)p;
            if (starts) {
                const long long sid = (long long)(unsigned)sc1[p], at = (long long)(sc1[p] >> 32);
                if (sid >= o.cap_paths || at + 2 > o.cap_pts) atomicOr(&cn->bad, HL_BAD_PLACE);
                else { gc_cut_start(o, sid, at, (int)p); member_off[sid] = (long long)sc2[p]; }
            }
        }
    }
    if (i >= total) return;
    const int64_t p = gc_path_of(off, n, i);                                      // every stroke has points, so this is the stroke of point i
    long long dst;
    if (!flag[p]) dst = (long long)(sc1[p] >> 32) + (i - off[p]);
    else {
        const u64 j = lidx[p];
        if (j >= (u64)nl) return;                                                 // said above
        const int4 a = J[j];
        if ((unsigned)a.y >= (unsigned)nl) return;
        const int first = ls[a.y];
        if (first < 0 || first >= n) return;
        const int own = hl_coincident(lp, link[(size_t)nl + j], (int)j) ? 1 : 2;
        const long long before = (long long)(unsigned)a.w - own;                 // points of the chain in front of this line
        if (i == off[p]) { if (own == 1) return; dst = (long long)(sc1[first] >> 32) + before; }
        else dst = (long long)(sc1[first] >> 32) + before + own - 1;
    }
    if (dst < 0 || dst >= o.cap_pts) { atomicOr(&cn->bad, HL_BAD_PLACE); return; }
    o.pts[dst] = pts[i];
}

// the rings of one call: explicit in steps, or the resident fitted paths ring_sub of orip_svg_hatch_link
struct HlRings { const int64_t* off; const int32_t* pts; const int32_t* sub; const int32_t* group; int64_t m; const orip_gcode_map* map; int clamp; };

// both entry points behind their own checks of the strokes: the other checks, then the pass.  `up_off` / `up_pts`: an explicit stroke list, uploaded once everything is checked
int hl_core(orip_ctx* c, const char* who, const int64_t* up_off, const int32_t* up_pts, const int32_t* cls, int64_t n, int64_t total, const HlRings& rg, int32_t reach, int64_t* stats) {
    const int64_t m = rg.m;
    if (reach < 1 || reach > ORIP_HATCH_LINK_REACH_MAX) ORIP_FAIL_AS(c, who, "reach %d: 1..2^20", reach);
    if (m < 0 || m > (1 << 26)) ORIP_FAIL_AS(c, who, "%lld rings: 0..2^26", (long long)m);
    if ((n > 0 && !cls) || (m > 0 && (!rg.group || (rg.sub ? false : !rg.off)))) ORIP_FAIL_AS(c, who, "bad arguments");
    for (int64_t k = 0; k < n; k++) if (cls[k] < -1) ORIP_FAIL_AS(c, who, "stroke %lld: class %d below -1", (long long)k, cls[k]);
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
    std::vector<long long> gspt; std::vector<int> ggrp;                       // the shapes: runs of one group
    for (int64_t r = 0; r < m; r++) if (r == 0 || rg.group[r] != rg.group[r - 1]) { gspt.push_back(roff[(size_t)r]); ggrp.push_back(rg.group[r]); }
    const int64_t ng = (int64_t)ggrp.size();
    gspt.push_back(R);

    for (int k = 0; k < ORIP_HATCH_LINK_STATS; k++) stats[k] = 0;
    if (n == 0) { ORIP_TRY(gc_cut_empty(c, who, c->hl, up_off != nullptr)); c->hl_n = 0; c->hl_paths = 0; return 0; }
    const size_t N1 = (size_t)n + 1;
    int *d_cls, *rsub, *d_ggrp; long long *d_roff, *d_gspt; int2* rpts; int4* edges; u64 *flag, *lidx, *cs, *sc; HlCounters* cn;
    { Carve L; L.take(d_cls, (size_t)n); L.take(d_roff, (size_t)m + 1); L.take(rsub, (size_t)m); L.take(rpts, (size_t)R); L.take(edges, (size_t)R); L.take(d_gspt, (size_t)ng + 1);
      L.take(d_ggrp, (size_t)ng); L.take(flag, N1); L.take(lidx, N1); L.take(cs, 2 * N1); L.take(sc, 2 * N1); L.take(cn, 1); HIPC_AS(c, who, L.commit(c->hl_tmp, 64)); }
    long long* r_moff; int* r_member;
    { Carve L; L.take(r_moff, N1); L.take(r_member, (size_t)n); HIPC_AS(c, who, L.commit(c->hl_res, 64)); }
    c->hl_n = -1;
    bool sources;
    ORIP_TRY(gc_cut_intake(c, who, c->hl, up_off, up_pts, n, total, sources));
    HIPC_AS(c, who, hipMemcpyAsync(d_cls, cls, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemcpyAsync(d_roff, roff.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemcpyAsync(d_gspt, gspt.data(), ((size_t)ng + 1) * 8, hipMemcpyHostToDevice, s));
    if (ng) HIPC_AS(c, who, hipMemcpyAsync(d_ggrp, ggrp.data(), (size_t)ng * 4, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemsetAsync(cn, 0, sizeof(HlCounters), s));
    const dim3 b(256), gn1(cdiv((int64_t)N1, 256));
    if (R) {
        if (rg.sub) {
            HIPC_AS(c, who, hipMemcpyAsync(rsub, rg.sub, (size_t)m * 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_hl_rings, dim3(cdiv(R, 256)), b, 0, s, d_roff, m, R, rsub, c->sv_off.as<long long>(), c->sv_pts.as<double2>(), *rg.map, rg.clamp, rpts, cn);
        } else HIPC_AS(c, who, hipMemcpyAsync(rpts, rg.pts, (size_t)R * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_hl_edges, dim3(cdiv(R, 256)), b, 0, s, d_roff, m, R, rpts, edges);
    }
    const long long* d_off = c->gc_off.as<long long>(); const int2* d_pts = c->gc_pts.as<int2>();
    hipLaunchKernelGGL(k_hl_flag, gn1, b, 0, s, d_off, n, d_cls, flag);
    HIPC_AS(c, who, gc_scan_u64(c, flag, lidx, N1));
    HIPC_AS(c, who, hipGetLastError());
    struct { u64 nl; HlCounters cn; } h1;                                     // first read-back: the lines, and what the conversion of the rings found
    HIPC_AS(c, who, hipMemcpyAsync(&h1.nl, lidx + n, 8, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipMemcpyAsync(&h1.cn, cn, sizeof(HlCounters), hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    if (h1.cn.bad & HL_BAD_NOT_FINITE) { gc_drop(c); ORIP_FAIL_AS(c, who, "a ring holds a coordinate that is not finite after the conversion to steps"); }
    if (h1.cn.bad & HL_BAD_RANGE) { gc_drop(c); ORIP_FAIL_AS(c, who, "a ring holds a point more than 2^30 steps off the sheet after the conversion to steps"); }
    if (h1.nl > (u64)n) { gc_drop(c); ORIP_FAIL_AS(c, who, "the lines do not add up (internal error)"); }
    const int nl = (int)h1.nl;
    const size_t Z = (size_t)nl;
    int4 *lp, *J; int *lc, *ls, *link; u64 *keys, *cnts, *bestd; unsigned *vals, *besti; int2* tot;
    { Carve L; L.take(lp, Z); L.take(lc, Z); L.take(ls, Z); L.take(keys, 2 * Z); L.take(vals, 2 * Z); L.take(cnts, 2 * (Z + 1)); L.take(bestd, 2 * Z); L.take(besti, 2 * Z);
      L.take(link, 2 * Z); L.take(J, 2 * Z); L.take(tot, Z); HIPC_AS(c, who, L.commit(c->hl_ln, 64)); }
    u64 P = 0;
    const int4* Jfin = J;
    if (nl) {
        const dim3 gl(cdiv(nl, 256)), gl1(cdiv((int64_t)nl + 1, 256));
        HIPC_AS(c, who, hipMemsetAsync(bestd, 0xFF, 2 * Z * 8, s));
        HIPC_AS(c, who, hipMemsetAsync(besti, 0xFF, 2 * Z * 4, s));
        HIPC_AS(c, who, hipMemsetAsync(link, 0xFF, 2 * Z * 4, s));
        hipLaunchKernelGGL(k_hl_lines, dim3(cdiv(n, 256)), b, 0, s, d_off, d_pts, n, d_cls, flag, lidx, nl, (int)reach, lp, lc, ls, keys, vals, cn);
        { ProfScope ps(c, "hl_sort");
          HIPC_AS(c, who, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, keys, keys + Z, vals, vals + Z, Z, 0, 64, s); })); }
        const HlLines L = {lp, lc, keys + Z, vals + Z, nl, (int)reach};
        { ProfScope ps(c, "hl_count");
          hipLaunchKernelGGL(k_hl_count, gl1, b, 0, s, L, cnts);
          HIPC_AS(c, who, gc_scan_u64(c, cnts, cnts + Z + 1, Z + 1)); }
        HIPC_AS(c, who, hipGetLastError());
        HIPC_AS(c, who, hipMemcpyAsync(&P, cnts + Z + 1 + Z, 8, hipMemcpyDeviceToHost, s));       // second read-back: the pairs in reach
        HIPC_AS(c, who, hipStreamSynchronize(s));
        if (P >= (1ull << 30)) { gc_drop(c); ORIP_FAIL_AS(c, who, "%llu pairs in reach: fewer than 2^30", P); }
        uint2* pairs; uint8_t* elig;
        { Carve Lp; Lp.take(pairs, (size_t)P); Lp.take(elig, (size_t)P); HIPC_AS(c, who, Lp.commit(c->hl_pair, 64)); }
        if (P) {
            const HlShapes sh = {d_gspt, d_ggrp, edges, ng};
            hipLaunchKernelGGL(k_hl_fill, gl, b, 0, s, L, cnts, cnts + Z + 1, P, pairs, cn);
            { ProfScope ps(c, "hl_elig");
              hipLaunchKernelGGL(k_hl_elig, dim3((unsigned)std::min<u64>(P, HL_BLOCKS)), dim3(64), 0, s, P, pairs, nl, lp, lc, sh, elig, bestd, cn); }
            hipLaunchKernelGGL(k_hl_best, dim3(cdiv((int64_t)P, 256)), b, 0, s, P, pairs, elig, nl, lp, bestd, besti);
            hipLaunchKernelGGL(k_hl_mutual, gl, b, 0, s, nl, lp, besti, link, cn);
        }
        int rounds = 0; while (((int64_t)1 << rounds) < nl) rounds++;
        int4 *src = J, *dst = J + Z;
        hipLaunchKernelGGL(k_hl_chain0, gl, b, 0, s, nl, lp, link, src, cn);
        { ProfScope ps(c, "hl_jump");
          for (int r = 0; r < rounds; r++) { hipLaunchKernelGGL(k_hl_jump, gl, b, 0, s, src, dst, nl); std::swap(src, dst); } }
        Jfin = src;
        hipLaunchKernelGGL(k_hl_tails, gl, b, 0, s, nl, link, Jfin, tot, cn);
    }
    hipLaunchKernelGGL(k_hl_heads, gn1, b, 0, s, d_off, n, flag, lidx, nl, link, tot, cs, cn);
    HIPC_AS(c, who, gc_scan_u64(c, cs, sc, N1));
    HIPC_AS(c, who, gc_scan_u64(c, cs + N1, sc + N1, N1));
    ORIP_TRY(gc_cut_ensure(c, who, c->hl, n, total));                         // the output is never larger than the input
    const GcCutOut o = gc_cut_out(c, c->hl, sources, total, n);
    { ProfScope ps(c, "hl_emit");
      hipLaunchKernelGGL(k_hl_emit, dim3(cdiv(std::max<int64_t>(total, n + 1), 256)), b, 0, s, d_off, d_pts, n, total, flag, lidx, nl, lp, ls, link, Jfin, sc, o, r_moff, r_member, cn); }
    HIPC_AS(c, who, hipGetLastError());
    struct { u64 tot, members; HlCounters cn; } h;                            // third read-back: the totals and the counters
    HIPC_AS(c, who, hipMemcpyAsync(&h.tot, sc + n, 8, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipMemcpyAsync(&h.members, sc + N1 + n, 8, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipMemcpyAsync(&h.cn, cn, sizeof(HlCounters), hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    int64_t paths, points;
    gc_cut_totals(h.tot, paths, points);
    if (h.cn.bad || h.members != (u64)n || paths != n - (int64_t)h.cn.links || points != total - (int64_t)h.cn.coincident || h.cn.eligible > P || h.cn.links > h.cn.eligible) {
        gc_drop(c); ORIP_FAIL_AS(c, who, "the chains do not add up (internal error %u)", h.cn.bad);
    }
    gc_cut_publish(c, c->hl, sources, paths, points);
    c->hl_n = n; c->hl_paths = paths;
    stats[0] = nl; stats[1] = (int64_t)P; stats[2] = (int64_t)h.cn.eligible; stats[3] = (int64_t)h.cn.links; stats[4] = (int64_t)h.cn.coincident;
    stats[5] = paths; stats[6] = points; stats[7] = (int64_t)h.cn.link_steps;
    return 0;
}
}  // namespace

// include/orip.h states the rule; the zigzags become the resident step polylines
extern "C" int orip_gcode_hatch_link(orip_ctx* c, const int64_t* off, const int32_t* pts, const int32_t* cls, int64_t n, const int64_t* ring_off, const int32_t* ring_pts,
                                     const int32_t* ring_group, int64_t m, int32_t reach, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats) ORIP_FAIL(c, "bad arguments");
    int64_t total;
    ORIP_TRY(gc_steps_check(c, __func__, off, pts, n, true, total, 28));
    const HlRings rg = {ring_off, ring_pts, nullptr, ring_group, m, nullptr, 0};
    return hl_core(c, __func__, off, pts, cls, n, total, rg, reach, stats);
}

extern "C" int orip_svg_hatch_link(orip_ctx* c, const int32_t* cls, int64_t n, const int32_t* ring_sub, const int32_t* ring_group, int64_t m, const orip_gcode_map* map,
                                   int32_t flags, int32_t reach, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats || !map || (m > 0 && !ring_sub)) ORIP_FAIL(c, "bad arguments");
    if (flags & ~ORIP_HATCH_LINK_CLAMP) ORIP_FAIL(c, "unknown flags %d", flags);
    if (map->W < 1 || map->H < 1 || map->W > GC_COORD_MAX || map->H > GC_COORD_MAX) ORIP_FAIL(c, "target size %d x %d steps: each side must be in 1..2^30", map->W, map->H);
    int64_t total;
    ORIP_TRY(gc_steps_check(c, __func__, nullptr, nullptr, n, false, total, 28));
    static const int32_t none = 0;
    const HlRings rg = {nullptr, nullptr, ring_sub ? ring_sub : &none, ring_group, m, map, (flags & ORIP_HATCH_LINK_CLAMP) ? 1 : 0};
    return hl_core(c, __func__, nullptr, nullptr, cls, n, total, rg, reach, stats);
}

extern "C" int orip_gcode_hatch_link_fetch(orip_ctx* c, int64_t* member_off, int32_t* member) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (c->hl_n < 0) ORIP_FAIL(c, "no result: the hatch link has not succeeded since the last failure");
    if (!member_off || (c->hl_n > 0 && !member)) ORIP_FAIL(c, "bad arguments");
    if (c->hl_n == 0) { member_off[0] = 0; return 0; }
    hipStream_t s = LN(c).stream;
    const size_t n = (size_t)c->hl_n;
    long long* r_moff; int* r_member;                                         // the layout hl_core carved; the buffer already holds it, so nothing grows
    { Carve L; L.take(r_moff, n + 1); L.take(r_member, n); HIPC(c, L.commit(c->hl_res, 64)); }
    HIPC(c, hipMemcpyAsync(member_off, r_moff, (size_t)(c->hl_paths + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(member, r_member, n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
