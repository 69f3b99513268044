// csrc/hatch_angle.hip -- --hatch-angle-deg of svg2stream.py / svg2gcode.py: hatch lines along any integer direction u (orip_svg_hatch_angle; the rule is
// stated in include/orip.h, is exact in integers and rationals on the step grid and has one answer for every input).  Ours: the reference's hatch_fill
// knows X and Y only, and its float-and-truncate arithmetic is not rotation-covariant.  The scaffolding is that of hatch.hip (hatch_common.h); what differs
// is the coordinate pair (s, w) = (n . p, u . p) in the place of (y, x), the crossing record and every piece of arithmetic on it.
//
// 0. Quantise.  One thread per resident point: q = rint(v * steps_per_mm) as hatch.hip does it, |q| >= 2^24 raises a flag; its group and its successor;
//    64-bit atomicMin / atomicMax give each group its range of s for BOTH families (the family along n' = (-uy, ux) has s' = -ux x - uy y).
// Then per family, with (ux, uy) its own direction:
// 1. Lines.  One thread per group: k0 = floor(min s / D) + 1 and the number of lines up to floor(max s / D); an exclusive scan gives the first global row.
// 2. Chunks.  One thread per edge: its lines floor(s_a / D) + 1 .. floor(s_b / D) in chunks of at most 64; a scan places the chunks.
// 3. Count, scan, fill.  One thread per chunk; the second run writes the crossing w = num / den, num = w_a (s_b - s_a) + (k D - s_a)(w_b - w_a) < 2^77 in
//    magnitude as two 64-bit words, den = s_b - s_a in (0, 2^38), and the row, through a cursor per row.
// 4. Sort inside each row by the exact order of w (ha_less: one 128-bit cross product per side, below 2^115): up to 64 crossings one wave in registers
//    (bitonic over __shfl_xor), up to 2048 one block in LDS (bitonic on three word arrays, 48 KB).  If any row is longer, rocPRIM's merge sort orders the
//    whole record array by (row, w) in the place of both: the rows are contiguous already, so it sorts inside them.  Equal w are interchangeable: every
//    later step reads the value, never the representation.  The padding of a bitonic network is den = 0, which compares above everything.
// 5. Pair.  One thread per crossing: an even place with a successor in its row; kept iff w_1 - w_0 > 2 I, one comparison of 128-bit products (below 2^122).
//    Both end points are rounded (ha_point: the exact rational, nearest step, halves toward +infinity; the quotient is estimated in double and corrected
//    against the exact 128-bit remainder, so no result of floating point is trusted); coinciding ends are counted in `collapsed` and dropped.
// 6. Emit.  One thread per kept pair: the same two points again, reversed when k & 1 under serpentine, as mm rounded to four decimals.
// Nothing is committed (sv_n, sv_total, ht_nseg) before the last kernel of the last family has run.  Every index is bounded by a count computed on the
// device and checked on the host before the buffers are sized, as in hatch.hip.
//
// Magnitudes: |q| < 2^24, |u| <= 2^12 per component, so |s|, |w| < 2^37, U2 <= 2^25; spacing, inset < 2^31, so D, I < 2^44 (the host computes both, exactly).
// A point's numerator: (num + I den) u < 2^83 2^12, doubled for the rounding 2^96; its denominator 2 den U2 <= 2^64, kept in 128 bits.
#include "hatch_common.h"
#include "sv_round.h"
#include <rocprim/rocprim.hpp>
#include <climits>
#include <cmath>

namespace {
typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;
constexpr double HA_QLIM = 16777216.0;
constexpr int HA_UMAX = 4096;

struct HaX { u64 lo, hi, den; unsigned row, pad; };                          // w = (hi:lo as signed 128 bits) / den; den == 0: the padding of a sort
__host__ __device__ __forceinline__ i128 ha_num(const HaX& a) { return (i128)(((u128)a.hi << 64) | a.lo); }
__host__ __device__ __forceinline__ bool ha_less3(u64 alo, u64 ahi, u64 aden, u64 blo, u64 bhi, u64 bden) {
    if (aden == 0) return false;
    if (bden == 0) return true;
    return (i128)(((u128)ahi << 64) | alo) * (i128)bden < (i128)(((u128)bhi << 64) | blo) * (i128)aden;
}
struct HaLess {                                                              // the merge sort's order: rows ascending, w ascending inside a row
    __host__ __device__ bool operator()(const HaX& a, const HaX& b) const { return a.row != b.row ? a.row < b.row : ha_less3(a.lo, a.hi, a.den, b.lo, b.hi, b.den); }
};
struct HaDir { long long ux, uy, U2, D, I; };                                // one family: its direction, u . u, the lines' distance and the inset in units of s and w

__device__ __forceinline__ double ha_double(i128 v) {
    const bool neg = v < 0;
    const u128 a = neg ? (u128)0 - (u128)v : (u128)v;
    const double d = (double)(u64)(a >> 64) * 18446744073709551616.0 + (double)(u64)a;
    return neg ? -d : d;
}
// floor((2 num + den) / (2 den)), den > 0: the nearest integer to num / den, halves toward +infinity.  |result| < 2^27 for every point asked for
__device__ __forceinline__ long long ha_round_div(i128 num, i128 den) {
    const i128 n2 = 2 * num + den, d2 = 2 * den;
    long long q = (long long)floor(ha_double(num) / ha_double(den) + 0.5);
    i128 rem = n2 - (i128)q * d2;
    for (int i = 0; i < 4 && rem < 0; i++) { q--; rem += d2; }
    for (int i = 0; i < 4 && rem >= d2; i++) { q++; rem -= d2; }
    return q;
}
// the point at w = N / d on line s = kD of the family: ((w ux - kD uy) / U2, (w uy + kD ux) / U2), each coordinate rounded
__device__ __forceinline__ int2 ha_point(const HaDir& F, i128 N, long long d, long long kD) {
    const i128 den = (i128)d * F.U2, sd = (i128)kD * d;
    return make_int2((int)ha_round_div(N * F.ux - sd * F.uy, den), (int)ha_round_div(N * F.uy + sd * F.ux, den));
}

__global__ __launch_bounds__(256) void k_ha_box_init(long long* __restrict__ box, int64_t G) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < G) { box[4 * g] = LLONG_MAX; box[4 * g + 1] = LLONG_MIN; box[4 * g + 2] = LLONG_MAX; box[4 * g + 3] = LLONG_MIN; }
}

// box[4 g ..]: min s, max s of the family along u, then of the family along (-uy, ux)
__global__ __launch_bounds__(256) void k_ha_quant(const long long* __restrict__ off, const double2* __restrict__ pts, const int* __restrict__ gid, int64_t P, int64_t total, double spm,
                                                  long long ux, long long uy, int2* __restrict__ q, int* __restrict__ pgrp, int* __restrict__ nxt, long long* __restrict__ box,
                                                  HtCounters* __restrict__ cn) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    int64_t lo = 0, hi = P;                                                  // last p with off[p] <= j
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= j) lo = mid; else hi = mid; }
    const double2 v = pts[j];
    const double fx = rint(sv_mul(v.x, spm)), fy = rint(sv_mul(v.y, spm));
    int2 r = make_int2(0, 0);
    if (fabs(fx) < HA_QLIM && fabs(fy) < HA_QLIM) r = make_int2((int)fx, (int)fy);      // not so for a NaN either
    else atomicOr(&cn->err, 1);
    const int g = gid[lo];
    q[j] = r; pgrp[j] = g;
    nxt[j] = (int)(j + 1 == off[lo + 1] ? off[lo] : j + 1);
    if (g >= 0) {
        const long long s0 = -uy * r.x + ux * r.y, s1 = -ux * r.x - uy * r.y;
        atomicMin(&box[4 * g], s0); atomicMax(&box[4 * g + 1], s0); atomicMin(&box[4 * g + 2], s1); atomicMax(&box[4 * g + 3], s1);
    }
}

// the first line and the number of lines of every group; nl[G] = 0 closes the scan
__global__ __launch_bounds__(256) void k_ha_lines(const long long* __restrict__ box, int64_t G, int fam, long long D, long long* __restrict__ k0, long long* __restrict__ nl) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > G) return;
    if (g == G) { nl[g] = 0; return; }
    const long long lo = box[4 * g + 2 * fam], hi = box[4 * g + 2 * fam + 1];
    if (lo > hi) { k0[g] = 0; nl[g] = 0; return; }                           // a group without points
    const long long a = ht_floordiv(lo, D) + 1, b = ht_floordiv(hi, D);
    k0[g] = a;
    nl[g] = b >= a ? b - a + 1 : 0;
}

struct HaEdge { long long sa, wa, sb, wb, klo, khi; int g; };
// the edge from point j to its successor, ordered to s_a < s_b, and the lines klo .. khi that it crosses (s_a < k D <= s_b); false: none
__device__ __forceinline__ bool ha_edge(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t j, const HaDir& F,
                                        const long long* __restrict__ k0, const long long* __restrict__ nl, HaEdge& e) {
    e.g = pgrp[j];
    if (e.g < 0) return false;
    const int2 a = q[j], b = q[nxt[j]];
    long long sa = -F.uy * a.x + F.ux * a.y, sb = -F.uy * b.x + F.ux * b.y, wa = F.ux * a.x + F.uy * a.y, wb = F.ux * b.x + F.uy * b.y;
    if (sa == sb) return false;
    if (sa > sb) { long long t = sa; sa = sb; sb = t; t = wa; wa = wb; wb = t; }
    e.sa = sa; e.sb = sb; e.wa = wa; e.wb = wb;
    const long long first = k0[e.g];
    e.klo = max(first, ht_floordiv(sa, F.D) + 1);                            // the group's range says so already; the clamps keep every row inside it
    e.khi = min(ht_floordiv(sb, F.D), first + nl[e.g] - 1);
    return e.khi >= e.klo;
}

__global__ __launch_bounds__(256) void k_ha_chunks(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t total, HaDir F,
                                                   const long long* __restrict__ k0, const long long* __restrict__ nl, long long* __restrict__ chunkn, HtCounters* __restrict__ cn) {
    __shared__ unsigned long long sum;
    if (threadIdx.x == 0) sum = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j <= total) {
        HaEdge e;
        long long n = 0;
        if (j < total && ha_edge(q, pgrp, nxt, j, F, k0, nl, e)) n = e.khi - e.klo + 1;
        chunkn[j] = (n + HT_CHUNK - 1) / HT_CHUNK;
        if (n) atomicAdd(&sum, (unsigned long long)n);
    }
    __syncthreads();
    if (threadIdx.x == 0 && sum) atomicAdd(&cn->crossings, sum);
}

// one thread per chunk of at most HT_CHUNK lines of one edge.  FILL false: counts per row; true: the crossings through the rows' cursors
template <bool FILL>
__global__ __launch_bounds__(256) void k_ha_cross(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t total, HaDir F,
                                                  const long long* __restrict__ k0, const long long* __restrict__ nl, const long long* __restrict__ rowbase,
                                                  const long long* __restrict__ chunkoff, int64_t C, int64_t R, int64_t X, unsigned* __restrict__ rowcnt,
                                                  const unsigned* __restrict__ rowoff, HaX* __restrict__ xs) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int64_t lo = 0, hi = total;                                              // last edge with chunkoff[edge] <= c: the one that owns chunk c
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (chunkoff[mid] <= c) lo = mid; else hi = mid; }
    HaEdge e;
    if (!ha_edge(q, pgrp, nxt, lo, F, k0, nl, e)) return;
    const long long ka = e.klo + (long long)HT_CHUNK * (c - chunkoff[lo]), kb = min(e.khi, ka + HT_CHUNK - 1);
    const long long rb = rowbase[e.g] - k0[e.g], den = e.sb - e.sa, dw = e.wb - e.wa;
    const i128 base = (i128)e.wa * den;
    for (long long k = ka; k <= kb; k++) {
        const long long row = rb + k;
        if (row < 0 || row >= R) continue;
        if (!FILL) { atomicAdd(&rowcnt[row], 1u); continue; }
        const long long p = (long long)rowoff[row] + atomicAdd(&rowcnt[row], 1u);
        if (p >= X) continue;
        const u128 num = (u128)(base + (i128)(k * F.D - e.sa) * dw);
        xs[p] = HaX{(u64)num, (u64)(num >> 64), (u64)den, (unsigned)row, 0u};
    }
}

__global__ __launch_bounds__(256) void k_ha_sort_wave(const HaX* __restrict__ xs, HaX* __restrict__ out, const unsigned* __restrict__ rowoff, const unsigned* __restrict__ rowcnt, int64_t R) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const unsigned lane = threadIdx.x & 63;
    if (r >= R) return;
    const unsigned n = rowcnt[r];
    if (n == 0 || n > HT_WAVE_MAX) return;                                   // the whole wave leaves together
    const unsigned o = rowoff[r];
    u64 lo = 0, hi = 0, den = 0;
    if (lane < n) { const HaX v = xs[o + lane]; lo = v.lo; hi = v.hi; den = v.den; }
    for (unsigned k = 2; k <= 64; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            const u64 plo = __shfl_xor(lo, (int)j, 64), phi = __shfl_xor(hi, (int)j, 64), pden = __shfl_xor(den, (int)j, 64);
            const bool up = (lane & k) == 0, low = (lane & j) == 0;
            // the lower place of an ascending pair keeps the smaller; on a tie both sides keep their own, so nothing is lost or doubled
            const bool take = up == low ? ha_less3(plo, phi, pden, lo, hi, den) : ha_less3(lo, hi, den, plo, phi, pden);
            if (take) { lo = plo; hi = phi; den = pden; }
        }
    if (lane < n) out[o + lane] = HaX{lo, hi, den, (unsigned)r, 0u};
}

__global__ __launch_bounds__(256) void k_ha_sort_block(const HaX* __restrict__ xs, HaX* __restrict__ out, const unsigned* __restrict__ rowoff, const unsigned* __restrict__ rowcnt,
                                                       const unsigned* __restrict__ medlist, unsigned n_med) {
    __shared__ u64 slo[HT_BLOCK_MAX], shi[HT_BLOCK_MAX], sden[HT_BLOCK_MAX];             // 48 KB
    if (blockIdx.x >= n_med) return;
    const unsigned r = medlist[blockIdx.x], n = rowcnt[r], o = rowoff[r];
    if (n > HT_BLOCK_MAX) return;
    unsigned m = 128;
    while (m < n) m <<= 1;
    for (unsigned i = threadIdx.x; i < m; i += 256) {
        HaX v{0, 0, 0, 0, 0};
        if (i < n) v = xs[o + i];
        slo[i] = v.lo; shi[i] = v.hi; sden[i] = v.den;
    }
    __syncthreads();
    for (unsigned k = 2; k <= m; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = threadIdx.x; i < m; i += 256) {
                const unsigned p = i ^ j;
                if (p > i) {
                    const u64 alo = slo[i], ahi = shi[i], aden = sden[i], blo = slo[p], bhi = shi[p], bden = sden[p];
                    const bool asc = (i & k) == 0;
                    if (asc ? ha_less3(blo, bhi, bden, alo, ahi, aden) : ha_less3(alo, ahi, aden, blo, bhi, bden)) {
                        slo[i] = blo; shi[i] = bhi; sden[i] = bden; slo[p] = alo; shi[p] = ahi; sden[p] = aden;
                    }
                }
            }
            __syncthreads();
        }
    for (unsigned i = threadIdx.x; i < n; i += 256) out[o + i] = HaX{slo[i], shi[i], sden[i], r, 0u};
}

// the pair of crossings i, i + 1 of one row: 0 dropped (we <= ws), 1 kept, 2 collapsed; a, b: the rounded ends in ascending w
__device__ __forceinline__ int ha_pair(const HaX* __restrict__ xs, int64_t i, const HaDir& F, long long kD, int2& a, int2& b) {
    const HaX x0 = xs[i], x1 = xs[i + 1];
    const i128 n0 = ha_num(x0), n1 = ha_num(x1);
    const long long d0 = (long long)x0.den, d1 = (long long)x1.den;
    if (d0 <= 0 || d1 <= 0) return 0;
    if (!(n1 * d0 - n0 * d1 > (i128)(2 * F.I) * d0 * d1)) return 0;          // we > ws
    a = ha_point(F, n0 + (i128)F.I * d0, d0, kD);
    b = ha_point(F, n1 - (i128)F.I * d1, d1, kD);
    return (a.x == b.x && a.y == b.y) ? 2 : 1;
}
// the group that owns a row and the row's line number
__device__ __forceinline__ long long ha_row_line(const long long* __restrict__ rowbase, const long long* __restrict__ k0, int64_t G, long long row, int64_t& g) {
    int64_t lo = 0, hi = G;                                                  // last group with rowbase[group] <= row
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (rowbase[mid] <= row) lo = mid; else hi = mid; }
    g = lo;
    return k0[lo] + (row - rowbase[lo]);
}

__global__ __launch_bounds__(256) void k_ha_pairs(const HaX* __restrict__ xs, const unsigned* __restrict__ rowoff, const unsigned* __restrict__ rowcnt, int64_t X, int64_t R, HaDir F,
                                                  const long long* __restrict__ rowbase, const long long* __restrict__ k0, int64_t G, unsigned* __restrict__ keep,
                                                  unsigned long long* __restrict__ collapsed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > X) return;
    unsigned kp = 0;
    if (i < X) {
        const unsigned row = xs[i].row;
        if (row < R) {
            const unsigned li = (unsigned)(i - rowoff[row]);
            if ((li & 1) == 0 && li + 1 < rowcnt[row] && i + 1 < X) {
                int64_t g; int2 a, b;
                const long long k = ha_row_line(rowbase, k0, G, row, g);
                const int r = ha_pair(xs, i, F, k * F.D, a, b);
                kp = r == 1;
                if (r == 2) atomicAdd(collapsed, 1ull);
            }
        }
    }
    keep[i] = kp;
}

__global__ __launch_bounds__(256) void k_ha_emit(const HaX* __restrict__ xs, const unsigned* __restrict__ keep, const unsigned* __restrict__ kpos, int64_t X, int64_t R,
                                                 const long long* __restrict__ rowbase, const long long* __restrict__ k0, int64_t G, HaDir F, int serpentine,
                                                 double spm, int64_t n0, int64_t t0, int64_t S, long long* __restrict__ off_out, double2* __restrict__ pts_out, const int* __restrict__ gnum,
                                                 int* __restrict__ grp_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= X || i + 1 >= X || !keep[i]) return;
    const int64_t s = kpos[i];
    if (s >= S) return;
    const long long row = xs[i].row;
    if (row >= R) return;
    int64_t g; int2 a, b;
    const long long k = ha_row_line(rowbase, k0, G, row, g);
    if (ha_pair(xs, i, F, k * F.D, a, b) != 1) return;
    if (serpentine && (k & 1)) { const int2 t = a; a = b; b = t; }
    pts_out[t0 + 2 * s] = make_double2(sv_round4(__ddiv_rn((double)a.x, spm)), sv_round4(__ddiv_rn((double)a.y, spm)));
    pts_out[t0 + 2 * s + 1] = make_double2(sv_round4(__ddiv_rn((double)b.x, spm)), sv_round4(__ddiv_rn((double)b.y, spm)));
    off_out[n0 + s + 1] = t0 + 2 * (s + 1);
    grp_out[s] = gnum[g];                                                    // the caller's number of the owning group
}

struct HaPlan {                       // what the families share: the quantised points (ht_pts) and where the next segments go
    int2* q; int *pgrp, *nxt, *gnum; long long* box; HtCounters* cn; unsigned long long* collapsed; long long *k0, *nl, *rowbase, *chunkn, *chunkoff;
    int64_t G, total, n, tot, n_sub; int serpentine; double spm;
};

// the nearest integer to sqrt(v), v < 2^88: (isqrt(4 v) + 1) >> 1
long long ha_rs(u128 v) {
    const u128 t = 4 * v;
    u64 lo = 0, hi = 1ull << 46;                                             // lo^2 <= t < hi^2
    while (hi - lo > 1) { const u64 mid = lo + (hi - lo) / 2; if ((u128)mid * mid <= t) lo = mid; else hi = mid; }
    return (long long)((lo + 1) >> 1);
}

// one family: appends its segments behind path P.n / point P.tot (not committed) and moves both on
int ha_family(orip_ctx* c, HaPlan& P, int fam, const HaDir& F, int64_t* stats) {
    hipStream_t s = LN(c).stream;
    const int64_t G = P.G, total = P.total;
    HIPC(c, hipMemsetAsync(P.cn, 0, sizeof(HtCounters), s));
    hipLaunchKernelGGL(k_ha_lines, dim3(cdiv(G + 1, 256)), dim3(256), 0, s, P.box, G, fam, F.D, P.k0, P.nl);
    ORIP_TRY(vscan_excl<int64_t>(c, (const int64_t*)P.nl, (int64_t*)P.rowbase, (size_t)G + 1));
    hipLaunchKernelGGL(k_ha_chunks, dim3(cdiv(total + 1, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, F, P.k0, P.nl, P.chunkn, P.cn);
    ORIP_TRY(vscan_excl<int64_t>(c, (const int64_t*)P.chunkn, (int64_t*)P.chunkoff, (size_t)total + 1));
    HIPC(c, hipGetLastError());
    long long R = 0, C = 0; HtCounters h;
    HIPC(c, hipMemcpyAsync(&R, P.rowbase + G, 8, hipMemcpyDeviceToHost, s)); HIPC(c, hipMemcpyAsync(&C, P.chunkoff + total, 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h, P.cn, sizeof h, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    const long long X = (long long)h.crossings;
    if (R < 0 || R > HT_MAX_ROWS) ORIP_FAIL(c, "%lld hatch lines: at most 2^26", R);
    if (X < 0 || X > HT_MAX_CROSSINGS) ORIP_FAIL(c, "%lld crossings: at most 2^30", X);
    if (C < 0 || C > X + total) ORIP_FAIL(c, "%lld chunks for %lld crossings of %lld edges", C, X, (long long)total);
    stats[1] += R; stats[2] += X;
    if (X == 0) return 0;
    unsigned *rowcnt, *rowoff, *medlist, *keep, *kpos; HaX *xs, *xs2;
    { Carve L; L.take(rowcnt, (size_t)R + 1); L.take(rowoff, (size_t)R + 1); L.take(medlist, (size_t)R); HIPC(c, L.commit(c->ht_rows, 64)); }
    { Carve L; L.take(xs, (size_t)X); L.take(xs2, (size_t)X); L.take(keep, (size_t)X + 1); L.take(kpos, (size_t)X + 1); HIPC(c, L.commit(c->ht_x, 64)); }
    HIPC(c, hipMemsetAsync(rowcnt, 0, (size_t)(R + 1) * 4, s));
    { ProfScope ps(c, "k_ha_cross_count");
      hipLaunchKernelGGL(k_ha_cross<false>, dim3(cdiv(C, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, F, P.k0, P.nl, P.rowbase, P.chunkoff, (int64_t)C, (int64_t)R, (int64_t)X,
                         rowcnt, (const unsigned*)rowoff, xs); }
    hipLaunchKernelGGL(k_ht_classify, dim3(cdiv(R + 1, 256)), dim3(256), 0, s, rowcnt, (int64_t)R, medlist, P.cn);
    ORIP_TRY(vscan_excl<unsigned>(c, rowcnt, rowoff, (size_t)R + 1));
    HIPC(c, hipMemsetAsync(rowcnt, 0, (size_t)(R + 1) * 4, s));
    { ProfScope ps(c, "k_ha_cross_fill");
      hipLaunchKernelGGL(k_ha_cross<true>, dim3(cdiv(C, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, F, P.k0, P.nl, P.rowbase, P.chunkoff, (int64_t)C, (int64_t)R, (int64_t)X,
                         rowcnt, (const unsigned*)rowoff, xs); }
    HIPC(c, hipGetLastError());
    unsigned xtot = 0;
    HIPC(c, hipMemcpyAsync(&xtot, rowoff + R, 4, hipMemcpyDeviceToHost, s)); HIPC(c, hipMemcpyAsync(&h, P.cn, sizeof h, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if ((long long)xtot != X) ORIP_FAIL(c, "the rows hold %u crossings, the edges %lld", xtot, X);
    if (h.n_big) {
        ProfScope ps(c, "ha_sort_merge");
        HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::merge_sort(tmp, bytes, xs, xs2, (size_t)X, HaLess(), s); }));
    } else {
        { ProfScope ps(c, "k_ha_sort_wave");
          hipLaunchKernelGGL(k_ha_sort_wave, dim3(cdiv(R, 4)), dim3(256), 0, s, xs, xs2, rowoff, rowcnt, (int64_t)R); }
        if (h.n_med) { ProfScope ps(c, "k_ha_sort_block");
          hipLaunchKernelGGL(k_ha_sort_block, dim3(h.n_med), dim3(256), 0, s, xs, xs2, rowoff, rowcnt, medlist, h.n_med); }
    }
    { ProfScope ps(c, "k_ha_pairs");
      hipLaunchKernelGGL(k_ha_pairs, dim3(cdiv(X + 1, 256)), dim3(256), 0, s, xs2, rowoff, rowcnt, (int64_t)X, (int64_t)R, F, P.rowbase, P.k0, G, keep, P.collapsed); }
    ORIP_TRY(vscan_excl<unsigned>(c, keep, kpos, (size_t)X + 1));
    unsigned S = 0;
    ORIP_TRY(vread(c, &S, (const unsigned*)kpos + X));
    stats[3] += S;
    if (S == 0) return 0;
    const int64_t n1 = P.n + S, t1 = P.tot + 2 * (int64_t)S;
    if (n1 >= HT_MAX_POINTS || t1 > HT_MAX_POINTS) ORIP_FAIL(c, "%lld paths with %lld points after hatching: at most 2^30 - 2 paths and 2^30 - 1 points", (long long)n1, (long long)t1);
    HIPC(c, c->sv_off.ensure((size_t)(n1 + 1) * 8 + 64, s, true)); HIPC(c, c->sv_pts.ensure((size_t)t1 * 16 + 64, s, true));
    HIPC(c, c->ht_grp.ensure((size_t)(n1 - P.n_sub) * 4 + 64, s, true));
    { ProfScope ps(c, "k_ha_emit");
      hipLaunchKernelGGL(k_ha_emit, dim3(cdiv(X, 256)), dim3(256), 0, s, xs2, keep, kpos, (int64_t)X, (int64_t)R, P.rowbase, P.k0, G, F, P.serpentine, P.spm, P.n, P.tot, (int64_t)S,
                         c->sv_off.as<long long>(), c->sv_pts.as<double2>(), P.gnum, c->ht_grp.as<int>() + (P.n - P.n_sub)); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    P.n = n1; P.tot = t1;
    return 0;
}
}  // namespace

extern "C" int orip_svg_hatch_angle(orip_ctx* c, const int32_t* fill_group, int64_t n_sub, double steps_per_mm, int32_t spacing, int32_t inset, int32_t ux, int32_t uy, int32_t flags,
                                    int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats || n_sub < 0 || (n_sub > 0 && !fill_group)) ORIP_FAIL(c, "bad arguments");
    for (int k = 0; k < 5; k++) stats[k] = 0;
    HtGroups grp;
    ORIP_TRY(ht_intake(c, __func__, fill_group, n_sub, steps_per_mm, spacing, inset, flags, grp));
    if ((ux == 0 && uy == 0) || ux < -HA_UMAX || ux > HA_UMAX || uy < -HA_UMAX || uy > HA_UMAX)
        ORIP_FAIL(c, "hatch direction (%d, %d): not zero, each component within +-4096", ux, uy);
    const int64_t G = grp.G, total = c->sv_total;
    stats[0] = G;
    if (G == 0 || total == 0) { c->ht_nseg = 0; c->sv_hatched = true; return 0; }
    const long long U2 = (long long)ux * ux + (long long)uy * uy;
    const long long D = ha_rs((u128)((u64)spacing * (u64)spacing) * (u64)U2), I = ha_rs((u128)((u64)inset * (u64)inset) * (u64)U2);
    const HaDir dir[2] = {HaDir{ux, uy, U2, D, I}, HaDir{-(long long)uy, ux, U2, D, I}};
    hipStream_t s = LN(c).stream;
    HaPlan P{};
    int* d_gid;
    { Carve L; L.take(d_gid, (size_t)n_sub); L.take(P.q, (size_t)total); L.take(P.pgrp, (size_t)total); L.take(P.nxt, (size_t)total); L.take(P.box, (size_t)4 * G); L.take(P.cn, 1);
      L.take(P.collapsed, 1); L.take(P.k0, (size_t)G); L.take(P.nl, (size_t)G + 1); L.take(P.rowbase, (size_t)G + 1); L.take(P.chunkn, (size_t)total + 1);
      L.take(P.chunkoff, (size_t)total + 1); L.take(P.gnum, (size_t)G); HIPC(c, L.commit(c->ht_pts, 64)); }
    P.G = G; P.total = total; P.n = c->sv_n; P.n_sub = c->sv_n; P.tot = total; P.serpentine = flags & ORIP_HATCH_SERPENTINE ? 1 : 0; P.spm = steps_per_mm;
    HIPC(c, hipMemcpyAsync(d_gid, grp.gid.data(), (size_t)n_sub * 4, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(P.gnum, grp.gnum.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(P.cn, 0, sizeof(HtCounters), s));
    HIPC(c, hipMemsetAsync(P.collapsed, 0, 8, s));
    hipLaunchKernelGGL(k_ha_box_init, dim3(cdiv(G, 256)), dim3(256), 0, s, P.box, G);
    { ProfScope ps(c, "k_ha_quant");
      hipLaunchKernelGGL(k_ha_quant, dim3(cdiv(total, 256)), dim3(256), 0, s, c->sv_off.as<long long>(), c->sv_pts.as<double2>(), d_gid, n_sub, total, steps_per_mm, (long long)ux, (long long)uy,
                         P.q, P.pgrp, P.nxt, P.box, P.cn); }
    HIPC(c, hipGetLastError());
    HtCounters h;
    ORIP_TRY(vread(c, &h, (const HtCounters*)P.cn));
    if (h.err) ORIP_FAIL(c, "a coordinate reaches 2^24 steps at %g steps per mm: the hatch at an angle keeps its products inside 128 bits", steps_per_mm);
    int64_t st[4] = {0, 0, 0, 0};
    if (flags & ORIP_HATCH_HORIZONTAL) ORIP_TRY(ha_family(c, P, 0, dir[0], st));
    if (flags & ORIP_HATCH_VERTICAL) ORIP_TRY(ha_family(c, P, 1, dir[1], st));
    unsigned long long coll = 0;
    ORIP_TRY(vread(c, &coll, (const unsigned long long*)P.collapsed));
    stats[1] = st[1]; stats[2] = st[2]; stats[3] = st[3]; stats[4] = (int64_t)coll;
    c->ht_nseg = P.n - c->sv_n;
    c->sv_n = P.n; c->sv_total = P.tot; c->sv_hatched = true; c->sv_box_ok = false;
    return 0;
}
