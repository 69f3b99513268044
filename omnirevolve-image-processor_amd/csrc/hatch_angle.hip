// csrc/hatch_angle.hip -- --hatch-angle-deg of svg2stream.py / svg2gcode.py: hatch lines along any integer direction u (orip_svg_hatch_angle; the rule is
// stated in include/orip.h, is exact in integers and rationals on the step grid and has one answer for every input).  Ours: the reference's hatch_fill
// knows X and Y only, and its float-and-truncate arithmetic is not rotation-covariant.  The frame is that of hatch.hip, stated once in hatch_common.h, which
// numbers the steps; HaRule below puts into it the coordinate pair (s, w) = (n . p, u . p) in the place of (y, x), the crossing record and every piece of
// arithmetic on it.
//
// 0. Quantise.  |q| >= 2^24 raises the flag; 64-bit atomicMin / atomicMax give each group its range of s for BOTH families (the family along
//    n' = (-uy, ux) has s' = -ux x - uy y): box = min s, max s, min s', max s'.
// Then per family, with (ux, uy) its own direction:
// 1. Lines.  k0 = floor(min s / D) + 1 and the number of lines up to floor(max s / D); line k is the global one, s = k D.
// 2. Chunks.  An edge, ordered to s_a < s_b, crosses the lines floor(s_a / D) + 1 .. floor(s_b / D).
// 3. Fill.  The crossing w = num / den, num = w_a (s_b - s_a) + (k D - s_a)(w_b - w_a) < 2^77 in magnitude as two 64-bit words, den = s_b - s_a in
//    (0, 2^38), and the row, in one record.
// 4. Sort inside each row by the exact order of w (ha_less3: one 128-bit cross product per side, below 2^115): up to 64 crossings one wave in registers
//    (bitonic over __shfl_xor), up to 2048 one block in LDS (bitonic on three word arrays, 48 KB).  If any row is longer, rocPRIM's merge sort orders the
//    whole record array by (row, w) in the place of both: the rows are contiguous already, so it sorts inside them.  Equal w are interchangeable: every
//    later step reads the value, never the representation.  The padding of a bitonic network is den = 0, which compares above everything.
// 5. Pair.  Kept iff w_1 - w_0 > 2 I, one comparison of 128-bit products (below 2^122).  Both end points are rounded (ha_point: the exact rational, nearest
//    step, halves toward +infinity; the quotient is estimated in double and corrected against the exact 128-bit remainder, so no result of floating point
//    is trusted); coinciding ends are counted in `collapsed` and dropped.
// 6. Emit.  The same two points again, reversed when k & 1 under serpentine.
//
// Magnitudes: |q| < 2^24, |u| <= 2^12 per component, so |s|, |w| < 2^37, U2 <= 2^25; spacing, inset < 2^31, so D, I < 2^44 (the host computes both, exactly).
// A point's numerator: (num + I den) u < 2^83 2^12, doubled for the rounding 2^96; its denominator 2 den U2 <= 2^64, kept in 128 bits.
#include "hatch_common.h"
#include <rocprim/rocprim.hpp>
#include <climits>
#include <cmath>

namespace {
typedef unsigned long long u64;
typedef __int128 i128;
typedef unsigned __int128 u128;
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

struct HaEdge { long long sa, wa, sb, wb, klo, khi; int g; };

struct HaRule {
    typedef HaDir Dir; typedef long long Box; typedef HaEdge Edge; typedef HaX X;
    static constexpr double QLIM = 16777216.0;
    static constexpr bool CROW = false, COLLAPSED = true;                    // the row travels in the record; coinciding ends are counted
    static constexpr const char *QLIM_MSG = "a coordinate reaches 2^24 steps at %g steps per mm: the hatch at an angle keeps its products inside 128 bits";
    static constexpr const char *S_QUANT = "k_ha_quant", *S_COUNT = "k_ha_cross_count", *S_FILL = "k_ha_cross_fill", *S_PAIRS = "k_ha_pairs", *S_EMIT = "k_ha_emit";

    // box: min s, max s of the family along u, then of the family along (-uy, ux); F is the first family
    static __device__ __forceinline__ void box_clear(long long* b) { b[0] = LLONG_MAX; b[1] = LLONG_MIN; b[2] = LLONG_MAX; b[3] = LLONG_MIN; }
    static __device__ __forceinline__ void box_add(long long* b, int2 r, const HaDir& F) {
        const long long s0 = -F.uy * r.x + F.ux * r.y, s1 = -F.ux * r.x - F.uy * r.y;
        atomicMin(&b[0], s0); atomicMax(&b[1], s0); atomicMin(&b[2], s1); atomicMax(&b[3], s1);
    }
    // the first line and the number of lines of a group
    static __device__ __forceinline__ void lines(const long long* b, int fam, const HaDir& F, long long& k0, long long& n) {
        const long long lo = b[2 * fam], hi = b[2 * fam + 1];
        if (lo > hi) { k0 = 0; n = 0; return; }                              // a group without points
        const long long first = ht_floordiv(lo, F.D) + 1, last = ht_floordiv(hi, F.D);
        k0 = first;
        n = last >= first ? last - first + 1 : 0;
    }
    static __device__ __forceinline__ long long line0(long long k0) { return k0; }  // first[g] is k0, the number of the group's first line
    // the edge from point j to its successor, ordered to s_a < s_b, and the lines klo .. khi that it crosses (s_a < k D <= s_b); false: none
    static __device__ __forceinline__ bool edge(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t j, const HaDir& F,
                                                const long long* __restrict__ k0, const long long* __restrict__ nl, HaEdge& e) {
        e.g = pgrp[j];
        if (e.g < 0) return false;
        const int2 a = q[j], b = q[nxt[j]];
        long long sa = -F.uy * a.x + F.ux * a.y, sb = -F.uy * b.x + F.ux * b.y, wa = F.ux * a.x + F.uy * a.y, wb = F.ux * b.x + F.uy * b.y;
        if (sa == sb) return false;
        if (sa > sb) { long long t = sa; sa = sb; sb = t; t = wa; wa = wb; wb = t; }
        e.sa = sa; e.sb = sb; e.wa = wa; e.wb = wb;
        const long long first = k0[e.g];
        e.klo = max(first, ht_floordiv(sa, F.D) + 1);                        // the group's range says so already; the clamps keep every row inside it
        e.khi = min(ht_floordiv(sb, F.D), first + nl[e.g] - 1);
        return e.khi >= e.klo;
    }
    static __device__ __forceinline__ void cross(const HaEdge& e, const HaDir& F, long long, long long k, unsigned row, long long p, HaX* __restrict__ xs, unsigned*) {
        const long long den = e.sb - e.sa;
        const u128 num = (u128)((i128)e.wa * den + (i128)(k * F.D - e.sa) * (e.wb - e.wa));
        xs[p] = HaX{(u64)num, (u64)(num >> 64), (u64)den, row, 0u};
    }
    static __device__ __forceinline__ unsigned row(const HaX* __restrict__ xs, const unsigned*, int64_t i) { return xs[i].row; }
    // the pair of crossings i, i + 1 of one row: 0 dropped (we <= ws), 1 kept, 2 collapsed; a, b: the rounded ends in ascending w
    static __device__ __forceinline__ int pair(const HaX* __restrict__ xs, int64_t i, const HaDir& F, long long kD, int2& a, int2& b) {
        const HaX x0 = xs[i], x1 = xs[i + 1];
        const i128 n0 = ha_num(x0), n1 = ha_num(x1);
        const long long d0 = (long long)x0.den, d1 = (long long)x1.den;
        if (d0 <= 0 || d1 <= 0) return 0;
        if (!(n1 * d0 - n0 * d1 > (i128)(2 * F.I) * d0 * d1)) return 0;      // we > ws
        a = ha_point(F, n0 + (i128)F.I * d0, d0, kD);
        b = ha_point(F, n1 - (i128)F.I * d1, d1, kD);
        return (a.x == b.x && a.y == b.y) ? 2 : 1;
    }
    static __device__ __forceinline__ int keep(const HaX* __restrict__ xs, int64_t i, const HaDir& F, const long long* __restrict__ rowbase, const long long* __restrict__ k0, int64_t G,
                                               long long row) {
        int64_t g; int2 a, b;
        return pair(xs, i, F, ht_row_line<HaRule>(rowbase, k0, G, row, g) * F.D, a, b);
    }
    static __device__ __forceinline__ int ends(const HaX* __restrict__ xs, int64_t i, const HaDir& F, long long, long long k, double spm, double2& a, double2& b) {
        int2 pa, pb;
        const int r = pair(xs, i, F, k * F.D, pa, pb);
        if (r != 1) return r;
        a = make_double2(ht_mm((double)pa.x, spm), ht_mm((double)pa.y, spm));
        b = make_double2(ht_mm((double)pb.x, spm), ht_mm((double)pb.y, spm));
        return 1;
    }
    static int sort_rows(orip_ctx* c, const char* who, HaX* xs, HaX* xs2, const unsigned* rowoff, const unsigned* rowcnt, const unsigned* medlist, int64_t R, int64_t X, const HtCounters& h) {
        hipStream_t s = LN(c).stream;
        if (h.n_big) {
            ProfScope ps(c, "ha_sort_merge");
            HIPC_AS(c, who, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::merge_sort(tmp, bytes, xs, xs2, (size_t)X, HaLess(), s); }));
            return 0;
        }
        { ProfScope ps(c, "k_ha_sort_wave");
          hipLaunchKernelGGL(k_ha_sort_wave, dim3(cdiv(R, 4)), dim3(256), 0, s, xs, xs2, rowoff, rowcnt, R); }
        if (h.n_med) { ProfScope ps(c, "k_ha_sort_block");
          hipLaunchKernelGGL(k_ha_sort_block, dim3(h.n_med), dim3(256), 0, s, xs, xs2, rowoff, rowcnt, medlist, h.n_med); }
        return 0;
    }
};

// the nearest integer to sqrt(v), v < 2^88: (isqrt(4 v) + 1) >> 1
long long ha_rs(u128 v) {
    const u128 t = 4 * v;
    u64 lo = 0, hi = 1ull << 46;                                             // lo^2 <= t < hi^2
    while (hi - lo > 1) { const u64 mid = lo + (hi - lo) / 2; if ((u128)mid * mid <= t) lo = mid; else hi = mid; }
    return (long long)((lo + 1) >> 1);
}
}  // namespace

extern "C" int orip_svg_hatch_angle(orip_ctx* c, const int32_t* fill_group, int64_t n_sub, double steps_per_mm, int32_t spacing, int32_t inset, int32_t ux, int32_t uy, int32_t flags,
                                    int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    HtGroups grp;
    ORIP_TRY(ht_intake(c, __func__, fill_group, n_sub, steps_per_mm, spacing, inset, flags, stats, 5, grp));
    if ((ux == 0 && uy == 0) || ux < -HA_UMAX || ux > HA_UMAX || uy < -HA_UMAX || uy > HA_UMAX)
        ORIP_FAIL(c, "hatch direction (%d, %d): not zero, each component within +-4096", ux, uy);
    const long long U2 = (long long)ux * ux + (long long)uy * uy;
    const long long D = ha_rs((u128)((u64)spacing * (u64)spacing) * (u64)U2), I = ha_rs((u128)((u64)inset * (u64)inset) * (u64)U2);
    const HaDir dir[2] = {HaDir{ux, uy, U2, D, I}, HaDir{-(long long)uy, ux, U2, D, I}};
    return ht_fill<HaRule>(c, __func__, grp, n_sub, steps_per_mm, flags, dir, stats);
}
