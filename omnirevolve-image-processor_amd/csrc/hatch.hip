// csrc/hatch.hip -- hatch fill of the fitted SVG paths: hatch_fill of the reference's demo sheet generator (stream_generators/plotter_demo/
// omnirevolve_plotter_demo.py:220-260) for every fill group of a drawing at once.  The reference loops lines x edges per group in Python; here the same
// integers come out of edge -> row binning, a scan, a sort inside each row and a pairing pass.  include/orip.h states the rules; hatch_common.h states the
// frame that runs them (the kernels' heads, the per-direction driver, the call's prelude and commit) and numbers its steps; HtRule below is what this
// hatch puts into them, and hatch_angle.hip (the exact hatch along any direction) puts its own rule into the same frame.
//
// 0. Quantise.  |q| >= 2^30 raises the flag; integer atomicMin / atomicMax give each group's box (min x, min y, max x, max y).
// Then per direction (for the vertical one every point is read as (y, x)):
// 1. Lines.  y0 and the number of lines (:230-236); line k counts from 0 at y0.
// 2. Chunks.  An edge, ordered to y1 < y2, crosses the lines k with y1 < y0 + k * spacing <= y2.
// 3. Fill.  x = x1 + t * (x2 - x1) (:246-247, every operation rounded on its own), a double; the row travels beside it in `crow`.  Equal doubles are
//    indistinguishable to every later step.
// 4. Sort, ascending in x: up to 64 crossings one wave in registers (bitonic over __shfl_xor), up to 2048 one block in LDS (bitonic, 16 KB), anything larger
//    rocPRIM's segmented radix sort, which is handed empty segments for all other rows.  Each path writes its own rows of the sorted copy.
// 5. Pair.  sx = trunc(x_a + inset), ex = trunc(x_b - inset), kept when ex > sx (:250-254).  Nothing collapses.
// 6. Emit.  (sx, y) and (ex, y), reversed on odd lines under serpentine (:255-260).
#include "hatch_common.h"
#include <rocprim/rocprim.hpp>
#include <climits>
#include <cmath>

namespace {
__global__ __launch_bounds__(256) void k_ht_sort_wave(const double* __restrict__ xs, double* __restrict__ out, const unsigned* __restrict__ rowoff, const unsigned* __restrict__ rowcnt, int64_t R) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const unsigned lane = threadIdx.x & 63;
    if (r >= R) return;
    const unsigned n = rowcnt[r];
    if (n == 0 || n > HT_WAVE_MAX) return;                                   // the whole wave leaves together
    const unsigned o = rowoff[r];
    double v = lane < n ? xs[o + lane] : INFINITY;
    for (unsigned k = 2; k <= 64; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            const double w = __shfl_xor(v, (int)j, 64);
            const bool up = (lane & k) == 0, low = (lane & j) == 0;
            v = up == low ? fmin(v, w) : fmax(v, w);
        }
    if (lane < n) out[o + lane] = v;
}

__global__ __launch_bounds__(256) void k_ht_sort_block(const double* __restrict__ xs, double* __restrict__ out, const unsigned* __restrict__ rowoff, const unsigned* __restrict__ rowcnt,
                                                       const unsigned* __restrict__ medlist, unsigned n_med) {
    __shared__ double sh[HT_BLOCK_MAX];
    if (blockIdx.x >= n_med) return;
    const unsigned r = medlist[blockIdx.x], n = rowcnt[r], o = rowoff[r];
    if (n > HT_BLOCK_MAX) return;
    unsigned m = 128;
    while (m < n) m <<= 1;
    for (unsigned i = threadIdx.x; i < m; i += 256) sh[i] = i < n ? xs[o + i] : INFINITY;
    __syncthreads();
    for (unsigned k = 2; k <= m; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = threadIdx.x; i < m; i += 256) {
                const unsigned p = i ^ j;
                if (p > i) {
                    const double a = sh[i], b = sh[p];
                    if ((a > b) == ((i & k) == 0)) { sh[i] = b; sh[p] = a; }
                }
            }
            __syncthreads();
        }
    for (unsigned i = threadIdx.x; i < n; i += 256) out[o + i] = sh[i];
}

// the segments of the segmented sort: a row beyond the block sort is its range of crossings, every other row is empty
struct HtBigSeg {
    const unsigned* off; const unsigned* cnt; unsigned end;
    __host__ __device__ unsigned operator()(unsigned r) const { return off[r] + (end && cnt[r] > HT_BLOCK_MAX ? cnt[r] : 0u); }
};

struct HtDir { int vert, spacing, inset; };                                  // one direction
struct HtEdge { long long x1, y1, x2, y2, klo, khi; int g; };

struct HtRule {
    typedef HtDir Dir; typedef int Box; typedef HtEdge Edge; typedef double X;
    static constexpr double QLIM = 1073741824.0;
    static constexpr bool CROW = true, COLLAPSED = false;
    static constexpr const char *QLIM_MSG = "a coordinate reaches 2^30 hatch units at %g steps per mm";
    static constexpr const char *S_QUANT = "k_ht_quant", *S_COUNT = "k_ht_cross_count", *S_FILL = "k_ht_cross_fill", *S_PAIRS = "k_ht_pairs", *S_EMIT = "k_ht_emit";

    static __device__ __forceinline__ void box_clear(int* b) { b[0] = INT_MAX; b[1] = INT_MAX; b[2] = INT_MIN; b[3] = INT_MIN; }
    static __device__ __forceinline__ void box_add(int* b, int2 r, const HtDir&) { atomicMin(&b[0], r.x); atomicMin(&b[1], r.y); atomicMax(&b[2], r.x); atomicMax(&b[3], r.y); }
    // y0 and the number of lines of a group (:230-236)
    static __device__ __forceinline__ void lines(const int* b, int, const HtDir& F, long long& y0, long long& n) {
        const long long lo = b[F.vert ? 0 : 1], hi = b[F.vert ? 2 : 3];
        const long long b0 = ht_floordiv(lo + F.spacing / 2, F.spacing) * F.spacing;
        y0 = b0;
        n = hi >= b0 ? (hi - b0) / F.spacing + 1 : 0;
    }
    static __device__ __forceinline__ long long line0(long long) { return 0; }      // first[g] is y0, a coordinate: line 0 lies there
    // the edge from point j to its successor, ordered to y1 < y2, and the lines klo .. khi of its group that it crosses (y1 < y <= y2); false: none
    static __device__ __forceinline__ bool edge(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t j, const HtDir& F,
                                                const long long* __restrict__ y0, const long long* __restrict__ nl, HtEdge& e) {
        e.g = pgrp[j];
        if (e.g < 0) return false;
        int2 a = q[j], b = q[nxt[j]];
        if (F.vert) { a = make_int2(a.y, a.x); b = make_int2(b.y, b.x); }
        if (a.y == b.y) return false;
        if (a.y > b.y) { const int2 t = a; a = b; b = t; }
        e.x1 = a.x; e.y1 = a.y; e.x2 = b.x; e.y2 = b.y;
        const long long base = y0[e.g];
        e.klo = max(0ll, ht_floordiv(e.y1 - base, F.spacing) + 1);
        e.khi = min(ht_floordiv(e.y2 - base, F.spacing), nl[e.g] - 1);        // y2 <= max_y says so already; the clamp keeps every row inside the group's range
        return e.khi >= e.klo;
    }
    static __device__ __forceinline__ void cross(const HtEdge& e, const HtDir& F, long long y0, long long k, unsigned row, long long p, double* __restrict__ xs, unsigned* __restrict__ crow) {
        const double t = __ddiv_rn((double)(y0 + k * F.spacing - e.y1), (double)(e.y2 - e.y1));
        xs[p] = sv_add((double)e.x1, sv_mul(t, (double)(e.x2 - e.x1)));
        crow[p] = row;
    }
    static __device__ __forceinline__ unsigned row(const double*, const unsigned* __restrict__ crow, int64_t i) { return crow[i]; }
    static __device__ __forceinline__ bool pair(const double* __restrict__ xs, int64_t i, int inset, long long& sx, long long& ex) {
        sx = (long long)sv_add(xs[i], (double)inset); ex = (long long)sv_sub(xs[i + 1], (double)inset);      // int(): toward zero
        return ex > sx;
    }
    static __device__ __forceinline__ int keep(const double* __restrict__ xs, int64_t i, const HtDir& F, const long long*, const long long*, int64_t, long long) {
        long long sx, ex;
        return pair(xs, i, F.inset, sx, ex);
    }
    static __device__ __forceinline__ int ends(const double* __restrict__ xs, int64_t i, const HtDir& F, long long y0, long long k, double spm, double2& a, double2& b) {
        long long sx, ex;
        if (!pair(xs, i, F.inset, sx, ex)) return 0;
        const double pa = ht_mm((double)sx, spm), pb = ht_mm((double)ex, spm), l = ht_mm((double)(y0 + k * F.spacing), spm);
        a = F.vert ? make_double2(l, pa) : make_double2(pa, l);
        b = F.vert ? make_double2(l, pb) : make_double2(pb, l);
        return 1;
    }
    static int sort_rows(orip_ctx* c, const char* who, double* xs, double* xs2, const unsigned* rowoff, const unsigned* rowcnt, const unsigned* medlist, int64_t R, int64_t X, const HtCounters& h) {
        hipStream_t s = LN(c).stream;
        { ProfScope ps(c, "k_ht_sort_wave");
          hipLaunchKernelGGL(k_ht_sort_wave, dim3(cdiv(R, 4)), dim3(256), 0, s, xs, xs2, rowoff, rowcnt, R); }
        if (h.n_med) { ProfScope ps(c, "k_ht_sort_block");
          hipLaunchKernelGGL(k_ht_sort_block, dim3(h.n_med), dim3(256), 0, s, xs, xs2, rowoff, rowcnt, medlist, h.n_med); }
        if (h.n_big) {
            ProfScope ps(c, "ht_sort_segmented");
            auto rows = rocprim::counting_iterator<unsigned>(0u);
            auto first = rocprim::make_transform_iterator(rows, HtBigSeg{rowoff, rowcnt, 0u}), last = rocprim::make_transform_iterator(rows, HtBigSeg{rowoff, rowcnt, 1u});
            HIPC_AS(c, who, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::segmented_radix_sort_keys(tmp, bytes, xs, xs2, (unsigned)X, (unsigned)R, first, last, 0u, 64u, s); }));
        }
        return 0;
    }
};
}  // namespace

extern "C" int orip_svg_hatch(orip_ctx* c, const int32_t* fill_group, int64_t n_sub, double steps_per_mm, int32_t spacing, int32_t inset, int32_t flags, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    HtGroups grp;
    ORIP_TRY(ht_intake(c, __func__, fill_group, n_sub, steps_per_mm, spacing, inset, flags, stats, 4, grp));
    const HtDir dir[2] = {HtDir{0, spacing, inset}, HtDir{1, spacing, inset}};
    return ht_fill<HtRule>(c, __func__, grp, n_sub, steps_per_mm, flags, dir, stats);
}

extern "C" int orip_svg_hatch_groups_fetch(orip_ctx* c, int32_t* group_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!c->sv_ready || !c->sv_hatched) ORIP_FAIL(c, "no hatch lines: orip_svg_hatch has not succeeded on the resident paths");
    if (c->ht_nseg == 0) return 0;
    if (!group_out) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(group_out, c->ht_grp.p, (size_t)c->ht_nseg * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
