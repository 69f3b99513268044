// csrc/hatch.hip -- hatch fill of the fitted SVG paths: hatch_fill of the reference's demo sheet generator (stream_generators/plotter_demo/
// omnirevolve_plotter_demo.py:220-260) for every fill group of a drawing at once.  The reference loops lines x edges per group in Python; here the same
// integers come out of edge -> row binning, a scan, a sort inside each row and a pairing pass.  include/orip.h states the rules; this is how they run.
//
// 0. Quantise.  One thread per resident point: q = rint(v * steps_per_mm), its subpath by binary search, from it the fill group and the successor of the
//    point in its closed subpath (poly[(i + 1) % n], :242); integer atomicMin / atomicMax give each group's box.  |q| >= 2^30 raises a flag.
// Then per direction (for the vertical one every point is read as (y, x)):
// 1. Lines.  One thread per group: y0 and the number of lines (:230-236); an exclusive scan gives each group its first global row.
// 2. Chunks.  One thread per edge: the range of lines k with y1 < y0 + k * spacing <= y2, cut into chunks of at most 64 lines, so that an edge spanning
//    thousands of rows is the work of many threads; a scan of the chunk counts places them.  The crossings are summed for the size check.
// 3. Count, scan, fill.  One thread per chunk (its edge by binary search) adds 1 to each of its rows; after an exclusive scan of the rows' counts the same
//    kernel runs again and writes x = x1 + t * (x2 - x1) (:246-247, every operation rounded on its own) through a cursor per row.  The arrival order inside
//    a row is arbitrary; the sort removes it, and equal doubles are indistinguishable.
// 4. Sort inside each row, by its count: up to 64 crossings one wave in registers (bitonic over __shfl_xor), up to 2048 one block in LDS (bitonic), anything
//    larger rocPRIM's segmented radix sort, which is handed empty segments for all other rows.  Each path writes its own rows of the sorted copy.
// 5. Pair.  One thread per crossing: an even place with a successor in its row is a pair (:250-251); sx = trunc(x_a + inset), ex = trunc(x_b - inset), kept
//    when ex > sx (:252-254).  An exclusive scan of the kept flags is the output order: groups ascending, lines ascending, pairs ascending in x.
// 6. Emit.  One thread per kept pair appends a 2-point path behind the resident ones, reversed on odd lines under serpentine (:255-260), each coordinate
//    k -> k / steps_per_mm rounded to 4 decimals as the fit rounds.
// Nothing is committed (sv_n, sv_total) before the last kernel of the last direction has run, so an error leaves the resident paths as they were.  Every
// index is bounded by a count computed on the device and checked on the host before the buffers are sized: rows by the scanned line counts, crossings by
// the scanned row counts, outputs by the scanned kept flags.  The limits, the counters, k_ht_classify and the intake of a call are in hatch_common.h, which
// hatch_angle.hip (the exact hatch along any direction) shares.
#include "hatch_common.h"
#include "sv_round.h"
#include <rocprim/rocprim.hpp>
#include <climits>
#include <cmath>

namespace {
constexpr double HT_QLIM = 1073741824.0;

__global__ __launch_bounds__(256) void k_ht_box_init(int* __restrict__ box, int64_t G) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < G) { box[4 * g] = INT_MAX; box[4 * g + 1] = INT_MAX; box[4 * g + 2] = INT_MIN; box[4 * g + 3] = INT_MIN; }
}

__global__ __launch_bounds__(256) void k_ht_quant(const long long* __restrict__ off, const double2* __restrict__ pts, const int* __restrict__ gid, int64_t P, int64_t total, double spm,
                                                  int2* __restrict__ q, int* __restrict__ pgrp, int* __restrict__ nxt, int* __restrict__ box, HtCounters* __restrict__ cn) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    int64_t lo = 0, hi = P;                                                  // last p with off[p] <= j
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= j) lo = mid; else hi = mid; }
    const double2 v = pts[j];
    const double fx = rint(sv_mul(v.x, spm)), fy = rint(sv_mul(v.y, spm));
    int2 r = make_int2(0, 0);
    if (fabs(fx) < HT_QLIM && fabs(fy) < HT_QLIM) r = make_int2((int)fx, (int)fy);      // not so for a NaN either
    else atomicOr(&cn->err, 1);
    const int g = gid[lo];
    q[j] = r; pgrp[j] = g;
    nxt[j] = (int)(j + 1 == off[lo + 1] ? off[lo] : j + 1);
    if (g >= 0) { atomicMin(&box[4 * g], r.x); atomicMin(&box[4 * g + 1], r.y); atomicMax(&box[4 * g + 2], r.x); atomicMax(&box[4 * g + 3], r.y); }
}

// y0 and the number of lines of every group (:230-236); nl[G] = 0 closes the scan
__global__ __launch_bounds__(256) void k_ht_lines(const int* __restrict__ box, int64_t G, int spacing, int vert, long long* __restrict__ y0, long long* __restrict__ nl) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > G) return;
    if (g == G) { nl[g] = 0; return; }
    const long long lo = box[4 * g + (vert ? 0 : 1)], hi = box[4 * g + (vert ? 2 : 3)];
    const long long b = ht_floordiv(lo + spacing / 2, spacing) * spacing;
    y0[g] = b;
    nl[g] = hi >= b ? (hi - b) / spacing + 1 : 0;
}

struct HtEdge { long long x1, y1, x2, y2, klo, khi; int g; };
// the edge from point j to its successor, ordered to y1 < y2, and the lines klo .. khi of its group that it crosses (y1 < y <= y2); false: none
__device__ __forceinline__ bool ht_edge(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t j, int vert,
                                        const long long* __restrict__ y0, const long long* __restrict__ nl, int spacing, HtEdge& e) {
    e.g = pgrp[j];
    if (e.g < 0) return false;
    int2 a = q[j], b = q[nxt[j]];
    if (vert) { a = make_int2(a.y, a.x); b = make_int2(b.y, b.x); }
    if (a.y == b.y) return false;
    if (a.y > b.y) { const int2 t = a; a = b; b = t; }
    e.x1 = a.x; e.y1 = a.y; e.x2 = b.x; e.y2 = b.y;
    const long long base = y0[e.g];
    e.klo = max(0ll, ht_floordiv(e.y1 - base, spacing) + 1);
    e.khi = min(ht_floordiv(e.y2 - base, spacing), nl[e.g] - 1);              // y2 <= max_y says so already; the clamp keeps every row inside the group's range
    return e.khi >= e.klo;
}

__global__ __launch_bounds__(256) void k_ht_chunks(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t total, int vert,
                                                   const long long* __restrict__ y0, const long long* __restrict__ nl, int spacing, long long* __restrict__ chunkn,
                                                   HtCounters* __restrict__ cn) {
    __shared__ unsigned long long sum;
    if (threadIdx.x == 0) sum = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j <= total) {
        HtEdge e;
        long long n = 0;
        if (j < total && ht_edge(q, pgrp, nxt, j, vert, y0, nl, spacing, e)) n = e.khi - e.klo + 1;
        chunkn[j] = (n + HT_CHUNK - 1) / HT_CHUNK;
        if (n) atomicAdd(&sum, (unsigned long long)n);
    }
    __syncthreads();
    if (threadIdx.x == 0 && sum) atomicAdd(&cn->crossings, sum);
}

// one thread per chunk of at most HT_CHUNK lines of one edge.  FILL false: counts per row; true: the crossings through the rows' cursors
template <bool FILL>
__global__ __launch_bounds__(256) void k_ht_cross(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t total, int vert,
                                                  const long long* __restrict__ y0, const long long* __restrict__ nl, const long long* __restrict__ rowbase, int spacing,
                                                  const long long* __restrict__ chunkoff, int64_t C, int64_t R, int64_t X, unsigned* __restrict__ rowcnt,
                                                  const unsigned* __restrict__ rowoff, double* __restrict__ xs, unsigned* __restrict__ crow) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int64_t lo = 0, hi = total;                                              // last edge with chunkoff[edge] <= c: the one that owns chunk c
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (chunkoff[mid] <= c) lo = mid; else hi = mid; }
    HtEdge e;
    if (!ht_edge(q, pgrp, nxt, lo, vert, y0, nl, spacing, e)) return;
    const long long k0 = e.klo + (long long)HT_CHUNK * (c - chunkoff[lo]), k1 = min(e.khi, k0 + HT_CHUNK - 1);
    const long long base = y0[e.g], rb = rowbase[e.g];
    const double dy = (double)(e.y2 - e.y1), dx = (double)(e.x2 - e.x1), x1 = (double)e.x1;
    for (long long k = k0; k <= k1; k++) {
        const long long row = rb + k;
        if (row < 0 || row >= R) continue;
        if (!FILL) { atomicAdd(&rowcnt[row], 1u); continue; }
        const long long p = (long long)rowoff[row] + atomicAdd(&rowcnt[row], 1u);
        if (p >= X) continue;
        const double t = __ddiv_rn((double)(base + k * spacing - e.y1), dy);
        xs[p] = sv_add(x1, sv_mul(t, dx));
        crow[p] = (unsigned)row;
    }
}

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

__device__ __forceinline__ bool ht_pair(const double* __restrict__ xs, int64_t i, int inset, long long& sx, long long& ex) {
    sx = (long long)sv_add(xs[i], (double)inset); ex = (long long)sv_sub(xs[i + 1], (double)inset);      // int(): toward zero
    return ex > sx;
}

__global__ __launch_bounds__(256) void k_ht_pairs(const double* __restrict__ xs, const unsigned* __restrict__ crow, const unsigned* __restrict__ rowoff, const unsigned* __restrict__ rowcnt,
                                                  int64_t X, int64_t R, int inset, unsigned* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > X) return;
    unsigned kp = 0;
    if (i < X) {
        const unsigned row = crow[i];
        if (row < R) {
            const unsigned li = (unsigned)(i - rowoff[row]);
            long long sx, ex;
            if ((li & 1) == 0 && li + 1 < rowcnt[row] && i + 1 < X) kp = ht_pair(xs, i, inset, sx, ex);
        }
    }
    keep[i] = kp;
}

__global__ __launch_bounds__(256) void k_ht_emit(const double* __restrict__ xs, const unsigned* __restrict__ crow, const unsigned* __restrict__ keep, const unsigned* __restrict__ kpos, int64_t X,
                                                 const long long* __restrict__ rowbase, int64_t G, const long long* __restrict__ y0, int spacing, int inset, int serpentine, int vert,
                                                 double spm, int64_t n0, int64_t t0, int64_t S, long long* __restrict__ off_out, double2* __restrict__ pts_out, const int* __restrict__ gnum,
                                                 int* __restrict__ grp_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= X || !keep[i]) return;
    const int64_t s = kpos[i];
    if (s >= S) return;
    const long long row = crow[i];
    int64_t lo = 0, hi = G;                                                  // last group with rowbase[group] <= row: the one that owns the row
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (rowbase[mid] <= row) lo = mid; else hi = mid; }
    const long long k = row - rowbase[lo], y = y0[lo] + k * spacing;
    long long sx, ex;
    ht_pair(xs, i, inset, sx, ex);
    const bool rev = serpentine && (k & 1);
    const double a = sv_round4(__ddiv_rn((double)(rev ? ex : sx), spm)), b = sv_round4(__ddiv_rn((double)(rev ? sx : ex), spm)), l = sv_round4(__ddiv_rn((double)y, spm));
    pts_out[t0 + 2 * s] = vert ? make_double2(l, a) : make_double2(a, l);
    pts_out[t0 + 2 * s + 1] = vert ? make_double2(l, b) : make_double2(b, l);
    off_out[n0 + s + 1] = t0 + 2 * (s + 1);
    grp_out[s] = gnum[lo];                                                   // the caller's number of the owning group
}

struct HtPlan {                       // what the directions share: the quantised points (ht_pts) and where the next segments go
    int2* q; int *pgrp, *nxt, *box, *gnum; HtCounters* cn; long long *y0, *nl, *rowbase, *chunkn, *chunkoff;
    int64_t G, total, n, tot, n_sub; int spacing, inset, serpentine; double spm;
};

// one direction: appends its segments behind path P.n / point P.tot (not committed) and moves both on
int ht_direction(orip_ctx* c, HtPlan& P, int vert, int64_t* stats) {
    hipStream_t s = LN(c).stream;
    const int64_t G = P.G, total = P.total;
    HIPC(c, hipMemsetAsync(P.cn, 0, sizeof(HtCounters), s));
    hipLaunchKernelGGL(k_ht_lines, dim3(cdiv(G + 1, 256)), dim3(256), 0, s, P.box, G, P.spacing, vert, P.y0, P.nl);
    ORIP_TRY(vscan_excl<int64_t>(c, (const int64_t*)P.nl, (int64_t*)P.rowbase, (size_t)G + 1));
    hipLaunchKernelGGL(k_ht_chunks, dim3(cdiv(total + 1, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, vert, P.y0, P.nl, P.spacing, P.chunkn, P.cn);
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
    unsigned *rowcnt, *rowoff, *medlist, *crow, *keep, *kpos; double *xs, *xs2;
    { Carve L; L.take(rowcnt, (size_t)R + 1); L.take(rowoff, (size_t)R + 1); L.take(medlist, (size_t)R); HIPC(c, L.commit(c->ht_rows, 64)); }
    { Carve L; L.take(xs, (size_t)X); L.take(xs2, (size_t)X); L.take(crow, (size_t)X); L.take(keep, (size_t)X + 1); L.take(kpos, (size_t)X + 1); HIPC(c, L.commit(c->ht_x, 64)); }
    HIPC(c, hipMemsetAsync(rowcnt, 0, (size_t)(R + 1) * 4, s));
    { ProfScope ps(c, "k_ht_cross_count");
      hipLaunchKernelGGL(k_ht_cross<false>, dim3(cdiv(C, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, vert, P.y0, P.nl, P.rowbase, P.spacing, P.chunkoff, (int64_t)C, (int64_t)R, (int64_t)X,
                         rowcnt, (const unsigned*)rowoff, xs, crow); }
    hipLaunchKernelGGL(k_ht_classify, dim3(cdiv(R + 1, 256)), dim3(256), 0, s, rowcnt, (int64_t)R, medlist, P.cn);
    ORIP_TRY(vscan_excl<unsigned>(c, rowcnt, rowoff, (size_t)R + 1));
    HIPC(c, hipMemsetAsync(rowcnt, 0, (size_t)(R + 1) * 4, s));
    { ProfScope ps(c, "k_ht_cross_fill");
      hipLaunchKernelGGL(k_ht_cross<true>, dim3(cdiv(C, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, vert, P.y0, P.nl, P.rowbase, P.spacing, P.chunkoff, (int64_t)C, (int64_t)R, (int64_t)X,
                         rowcnt, (const unsigned*)rowoff, xs, crow); }
    HIPC(c, hipGetLastError());
    unsigned xtot = 0;
    HIPC(c, hipMemcpyAsync(&xtot, rowoff + R, 4, hipMemcpyDeviceToHost, s)); HIPC(c, hipMemcpyAsync(&h, P.cn, sizeof h, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if ((long long)xtot != X) ORIP_FAIL(c, "the rows hold %u crossings, the edges %lld", xtot, X);
    { ProfScope ps(c, "k_ht_sort_wave");
      hipLaunchKernelGGL(k_ht_sort_wave, dim3(cdiv(R, 4)), dim3(256), 0, s, xs, xs2, rowoff, rowcnt, (int64_t)R); }
    if (h.n_med) { ProfScope ps(c, "k_ht_sort_block");
      hipLaunchKernelGGL(k_ht_sort_block, dim3(h.n_med), dim3(256), 0, s, xs, xs2, rowoff, rowcnt, medlist, h.n_med); }
    if (h.n_big) {
        ProfScope ps(c, "ht_sort_segmented");
        auto rows = rocprim::counting_iterator<unsigned>(0u);
        auto first = rocprim::make_transform_iterator(rows, HtBigSeg{rowoff, rowcnt, 0u}), last = rocprim::make_transform_iterator(rows, HtBigSeg{rowoff, rowcnt, 1u});
        HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::segmented_radix_sort_keys(tmp, bytes, xs, xs2, (unsigned)X, (unsigned)R, first, last, 0u, 64u, s); }));
    }
    hipLaunchKernelGGL(k_ht_pairs, dim3(cdiv(X + 1, 256)), dim3(256), 0, s, xs2, crow, rowoff, rowcnt, (int64_t)X, (int64_t)R, P.inset, keep);
    ORIP_TRY(vscan_excl<unsigned>(c, keep, kpos, (size_t)X + 1));
    unsigned S = 0;
    ORIP_TRY(vread(c, &S, (const unsigned*)kpos + X));
    stats[3] += S;
    if (S == 0) return 0;
    const int64_t n1 = P.n + S, t1 = P.tot + 2 * (int64_t)S;
    if (n1 >= HT_MAX_POINTS || t1 > HT_MAX_POINTS) ORIP_FAIL(c, "%lld paths with %lld points after hatching: at most 2^30 - 2 paths and 2^30 - 1 points", (long long)n1, (long long)t1);
    HIPC(c, c->sv_off.ensure((size_t)(n1 + 1) * 8 + 64, s, true)); HIPC(c, c->sv_pts.ensure((size_t)t1 * 16 + 64, s, true));
    HIPC(c, c->ht_grp.ensure((size_t)(n1 - P.n_sub) * 4 + 64, s, true));
    { ProfScope ps(c, "k_ht_emit");
      hipLaunchKernelGGL(k_ht_emit, dim3(cdiv(X, 256)), dim3(256), 0, s, xs2, crow, keep, kpos, (int64_t)X, P.rowbase, G, P.y0, P.spacing, P.inset, P.serpentine, vert, P.spm, P.n, P.tot, (int64_t)S,
                         c->sv_off.as<long long>(), c->sv_pts.as<double2>(), P.gnum, c->ht_grp.as<int>() + (P.n - P.n_sub)); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    P.n = n1; P.tot = t1;
    return 0;
}
}  // namespace

extern "C" int orip_svg_hatch(orip_ctx* c, const int32_t* fill_group, int64_t n_sub, double steps_per_mm, int32_t spacing, int32_t inset, int32_t flags, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats || n_sub < 0 || (n_sub > 0 && !fill_group)) ORIP_FAIL(c, "bad arguments");
    for (int k = 0; k < 4; k++) stats[k] = 0;
    HtGroups grp;
    ORIP_TRY(ht_intake(c, __func__, fill_group, n_sub, steps_per_mm, spacing, inset, flags, grp));
    const std::vector<int32_t>&gid = grp.gid, &gnum = grp.gnum;
    const int64_t G = grp.G;
    stats[0] = G;
    const int64_t total = c->sv_total;
    c->ht_nseg = 0;
    if (G == 0 || total == 0) { c->sv_hatched = true; return 0; }
    hipStream_t s = LN(c).stream;
    HtPlan P{};
    int* d_gid;
    { Carve L; L.take(d_gid, (size_t)n_sub); L.take(P.q, (size_t)total); L.take(P.pgrp, (size_t)total); L.take(P.nxt, (size_t)total); L.take(P.box, (size_t)4 * G); L.take(P.cn, 1);
      L.take(P.y0, (size_t)G); L.take(P.nl, (size_t)G + 1); L.take(P.rowbase, (size_t)G + 1); L.take(P.chunkn, (size_t)total + 1); L.take(P.chunkoff, (size_t)total + 1);
      L.take(P.gnum, (size_t)G); HIPC(c, L.commit(c->ht_pts, 64)); }
    P.G = G; P.total = total; P.n = c->sv_n; P.n_sub = c->sv_n; P.tot = total; P.spacing = spacing; P.inset = inset; P.serpentine = flags & ORIP_HATCH_SERPENTINE ? 1 : 0; P.spm = steps_per_mm;
    HIPC(c, hipMemcpyAsync(d_gid, gid.data(), (size_t)n_sub * 4, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(P.gnum, gnum.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(P.cn, 0, sizeof(HtCounters), s));
    hipLaunchKernelGGL(k_ht_box_init, dim3(cdiv(G, 256)), dim3(256), 0, s, P.box, G);
    { ProfScope ps(c, "k_ht_quant");
      hipLaunchKernelGGL(k_ht_quant, dim3(cdiv(total, 256)), dim3(256), 0, s, c->sv_off.as<long long>(), c->sv_pts.as<double2>(), d_gid, n_sub, total, steps_per_mm, P.q, P.pgrp, P.nxt, P.box, P.cn); }
    HIPC(c, hipGetLastError());
    HtCounters h;
    ORIP_TRY(vread(c, &h, (const HtCounters*)P.cn));
    if (h.err) ORIP_FAIL(c, "a coordinate reaches 2^30 hatch units at %g steps per mm", steps_per_mm);
    if (flags & ORIP_HATCH_HORIZONTAL) ORIP_TRY(ht_direction(c, P, 0, stats));
    if (flags & ORIP_HATCH_VERTICAL) ORIP_TRY(ht_direction(c, P, 1, stats));
    c->ht_nseg = P.n - c->sv_n;
    c->sv_n = P.n; c->sv_total = P.tot; c->sv_hatched = true; c->sv_box_ok = false;
    return 0;
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
