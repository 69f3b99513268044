// csrc/hatch_common.h -- the frame of the two hatch fills, stated once and templated on a rule (hatch.hip: HtRule, the reference's rule along X and Y;
// hatch_angle.hip: HaRule, ours, exact, along any direction).  A rule is a plain struct of types, constants and static functions; each unit's head comment
// lists what its rule puts into the steps below.
//
// 0. Quantise (k_hatch_quant).  One thread per resident point: its subpath by binary search, q = rint(v * steps_per_mm), |q| >= R::QLIM raises a flag;
//    from the subpath the fill group and the successor of the point in its closed subpath; R::box_add puts the point into its group's box with atomics.
// Then per direction (ht_direction), with the rule's direction record R::Dir passed by value:
// 1. Lines (k_hatch_lines).  One thread per group: R::lines gives the group's origin (first[g]: y0 or k0) and its number of lines; an exclusive scan gives
//    each group its first global row.
// 2. Chunks (k_hatch_chunks).  One thread per edge: R::edge gives the range of lines klo .. khi that it crosses, cut into chunks of at most HT_CHUNK lines,
//    so that an edge spanning thousands of rows is the work of many threads; a scan of the chunk counts places them.  The crossings are summed for the
//    size check.
// 3. Count, scan, fill (k_hatch_cross).  One thread per chunk (its edge by binary search) adds 1 to each of its rows; after an exclusive scan of the rows'
//    counts the same kernel runs again and R::cross writes the crossing of line k through a cursor per row.  The arrival order inside a row is arbitrary;
//    the sort removes it.  The row number travels in the record or in the separate array `crow` (R::CROW).
// 4. Sort inside each row by its class (k_ht_classify): up to HT_WAVE_MAX crossings one wave in registers, up to HT_BLOCK_MAX one block in LDS, anything
//    larger a rocPRIM sort.  R::sort_rows launches the rule's own kernels: the two bitonic networks stay one copy per rule (DESIGN 5 "hatch" says why).
// 5. Pair (k_hatch_pairs).  One thread per crossing: an even place with a successor in its row is a pair; R::keep decides 0 dropped, 1 kept, 2 collapsed
//    (counted).  An exclusive scan of the kept flags is the output order: groups ascending, lines ascending, pairs ascending along the line.
// 6. Emit (k_hatch_emit).  One thread per kept pair: the owning group by binary search, R::ends gives the two end points in mm (ht_mm), swapped on odd lines
//    under serpentine; the 2-point path goes behind the resident ones, the caller's group number into ht_grp.
// Nothing is committed (sv_n, sv_total, ht_nseg, the stats) before the last kernel of the last direction has run, so an error leaves the resident paths as
// they were.  Every index is bounded by a count computed on the device and checked on the host before the buffers are sized: rows by the scanned line
// counts, crossings by the scanned row counts, outputs by the scanned kept flags.
#pragma once
#include "vec_common.h"
#include "sv_round.h"
#include <vector>

namespace {
constexpr unsigned HT_WAVE_MAX = 64, HT_BLOCK_MAX = 2048;
constexpr int HT_CHUNK = 64;
constexpr int64_t HT_MAX_ROWS = 1ll << 26, HT_MAX_CROSSINGS = 1ll << 30, HT_MAX_POINTS = (1ll << 30) - 1;     // the last: what orip_gcode_to_steps accepts
constexpr double HT_MAX_SPM = 5000.0;

struct HtCounters { unsigned long long crossings; unsigned n_med, n_big; int err; int pad; };

__host__ __device__ __forceinline__ long long ht_floordiv(long long a, long long b) { const long long q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }     // b > 0
// the owner of v: the last index in [0, n) whose offset is <= v
__device__ __forceinline__ int64_t ht_owner(const long long* off, int64_t n, long long v) { return last_le((const int64_t*)off, n, v); }
// step k as mm, rounded to four decimals as the fit rounds
__device__ __forceinline__ double ht_mm(double k, double spm) { return sv_round4(__ddiv_rn(k, spm)); }

template <class R>
__global__ __launch_bounds__(256) void k_hatch_box_init(typename R::Box* __restrict__ box, int64_t G) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < G) R::box_clear(box + 4 * g);
}

template <class R>
__global__ __launch_bounds__(256) void k_hatch_quant(const long long* __restrict__ off, const double2* __restrict__ pts, const int* __restrict__ gid, int64_t P, int64_t total, double spm,
                                                     typename R::Dir F, int2* __restrict__ q, int* __restrict__ pgrp, int* __restrict__ nxt, typename R::Box* __restrict__ box,
                                                     HtCounters* __restrict__ cn) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const int64_t p = ht_owner(off, P, j);
    const double2 v = pts[j];
    const double fx = rint(sv_mul(v.x, spm)), fy = rint(sv_mul(v.y, spm));
    int2 r = make_int2(0, 0);
    if (fabs(fx) < R::QLIM && fabs(fy) < R::QLIM) r = make_int2((int)fx, (int)fy);      // not so for a NaN either
    else atomicOr(&cn->err, 1);
    const int g = gid[p];
    q[j] = r; pgrp[j] = g;
    nxt[j] = (int)(j + 1 == off[p + 1] ? off[p] : j + 1);
    if (g >= 0) R::box_add(box + 4 * g, r, F);
}

// the origin and the number of lines of every group; nl[G] = 0 closes the scan
template <class R>
__global__ __launch_bounds__(256) void k_hatch_lines(const typename R::Box* __restrict__ box, int64_t G, int fam, typename R::Dir F, long long* __restrict__ first, long long* __restrict__ nl) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > G) return;
    if (g == G) { nl[g] = 0; return; }
    R::lines(box + 4 * g, fam, F, first[g], nl[g]);
}

template <class R>
__global__ __launch_bounds__(256) void k_hatch_chunks(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t total, typename R::Dir F,
                                                      const long long* __restrict__ first, const long long* __restrict__ nl, long long* __restrict__ chunkn, HtCounters* __restrict__ cn) {
    __shared__ unsigned long long sum;
    if (threadIdx.x == 0) sum = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j <= total) {
        typename R::Edge e;
        long long n = 0;
        if (j < total && R::edge(q, pgrp, nxt, j, F, first, nl, e)) n = e.khi - e.klo + 1;
        chunkn[j] = (n + HT_CHUNK - 1) / HT_CHUNK;
        if (n) atomicAdd(&sum, (unsigned long long)n);
    }
    __syncthreads();
    if (threadIdx.x == 0 && sum) atomicAdd(&cn->crossings, sum);
}

// one thread per chunk of at most HT_CHUNK lines of one edge.  FILL false: counts per row; true: the crossings through the rows' cursors
template <class R, bool FILL>
__global__ __launch_bounds__(256) void k_hatch_cross(const int2* __restrict__ q, const int* __restrict__ pgrp, const int* __restrict__ nxt, int64_t total, typename R::Dir F,
                                                     const long long* __restrict__ first, const long long* __restrict__ nl, const long long* __restrict__ rowbase,
                                                     const long long* __restrict__ chunkoff, int64_t C, int64_t Rn, int64_t X, unsigned* __restrict__ rowcnt,
                                                     const unsigned* __restrict__ rowoff, typename R::X* __restrict__ xs, unsigned* __restrict__ crow) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t j = ht_owner(chunkoff, total, c);                          // the edge that owns chunk c
    typename R::Edge e;
    if (!R::edge(q, pgrp, nxt, j, F, first, nl, e)) return;
    const long long k0 = e.klo + (long long)HT_CHUNK * (c - chunkoff[j]), k1 = min(e.khi, k0 + HT_CHUNK - 1);
    const long long f = first[e.g], rb = rowbase[e.g] - R::line0(f);
    for (long long k = k0; k <= k1; k++) {
        const long long row = rb + k;
        if (row < 0 || row >= Rn) continue;
        if (!FILL) { atomicAdd(&rowcnt[row], 1u); continue; }
        const long long p = (long long)rowoff[row] + atomicAdd(&rowcnt[row], 1u);
        if (p >= X) continue;
        R::cross(e, F, f, k, (unsigned)row, p, xs, crow);
    }
}

// rows for the block sort go on a list (in any order); rows beyond it are counted: a non-zero count calls the large sort.  rowcnt[R] = 0 closes the scan
__global__ __launch_bounds__(256) void k_ht_classify(unsigned* __restrict__ rowcnt, int64_t R, unsigned* __restrict__ medlist, HtCounters* __restrict__ cn) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > R) return;
    if (r == R) { rowcnt[r] = 0; return; }
    const unsigned n = rowcnt[r];
    if (n > HT_BLOCK_MAX) atomicAdd(&cn->n_big, 1u);
    else if (n > HT_WAVE_MAX) { const unsigned i = atomicAdd(&cn->n_med, 1u); if (i < R) medlist[i] = (unsigned)r; }
}

// the group that owns a row, and the row's line number as the rule counts it
template <class R>
__device__ __forceinline__ long long ht_row_line(const long long* __restrict__ rowbase, const long long* __restrict__ first, int64_t G, long long row, int64_t& g) {
    g = ht_owner(rowbase, G, row);
    return R::line0(first[g]) + (row - rowbase[g]);
}

template <class R>
__global__ __launch_bounds__(256) void k_hatch_pairs(const typename R::X* __restrict__ xs, const unsigned* __restrict__ crow, const unsigned* __restrict__ rowoff,
                                                     const unsigned* __restrict__ rowcnt, int64_t X, int64_t Rn, typename R::Dir F, const long long* __restrict__ rowbase,
                                                     const long long* __restrict__ first, int64_t G, unsigned* __restrict__ keep, unsigned long long* __restrict__ collapsed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > X) return;
    unsigned kp = 0;
    if (i < X) {
        const unsigned row = R::row(xs, crow, i);
        if (row < Rn) {
            const unsigned li = (unsigned)(i - rowoff[row]);
            if ((li & 1) == 0 && li + 1 < rowcnt[row] && i + 1 < X) {
                const int r = R::keep(xs, i, F, rowbase, first, G, row);
                kp = r == 1;
                if (r == 2) atomicAdd(collapsed, 1ull);
            }
        }
    }
    keep[i] = kp;
}

template <class R>
__global__ __launch_bounds__(256) void k_hatch_emit(const typename R::X* __restrict__ xs, const unsigned* __restrict__ crow, const unsigned* __restrict__ keep, const unsigned* __restrict__ kpos,
                                                    int64_t X, int64_t Rn, const long long* __restrict__ rowbase, const long long* __restrict__ first, int64_t G, typename R::Dir F,
                                                    int serpentine, double spm, int64_t n0, int64_t t0, int64_t S, long long* __restrict__ off_out, double2* __restrict__ pts_out,
                                                    const int* __restrict__ gnum, int* __restrict__ grp_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= X || i + 1 >= X || !keep[i]) return;
    const int64_t s = kpos[i];
    if (s >= S) return;
    const long long row = R::row(xs, crow, i);
    if (row >= Rn) return;
    int64_t g; double2 a, b;
    const long long k = ht_row_line<R>(rowbase, first, G, row, g);
    if (R::ends(xs, i, F, first[g], k, spm, a, b) != 1) return;
    const bool rev = serpentine && (k & 1);
    pts_out[t0 + 2 * s] = make_double2(rev ? b.x : a.x, rev ? b.y : a.y);
    pts_out[t0 + 2 * s + 1] = make_double2(rev ? a.x : b.x, rev ? a.y : b.y);
    off_out[n0 + s + 1] = t0 + 2 * (s + 1);
    grp_out[s] = gnum[g];                                                    // the caller's number of the owning group
}

template <class R>
struct HtPlan {                       // what the directions share: the quantised points (ht_pts) and where the next segments go
    int2* q; int *pgrp, *nxt, *gnum; typename R::Box* box; HtCounters* cn; unsigned long long* collapsed; long long *first, *nl, *rowbase, *chunkn, *chunkoff;
    int64_t G, total, n, tot, n_sub; int serpentine; double spm;
};

// one direction: appends its segments behind path P.n / point P.tot (not committed) and moves both on
template <class R>
int ht_direction(orip_ctx* c, const char* who, HtPlan<R>& P, int fam, const typename R::Dir& F, int64_t* stats) {
    hipStream_t s = LN(c).stream;
    const int64_t G = P.G, total = P.total;
    HIPC_AS(c, who, hipMemsetAsync(P.cn, 0, sizeof(HtCounters), s));
    hipLaunchKernelGGL(k_hatch_lines<R>, dim3(cdiv(G + 1, 256)), dim3(256), 0, s, P.box, G, fam, F, P.first, P.nl);
    ORIP_TRY(vscan_excl<int64_t>(c, (const int64_t*)P.nl, (int64_t*)P.rowbase, (size_t)G + 1));
    hipLaunchKernelGGL(k_hatch_chunks<R>, dim3(cdiv(total + 1, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, F, P.first, P.nl, P.chunkn, P.cn);
    ORIP_TRY(vscan_excl<int64_t>(c, (const int64_t*)P.chunkn, (int64_t*)P.chunkoff, (size_t)total + 1));
    HIPC_AS(c, who, hipGetLastError());
    long long Rn = 0, C = 0; HtCounters h;
    HIPC_AS(c, who, hipMemcpyAsync(&Rn, P.rowbase + G, 8, hipMemcpyDeviceToHost, s)); HIPC_AS(c, who, hipMemcpyAsync(&C, P.chunkoff + total, 8, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipMemcpyAsync(&h, P.cn, sizeof h, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    const long long X = (long long)h.crossings;
    if (Rn < 0 || Rn > HT_MAX_ROWS) ORIP_FAIL_AS(c, who, "%lld hatch lines: at most 2^26", Rn);
    if (X < 0 || X > HT_MAX_CROSSINGS) ORIP_FAIL_AS(c, who, "%lld crossings: at most 2^30", X);
    if (C < 0 || C > X + total) ORIP_FAIL_AS(c, who, "%lld chunks for %lld crossings of %lld edges", C, X, (long long)total);
    stats[1] += Rn; stats[2] += X;
    if (X == 0) return 0;
    unsigned *rowcnt, *rowoff, *medlist, *crow = nullptr, *keep, *kpos; typename R::X *xs, *xs2;
    { Carve L; L.take(rowcnt, (size_t)Rn + 1); L.take(rowoff, (size_t)Rn + 1); L.take(medlist, (size_t)Rn); HIPC_AS(c, who, L.commit(c->ht_rows, 64)); }
    { Carve L; L.take(xs, (size_t)X); L.take(xs2, (size_t)X); if (R::CROW) L.take(crow, (size_t)X); L.take(keep, (size_t)X + 1); L.take(kpos, (size_t)X + 1);
      HIPC_AS(c, who, L.commit(c->ht_x, 64)); }
    HIPC_AS(c, who, hipMemsetAsync(rowcnt, 0, (size_t)(Rn + 1) * 4, s));
    { ProfScope ps(c, R::S_COUNT);
      hipLaunchKernelGGL((k_hatch_cross<R, false>), dim3(cdiv(C, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, F, P.first, P.nl, P.rowbase, P.chunkoff, (int64_t)C, (int64_t)Rn, (int64_t)X,
                         rowcnt, (const unsigned*)rowoff, xs, crow); }
    hipLaunchKernelGGL(k_ht_classify, dim3(cdiv(Rn + 1, 256)), dim3(256), 0, s, rowcnt, (int64_t)Rn, medlist, P.cn);
    ORIP_TRY(vscan_excl<unsigned>(c, rowcnt, rowoff, (size_t)Rn + 1));
    HIPC_AS(c, who, hipMemsetAsync(rowcnt, 0, (size_t)(Rn + 1) * 4, s));
    { ProfScope ps(c, R::S_FILL);
      hipLaunchKernelGGL((k_hatch_cross<R, true>), dim3(cdiv(C, 256)), dim3(256), 0, s, P.q, P.pgrp, P.nxt, total, F, P.first, P.nl, P.rowbase, P.chunkoff, (int64_t)C, (int64_t)Rn, (int64_t)X,
                         rowcnt, (const unsigned*)rowoff, xs, crow); }
    HIPC_AS(c, who, hipGetLastError());
    unsigned xtot = 0;
    HIPC_AS(c, who, hipMemcpyAsync(&xtot, rowoff + Rn, 4, hipMemcpyDeviceToHost, s)); HIPC_AS(c, who, hipMemcpyAsync(&h, P.cn, sizeof h, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    if ((long long)xtot != X) ORIP_FAIL_AS(c, who, "the rows hold %u crossings, the edges %lld", xtot, X);
    ORIP_TRY(R::sort_rows(c, who, xs, xs2, rowoff, rowcnt, medlist, (int64_t)Rn, (int64_t)X, h));
    { ProfScope ps(c, R::S_PAIRS);
      hipLaunchKernelGGL(k_hatch_pairs<R>, dim3(cdiv(X + 1, 256)), dim3(256), 0, s, xs2, crow, rowoff, rowcnt, (int64_t)X, (int64_t)Rn, F, P.rowbase, P.first, G, keep, P.collapsed); }
    ORIP_TRY(vscan_excl<unsigned>(c, keep, kpos, (size_t)X + 1));
    unsigned S = 0;
    ORIP_TRY(vread(c, &S, (const unsigned*)kpos + X));
    stats[3] += S;
    if (S == 0) return 0;
    const int64_t n1 = P.n + S, t1 = P.tot + 2 * (int64_t)S;
    if (n1 >= HT_MAX_POINTS || t1 > HT_MAX_POINTS)
        ORIP_FAIL_AS(c, who, "%lld paths with %lld points after hatching: at most 2^30 - 2 paths and 2^30 - 1 points", (long long)n1, (long long)t1);
    HIPC_AS(c, who, c->sv_off.ensure((size_t)(n1 + 1) * 8 + 64, s, true)); HIPC_AS(c, who, c->sv_pts.ensure((size_t)t1 * 16 + 64, s, true));
    HIPC_AS(c, who, c->ht_grp.ensure((size_t)(n1 - P.n_sub) * 4 + 64, s, true));
    { ProfScope ps(c, R::S_EMIT);
      hipLaunchKernelGGL(k_hatch_emit<R>, dim3(cdiv(X, 256)), dim3(256), 0, s, xs2, crow, keep, kpos, (int64_t)X, (int64_t)Rn, P.rowbase, P.first, G, F, P.serpentine, P.spm, P.n, P.tot, (int64_t)S,
                         c->sv_off.as<long long>(), c->sv_pts.as<double2>(), P.gnum, c->ht_grp.as<int>() + (P.n - P.n_sub)); }
    HIPC_AS(c, who, hipGetLastError());
    HIPC_AS(c, who, hipStreamSynchronize(s));
    P.n = n1; P.tot = t1;
    return 0;
}

// The groups in use renumbered 0 .. G - 1 in ascending order of their number (gid[p]: the rank of subpath p's group or -1; gnum[rank]: the caller's number).
struct HtGroups { std::vector<int32_t> gid, gnum; int64_t G = 0; };
// The intake of either hatch call: `stats` cleared, the state, the arguments both take, and the groups
inline int ht_intake(orip_ctx* c, const char* who, const int32_t* fill_group, int64_t n_sub, double steps_per_mm, int32_t spacing, int32_t inset, int32_t flags, int64_t* stats, int n_stats,
                     HtGroups& g) {
    if (!stats || n_sub < 0 || (n_sub > 0 && !fill_group)) ORIP_FAIL_AS(c, who, "bad arguments");
    for (int k = 0; k < n_stats; k++) stats[k] = 0;
    if (!c->sv_ready || !c->sv_fitted) ORIP_FAIL_AS(c, who, "no fitted paths: orip_svg_flatten and orip_svg_fit come first");
    if (c->sv_hatched) ORIP_FAIL_AS(c, who, "the resident paths are hatched already: flatten again first");
    if (n_sub != c->sv_n) ORIP_FAIL_AS(c, who, "%lld fill groups given, %lld paths resident", (long long)n_sub, (long long)c->sv_n);
    if (!(steps_per_mm > 0.0) || !(steps_per_mm <= HT_MAX_SPM)) ORIP_FAIL_AS(c, who, "steps per mm %g: hatching needs a value in (0, 5000], so that four decimals of a mm name every step", steps_per_mm);
    if (spacing < 1) ORIP_FAIL_AS(c, who, "hatch spacing %d steps: at least 1", spacing);
    if (inset < 0) ORIP_FAIL_AS(c, who, "hatch inset %d steps: at least 0", inset);
    if (!(flags & (ORIP_HATCH_HORIZONTAL | ORIP_HATCH_VERTICAL)) || (flags & ~(ORIP_HATCH_SERPENTINE | ORIP_HATCH_HORIZONTAL | ORIP_HATCH_VERTICAL)))
        ORIP_FAIL_AS(c, who, "flags %d: ORIP_HATCH_HORIZONTAL, ORIP_HATCH_VERTICAL or both, and ORIP_HATCH_SERPENTINE", flags);
    g.gid.assign((size_t)n_sub, -1);
    std::vector<int32_t> rank((size_t)n_sub, 0);
    for (int64_t p = 0; p < n_sub; p++) {
        if (fill_group[p] < -1 || fill_group[p] >= n_sub) ORIP_FAIL_AS(c, who, "subpath %lld: fill group %d of %lld", (long long)p, fill_group[p], (long long)n_sub);
        if (fill_group[p] >= 0) rank[fill_group[p]] = 1;
    }
    g.G = 0;
    for (int64_t k = 0; k < n_sub; k++) { const int32_t used = rank[k]; rank[k] = (int32_t)g.G; g.G += used; }
    for (int64_t p = 0; p < n_sub; p++) if (fill_group[p] >= 0) g.gid[p] = rank[fill_group[p]];
    g.gnum.assign((size_t)g.G, 0);                                             // rank -> the caller's number
    for (int64_t p = 0; p < n_sub; p++) if (g.gid[p] >= 0) g.gnum[g.gid[p]] = fill_group[p];
    return 0;
}

// Behind the intake: the plan carved and uploaded, the points quantised, the directions of `flags` run with dir[0] and dir[1], the result committed.
// stats[0 .. 3] = groups, lines, crossings, segments; stats[4] = the collapsed pairs where the rule counts them (R::COLLAPSED)
template <class R>
int ht_fill(orip_ctx* c, const char* who, const HtGroups& grp, int64_t n_sub, double steps_per_mm, int32_t flags, const typename R::Dir (&dir)[2], int64_t* stats) {
    const int64_t G = grp.G, total = c->sv_total;
    stats[0] = G;
    if (G == 0 || total == 0) { c->ht_nseg = 0; c->sv_hatched = true; return 0; }
    hipStream_t s = LN(c).stream;
    HtPlan<R> P{};
    int* d_gid;
    { Carve L; L.take(d_gid, (size_t)n_sub); L.take(P.q, (size_t)total); L.take(P.pgrp, (size_t)total); L.take(P.nxt, (size_t)total); L.take(P.box, (size_t)4 * G); L.take(P.cn, 1);
      if (R::COLLAPSED) L.take(P.collapsed, 1);
      L.take(P.first, (size_t)G); L.take(P.nl, (size_t)G + 1); L.take(P.rowbase, (size_t)G + 1); L.take(P.chunkn, (size_t)total + 1); L.take(P.chunkoff, (size_t)total + 1);
      L.take(P.gnum, (size_t)G); HIPC_AS(c, who, L.commit(c->ht_pts, 64)); }
    P.G = G; P.total = total; P.n = c->sv_n; P.n_sub = c->sv_n; P.tot = total; P.serpentine = flags & ORIP_HATCH_SERPENTINE ? 1 : 0; P.spm = steps_per_mm;
    HIPC_AS(c, who, hipMemcpyAsync(d_gid, grp.gid.data(), (size_t)n_sub * 4, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemcpyAsync(P.gnum, grp.gnum.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
    HIPC_AS(c, who, hipMemsetAsync(P.cn, 0, sizeof(HtCounters), s));
    if (R::COLLAPSED) HIPC_AS(c, who, hipMemsetAsync(P.collapsed, 0, 8, s));
    hipLaunchKernelGGL(k_hatch_box_init<R>, dim3(cdiv(G, 256)), dim3(256), 0, s, P.box, G);
    { ProfScope ps(c, R::S_QUANT);
      hipLaunchKernelGGL(k_hatch_quant<R>, dim3(cdiv(total, 256)), dim3(256), 0, s, c->sv_off.as<long long>(), c->sv_pts.as<double2>(), d_gid, n_sub, total, steps_per_mm, dir[0], P.q, P.pgrp, P.nxt,
                         P.box, P.cn); }
    HIPC_AS(c, who, hipGetLastError());
    HtCounters h;
    ORIP_TRY(vread(c, &h, (const HtCounters*)P.cn));
    if (h.err) ORIP_FAIL_AS(c, who, R::QLIM_MSG, steps_per_mm);
    int64_t st[4] = {0, 0, 0, 0};
    if (flags & ORIP_HATCH_HORIZONTAL) ORIP_TRY(ht_direction<R>(c, who, P, 0, dir[0], st));
    if (flags & ORIP_HATCH_VERTICAL) ORIP_TRY(ht_direction<R>(c, who, P, 1, dir[1], st));
    if (R::COLLAPSED) {
        unsigned long long coll = 0;
        ORIP_TRY(vread(c, &coll, (const unsigned long long*)P.collapsed));
        stats[4] = (int64_t)coll;
    }
    stats[1] = st[1]; stats[2] = st[2]; stats[3] = st[3];
    c->ht_nseg = P.n - c->sv_n;
    c->sv_n = P.n; c->sv_total = P.tot; c->sv_hatched = true; c->sv_box_ok = false;
    return 0;
}
}  // namespace
