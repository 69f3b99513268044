// csrc/fill.hip -- fill_layers of the raster pipeline: a colour mask is hatched on the canvas grid (orip_fill_mask, orip_fill_fetch; the rule is stated in
// include/orip.h, is exact in integers and has one answer for every input).  Ours: the reference has no such pass.
//
// A FAMILY is one direction u with its lines k = kmin .. kmin + L - 1: every k whose line can hold a sample of the canvas (the host bounds n.p over the
// canvas corners and widens by m, which is more than the m / 2 a rounded sample leaves its line; a line of the range without a sample costs its blocks
// and counts nowhere).  A ROW is a line of either family, the rows of the family along u first.  A BLOCK is 64 consecutive major coordinates a of one
// row: the work of one wave, one sample a lane; a row has NW = ceil(A / 64) blocks and block z = wbase + (k - kmin) NW + a / 64, so the blocks ascend as
// the segments leave: family, k, a.
//
// 1. k_fl_sample, one WAVE per block: every lane computes its sample (k, a), whether it exists and whether its pixel is INK (two floor divisions into the
//    mask's grid and one byte of the mask); a ballot gives the block's 64 ON bits, on[z].  lines, samples and on are summed per wave and added once; a
//    line is counted at its first existing sample (the existing samples of a line are one stretch of a, because b is monotone in a).
// 2. k_fl_count, one thread per block: run starts are w & ~(w << 1 | carry), the carry being the top bit of the row's block before, and run ends are the
//    mirror image; cs[z] = starts << 32 | ends.  One scan (gc_cut.h: gc_scan_u64) ranks both.  The i-th start of a row belongs to its i-th end and a row's
//    starts are as many as its ends, so over whole rows the rank of a start IS the rank of its end: no forward search, no walk along the line.
//    The host reads the runs R (first read-back) and sizes the per-run arrays.
// 3. k_fl_scatter, one wave per block with a bit set: a lane whose bit starts a run writes a0 and the row at the start's rank, a lane whose bit ends one
//    writes a1 at the end's rank.
// 4. k_fl_keep, one thread per run: s0 = a0 + im, s1 = a1 - im, keep = s1 - s0 >= lm; short and segments are summed per wave.  A scan of the keep flags
//    places the segments; the host reads their number (second read-back: 2^26 or more is refused).
// 5. k_fl_emit, one thread per kept run: the two samples again, at place kbase[r]; under ORIP_FILL_SERPENTINE a segment of a row with k & 1 counts from
//    the row's other end (the row's first and last place come from the two scans) and runs from s1 to s0: an index computation, not a second pass.
// Everything on the raster stages' stream, where the resident masks are written; a third read-back fetches the counters behind the last launch.
//
// Scratch (orip_ctx.h states the three buffers).  c->fl_tmp, ONE Carve: mask u8[h w] (explicit form only); on u64[Z + 1]; cs u64[Z + 1]; sc u64[Z + 1];
// FlCounters.  c->fl_runs, one Carve behind the first read-back, R runs: a0 int[R]; a1 int[R]; row int[R]; keep u64[R + 1]; kbase u64[R + 1].  Resident
// until the next call: c->fl_out = seg int4[segments]; c->fl_rows = segrow int[segments] (the row of every segment) and rfirst unsigned[rows + 1] (the first
// segment of every row; k_fl_rowfirst), which only orip_fill_link (fill_link.hip) reads.
#include "orip_ctx.h"
#include "fill_common.h"
#include <algorithm>
#include <cmath>

namespace {
typedef unsigned long long u64;
constexpr int FL_BLOCKS = 16384;                                                      // of four waves each; the waves stride over the blocks
constexpr u64 FL_MAX_BLOCKS = 1ull << 26, FL_MAX_SEGS = 1ull << 26;
constexpr unsigned FL_BAD_PLACE = 1, FL_BAD_PAIR = 2;
struct FlCounters { u64 lines, samples, on, nshort, segments; unsigned bad; };
struct FlFam { int ux, uy, xmajor, A, B, NW; long long D, kmin, L, row0; u64 wbase; };   // row0: the family's first row
struct FlGrid { FlFam fam[2]; int nf; FlInk ink; u64 Z; };

// the minor coordinate of line k at a; true when the sample exists
__host__ __device__ __forceinline__ bool fl_sample(const FlFam& f, long long k, long long a, long long& b) {
    long long N = f.xmajor ? k * f.D + (long long)f.uy * a : (long long)f.ux * a - k * f.D, d = f.xmajor ? f.ux : f.uy;
    if (d < 0) { N = -N; d = -d; }
    b = fl_floordiv(2 * N + d, 2 * d);
    return b >= 0 && b < f.B;
}
// block z: its family, its line's number in the family and its place in the row
__device__ __forceinline__ const FlFam& fl_block(const FlGrid& g, u64 z, long long& li, int& j) {
    const FlFam& f = g.fam[g.nf == 2 && z >= g.fam[1].wbase ? 1 : 0];
    li = (long long)((z - f.wbase) / (u64)f.NW); j = (int)((z - f.wbase) % (u64)f.NW);
    return f;
}
// the run starts and run ends among the ON bits of block z, the j-th of its row
__device__ __forceinline__ void fl_edges(const u64* __restrict__ on, u64 z, int j, int NW, u64& starts, u64& ends) {
    const u64 w = on[z], carry = j > 0 ? on[z - 1] >> 63 : 0, next = j < NW - 1 ? on[z + 1] & 1 : 0;
    starts = w & ~((w << 1) | carry); ends = w & ~((w >> 1) | (next << 63));
}

// ------------------------------------------------------------------------------------------------ 1. the ON bits
__global__ __launch_bounds__(256) void k_fl_sample(FlGrid g, u64* __restrict__ on, FlCounters* cn) {
    const int lane = threadIdx.x & 63;
    u64 n_lines = 0, n_samples = 0, n_on = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) on[g.Z] = 0;
    for (u64 z = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); z < g.Z; z += (u64)gridDim.x * 4) {      // z is the same in the whole wave
        long long li; int j;
        const FlFam& f = fl_block(g, z, li, j);
        const long long k = f.kmin + li, a = (long long)j * 64 + lane;
        long long b = 0;
        const bool ex = a < f.A && fl_sample(f, k, a, b);
        const bool ink = ex && (f.xmajor ? fl_ink(g.ink, a, b) : fl_ink(g.ink, b, a));
        const u64 me = __ballot(ex), mo = __ballot(ink);
        long long bp;
        const bool before = j > 0 && fl_sample(f, k, (long long)j * 64 - 1, bp);         // the sample in front of the block
        n_lines += (u64)__popcll(me & ~((me << 1) | (before ? 1ull : 0ull)));
        n_samples += (u64)__popcll(me); n_on += (u64)__popcll(mo);
        if (lane == 0) on[z] = mo;
    }
    if (lane == 0 && n_samples) { atomicAdd(&cn->lines, n_lines); atomicAdd(&cn->samples, n_samples); atomicAdd(&cn->on, n_on); }
}

// ------------------------------------------------------------------------------------------------ 2. runs per block
__global__ __launch_bounds__(256) void k_fl_count(FlGrid g, const u64* __restrict__ on, u64* __restrict__ cs) {
    const u64 z = (u64)blockIdx.x * 256 + threadIdx.x;
    if (z > g.Z) return;
    if (z == g.Z) { cs[z] = 0; return; }
    long long li; int j;
    const FlFam& f = fl_block(g, z, li, j);
    u64 starts, ends;
    fl_edges(on, z, j, f.NW, starts, ends);
    cs[z] = ((u64)__popcll(starts) << 32) | (u64)__popcll(ends);
}

// ------------------------------------------------------------------------------------------------ 3. the runs' ends, by rank
__global__ __launch_bounds__(256) void k_fl_scatter(FlGrid g, const u64* __restrict__ on, const u64* __restrict__ sc, u64 R, int* __restrict__ a0, int* __restrict__ a1,
                                                    int* __restrict__ row, FlCounters* cn) {
    const int lane = threadIdx.x & 63;
    const u64 below = (1ull << lane) - 1;
    for (u64 z = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); z < g.Z; z += (u64)gridDim.x * 4) {
        if (!on[z]) continue;
        long long li; int j;
        const FlFam& f = fl_block(g, z, li, j);
        u64 starts, ends;
        fl_edges(on, z, j, f.NW, starts, ends);
        const u64 base = sc[z];
        if ((starts >> lane) & 1) {
            const u64 r = (base >> 32) + (u64)__popcll(starts & below);
            if (r < R) { a0[r] = j * 64 + lane; row[r] = (int)(f.row0 + li); } else atomicOr(&cn->bad, FL_BAD_PAIR);
        }
        if ((ends >> lane) & 1) {
            const u64 r = (base & 0xffffffffull) + (u64)__popcll(ends & below);
            if (r < R) a1[r] = j * 64 + lane; else atomicOr(&cn->bad, FL_BAD_PAIR);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 4. the runs that are drawn
__global__ __launch_bounds__(256) void k_fl_keep(u64 R, const int* __restrict__ a0, const int* __restrict__ a1, int im, int lm, u64* __restrict__ keep, FlCounters* cn) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool run = r < R;
    const bool kp = run && ((long long)a1[r] - im) - ((long long)a0[r] + im) >= lm;
    if (r <= R) keep[r] = kp ? 1 : 0;
    if (run && a1[r] < a0[r]) atomicOr(&cn->bad, FL_BAD_PAIR);
    const u64 mk = __ballot(kp), mr = __ballot(run);
    if ((threadIdx.x & 63) == 0 && mr) { atomicAdd(&cn->segments, (u64)__popcll(mk)); atomicAdd(&cn->nshort, (u64)__popcll(mr & ~mk)); }
}

// ------------------------------------------------------------------------------------------------ 5. emit
__global__ __launch_bounds__(256) void k_fl_emit(FlGrid g, u64 R, u64 S, const u64* __restrict__ sc, const int* __restrict__ a0, const int* __restrict__ a1, const int* __restrict__ row,
                                                 const u64* __restrict__ keep, const u64* __restrict__ kbase, int im, int serpentine, int4* __restrict__ seg, int* __restrict__ segrow, FlCounters* cn) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= R || !keep[r]) return;
    const FlFam& f = g.fam[g.nf == 2 && row[r] >= g.fam[1].row0 ? 1 : 0];
    const long long li = row[r] - f.row0, k = f.kmin + li, s0 = (long long)a0[r] + im, s1 = (long long)a1[r] - im;
    const bool back = serpentine && (k & 1);
    u64 at = kbase[r];
    if (back) {                                                                       // from the row's other end: its runs are [r0, r1)
        const u64 z0 = f.wbase + (u64)li * (u64)f.NW, r0 = sc[z0] >> 32, r1 = sc[z0 + (u64)f.NW] >> 32;
        at = kbase[r0] + kbase[r1] - 1 - at;
    }
    long long b0, b1;
    if (!fl_sample(f, k, s0, b0) || !fl_sample(f, k, s1, b1) || at >= S) { atomicOr(&cn->bad, FL_BAD_PLACE); return; }
    const int4 fw = f.xmajor ? make_int4((int)s0, (int)b0, (int)s1, (int)b1) : make_int4((int)b0, (int)s0, (int)b1, (int)s1);
    seg[at] = back ? make_int4(fw.z, fw.w, fw.x, fw.y) : fw;
    segrow[at] = row[r];
}
// what orip_fill_link needs of the rows: the first segment of every row, rfirst[rows] = S.  Row q's runs start at sc[its first block] >> 32 and its segments at
// kbase of that run, whichever way the row is drawn: serpentine only reverses inside a row
__global__ __launch_bounds__(256) void k_fl_rowfirst(FlGrid g, long long rows, u64 R, u64 S, const u64* __restrict__ sc, const u64* __restrict__ kbase, unsigned* __restrict__ rfirst,
                                                     FlCounters* cn) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q > rows) return;
    u64 z0 = g.Z;
    if (q < rows) { const FlFam& f = g.fam[g.nf == 2 && q >= g.fam[1].row0 ? 1 : 0]; z0 = f.wbase + (u64)(q - f.row0) * (u64)f.NW; }
    const u64 r0 = sc[z0] >> 32;
    if (r0 > R || kbase[r0] > S) { atomicOr(&cn->bad, FL_BAD_PLACE); rfirst[q] = (unsigned)S; return; }
    rfirst[q] = (unsigned)kbase[r0];
}

long long fl_rs(u64 v) {                                                                  // the nearest integer to sqrt(v), v < 2^60
    u64 s = (u64)std::sqrt((long double)(4 * v));
    while (s * s > 4 * v) s--;
    while ((s + 1) * (s + 1) <= 4 * v) s++;
    return (long long)((s + 1) >> 1);
}
}  // namespace

// include/orip.h states the rule; the segments wait in c->fl_out for the fetch
extern "C" int orip_fill_mask(orip_ctx* c, const uint8_t* mask, int layer, int h, int w, int W, int H, int32_t num, int32_t den, int32_t dx, int32_t dy, int32_t ux, int32_t uy,
                              int32_t spacing, int32_t inset, int32_t min_len, int32_t flags, int64_t* stats) {
    orip_enter(c);
    constexpr int TOP = ORIP_FILL_COORD_MAX;
    if (!stats) ORIP_FAIL(c, "bad arguments");
    if (flags & ~(ORIP_FILL_SERPENTINE | ORIP_FILL_ALONG | ORIP_FILL_ACROSS)) ORIP_FAIL(c, "unknown flags %d", flags);
    if (!(flags & (ORIP_FILL_ALONG | ORIP_FILL_ACROSS))) ORIP_FAIL(c, "flags %d: ORIP_FILL_ALONG, ORIP_FILL_ACROSS or both", flags);
    if (h < 1 || w < 1 || h > TOP || w > TOP || (long long)h * w >= (1ll << 31)) ORIP_FAIL(c, "mask %d x %d: each side in 1..2^20, fewer than 2^31 pixels", w, h);
    if (W < 1 || H < 1 || W > TOP || H > TOP) ORIP_FAIL(c, "canvas %d x %d: each side in 1..2^20", W, H);
    if (num < 1 || num > TOP || den < 1 || den > TOP) ORIP_FAIL(c, "placement scale %d / %d: both in 1..2^20", num, den);
    if (dx < -TOP || dx > TOP || dy < -TOP || dy > TOP) ORIP_FAIL(c, "placement offset (%d, %d): both in -2^20..2^20", dx, dy);
    if ((ux == 0 && uy == 0) || ux < -ORIP_FILL_U_MAX || ux > ORIP_FILL_U_MAX || uy < -ORIP_FILL_U_MAX || uy > ORIP_FILL_U_MAX)
        ORIP_FAIL(c, "direction (%d, %d): not zero, max(|ux|, |uy|) <= 4096", ux, uy);
    if (spacing < 2 || spacing > ORIP_FILL_LEN_MAX) ORIP_FAIL(c, "spacing %d: 2..2^15", spacing);
    if (inset < 0 || inset > ORIP_FILL_LEN_MAX) ORIP_FAIL(c, "inset %d: 0..2^15", inset);
    if (min_len < 1 || min_len > ORIP_FILL_LEN_MAX) ORIP_FAIL(c, "min_len %d: 1..2^15", min_len);
    if (!mask) {
        if (!c->masks.p || layer < 0 || layer >= c->K) ORIP_FAIL(c, "no mask resident for layer %d", layer);
        if (h != c->H || w != c->W) ORIP_FAIL(c, "mask %d x %d given, the resident masks are %d x %d", w, h, c->W, c->H);
    }
    // the families: their lines and blocks
    const long long U2 = (long long)ux * ux + (long long)uy * uy, Rr = fl_rs((u64)U2), D = fl_rs((u64)spacing * (u64)spacing * (u64)U2), m = std::max(std::abs(ux), std::abs(uy));
    const int im = (int)((2ll * inset * m + Rr) / (2 * Rr)), lm = (int)std::max(1ll, (2ll * min_len * m + Rr) / (2 * Rr));
    FlGrid g{};
    g.ink = FlInk{nullptr, h, w, num, den, dx, dy};
    long long rows = 0;
    for (int pass = 0; pass < 2; pass++) {
        if (!(flags & (pass ? ORIP_FILL_ACROSS : ORIP_FILL_ALONG))) continue;
        FlFam& f = g.fam[g.nf];
        f.ux = pass ? -uy : ux; f.uy = pass ? ux : uy;
        f.xmajor = std::abs(f.ux) >= std::abs(f.uy) ? 1 : 0;
        f.A = f.xmajor ? W : H; f.B = f.xmajor ? H : W; f.NW = (f.A + 63) / 64; f.D = D;
        const long long cx = -(long long)f.uy * (W - 1), cy = (long long)f.ux * (H - 1);      // n.p at the corners: 0, cx, cy, cx + cy
        const long long lo = std::min(0ll, cx) + std::min(0ll, cy), hi = std::max(0ll, cx) + std::max(0ll, cy);
        f.kmin = -fl_floordiv(-(lo - m), D);
        f.L = std::max(0ll, fl_floordiv(hi + m, D) - f.kmin + 1);
        f.row0 = rows; f.wbase = g.Z;
        rows += f.L; g.Z += (u64)f.L * (u64)f.NW;
        if (f.L) g.nf++;                                                              // a family without a line takes no part
    }
    if (g.Z >= FL_MAX_BLOCKS) ORIP_FAIL(c, "%llu blocks of 64 samples over %lld lines: fewer than 2^26", g.Z, rows);

    for (int k = 0; k < ORIP_FILL_STATS; k++) stats[k] = 0;
    c->fk_paths = -1;                                                         // a link result belongs to the list this call replaces
    if (g.Z == 0) { c->fl_segs = 0; return 0; }                                  // nothing to launch: the list of no segments
    c->fl_segs = -1;                                                          // no segment list from here to the last read-back
    hipStream_t s = LN(c).stream;
    const size_t Z = (size_t)g.Z;
    u8* d_mask; u64 *on, *cs, *sc; FlCounters* cn;
    { Carve L; L.take(d_mask, mask ? (size_t)h * w : 0); L.take(on, Z + 1); L.take(cs, Z + 1); L.take(sc, Z + 1); L.take(cn, 1); HIPC(c, L.commit(c->fl_tmp, 64)); }
    if (mask) HIPC(c, hipMemcpyAsync(d_mask, mask, (size_t)h * w, hipMemcpyHostToDevice, s));
    g.ink.M = mask ? d_mask : c->masks.as<u8>() + (size_t)h * w * (size_t)layer;
    HIPC(c, hipMemsetAsync(cn, 0, sizeof(FlCounters), s));
    const dim3 b(256), gw((unsigned)std::min<u64>((g.Z + 3) / 4, FL_BLOCKS));
    { ProfScope ps(c, "fl_sample");
      hipLaunchKernelGGL(k_fl_sample, gw, b, 0, s, g, on, cn); }
    { ProfScope ps(c, "fl_count");
      hipLaunchKernelGGL(k_fl_count, dim3(cdiv((int64_t)Z + 1, 256)), b, 0, s, g, on, cs);
      HIPC(c, gc_scan_u64(c, cs, sc, Z + 1)); }
    HIPC(c, hipGetLastError());
    u64 tot = 0;
    FlCounters hc;
    HIPC(c, hipMemcpyAsync(&tot, sc + Z, 8, hipMemcpyDeviceToHost, s));              // first read-back: the runs
    HIPC(c, hipMemcpyAsync(&hc, cn, sizeof(FlCounters), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    const u64 R = tot >> 32;
    if (R != (tot & 0xffffffffull)) ORIP_FAIL(c, "the runs do not add up (%llu starts, %llu ends)", R, tot & 0xffffffffull);
    u64 S = 0;
    if (R) {
        int *a0, *a1, *row; u64 *keep, *kbase;
        { Carve L; L.each((size_t)R, a0, a1, row); L.each((size_t)R + 1, keep, kbase); HIPC(c, L.commit(c->fl_runs, 64)); }
        { ProfScope ps(c, "fl_runs");
          hipLaunchKernelGGL(k_fl_scatter, gw, b, 0, s, g, on, sc, R, a0, a1, row, cn);
          hipLaunchKernelGGL(k_fl_keep, dim3(cdiv((int64_t)R + 1, 256)), b, 0, s, R, a0, a1, im, lm, keep, cn);
          HIPC(c, gc_scan_u64(c, keep, kbase, (size_t)R + 1)); }
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(&S, kbase + R, 8, hipMemcpyDeviceToHost, s));          // second read-back: the segments
        HIPC(c, hipStreamSynchronize(s));
        if (S >= FL_MAX_SEGS) ORIP_FAIL(c, "%llu segments: fewer than 2^26", S);
        int4* seg; int* segrow; unsigned* rfirst;
        { Carve L; L.take(seg, (size_t)S); HIPC(c, L.commit(c->fl_out, 64)); }
        { Carve L; L.take(segrow, (size_t)S); L.take(rfirst, (size_t)rows + 1); HIPC(c, L.commit(c->fl_rows, 64)); }
        if (S) { ProfScope ps(c, "fl_emit");
          hipLaunchKernelGGL(k_fl_emit, dim3(cdiv((int64_t)R, 256)), b, 0, s, g, R, S, sc, a0, a1, row, keep, kbase, im, (flags & ORIP_FILL_SERPENTINE) ? 1 : 0, seg, segrow, cn);
          hipLaunchKernelGGL(k_fl_rowfirst, dim3(cdiv(rows + 1, 256)), b, 0, s, g, rows, R, S, sc, kbase, rfirst, cn); }
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(&hc, cn, sizeof(FlCounters), hipMemcpyDeviceToHost, s));      // third read-back: the counters
        HIPC(c, hipStreamSynchronize(s));
    }
    if (hc.bad || hc.segments != S || hc.nshort + hc.segments != R) ORIP_FAIL(c, "the segments do not add up (internal error %u)", hc.bad);
    c->fl_segs = (int64_t)S;
    c->fl_nrows = rows; c->fl_row1 = g.nf == 2 ? g.fam[1].row0 : rows;
    for (int k = 0; k < 2; k++) c->fl_xmajor[k] = g.fam[k].xmajor;
    stats[0] = (int64_t)hc.lines; stats[1] = (int64_t)hc.samples; stats[2] = (int64_t)hc.on; stats[3] = (int64_t)R; stats[4] = (int64_t)hc.nshort; stats[5] = (int64_t)hc.segments;
    return 0;
}

extern "C" int orip_fill_fetch(orip_ctx* c, int32_t* seg) {
    orip_enter(c);
    if (c->fl_segs < 0) ORIP_FAIL(c, "no result: the fill has not succeeded since the last failure");
    if (c->fl_segs == 0) return 0;
    if (!seg) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(seg, c->fl_out.p, (size_t)c->fl_segs * 16, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
