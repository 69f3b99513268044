// csrc/fill_link.hip -- fill connect of the raster pipeline: the hatch segments of a mask are drawn as zigzags, every link kept on the mask's ink
// (orip_fill_link, orip_fill_link_fetch; the rule is stated in include/orip.h, is exact in integers and has one answer for every input).  Ours: the
// reference has no such pass.
//
// The input is the resident segment list of orip_fill_mask (c->fl_out) with what the fill keeps for this pass (orip_ctx.h: c->fl_rows): the ROW of every
// segment and the first segment of every row.  A link only runs onto the next line of its own family, so the candidates of an END on row q are exactly the
// segments of row q + 1 (none when q + 1 is the first row of the other family), and inside a row the STARTs are strictly monotone in the family's major
// coordinate -- ascending, or descending where serpentine has turned the row -- so the window |major(START) - major(END)| <= reach is one binary search.
//
// 1. Pairs in reach.  fk_probe, one thread per END: the window of row q + 1, each START tested for max(|dx|, |dy|) <= reach and dx^2 + dy^2 <= reach^2 in
//    64-bit.  k_fk_count counts, a scan (gc_cut.h: gc_scan_u64) places, the host reads the total P (the one sizing read-back; 2^28 pairs or more is
//    refused); k_fk_list runs the same probe again and writes (a, b).
// 2. k_fk_elig, one WAVE per pair: the link's n + 1 pixels 64 at a time, a pixel a lane; every lane takes its pixel's INK as the fill's samples do (two floor
//    divisions into the mask's grid and one byte of the mask), a ballot decides, and the first block of 64 with a hole ends the walk.  Lane 0 of an
//    eligible pair takes two atomicMin of (d^2 << 32 | partner), best-out of a and best-in of b: d^2 <= 2^30 and an index is below 2^26, so the pair of
//    them is ONE word and one minimum, and no order of the waves shows.  The waves stride over the pairs under FK_BLOCKS.
// 3. k_fk_mutual, one thread per END: a -> b is a link iff each is the other's best; next / prev, links and link_steps.
// 4. Chains.  Links ascend by one row, so a chain is open, its head is its lowest member and it has at most as many members as a family has rows.  Heads by
//    pointer jumping over prev, head'[j] = head[head[j]], ping-pong between two arrays, `rounds` fixed on the host with 2^rounds >= the rows, no read-back in
//    between; a head that still has a prev afterwards is an internal error.  A member's RANK in its chain is its row minus its head's row: every link
//    advances exactly one row, so nothing has to be summed along the chain.  The tail (no next) hands the chain's size to its head.
// 5. Emit.  cs[j] = (2 members << 32 | 1) at a head, 0 elsewhere: one scan of the packed word places the points and numbers the strokes, as the cutting
//    passes scan theirs.  k_fk_emit, one thread per segment: its two points at the head's base + 2 rank, and a head its stroke's offset.
// Everything on the stream the fill uses (the raster stages' one); the second read-back fetches the totals and the counters behind the last launch.  Every
// index computed from device data is checked against its array before it is used; a miss sets FkCounters::bad and fails the call.
//
// Scratch, free between calls (orip_ctx.h states the buffers).  c->fk_tmp, ONE Carve, S segments: mask u8[h w] (explicit form only); cnt u64[S + 1]; base
// u64[S + 1]; best u64[2 S] (per END, per START); link int[2 S] (next, prev); head int[2 S] (the two arrays of the jumping); len int[S]; cs u64[S + 1]; sc
// u64[S + 1]; FkCounters.  c->fk_pair, behind the first read-back: pairs uint2[P].  Resident until the next call: c->fk_out = off long long[S + 1], pts
// int2[2 S].
#include "orip_ctx.h"
#include "fill_common.h"
#include <algorithm>

namespace {
typedef unsigned long long u64;
constexpr int FK_BLOCKS = 2048;                                                       // of four waves each; the waves stride over the pairs
constexpr u64 FK_MAX_PAIRS = 1ull << 28;
constexpr unsigned FK_BAD_LIST = 1, FK_BAD_CHAIN = 2, FK_BAD_PLACE = 4;
struct FkCounters { u64 eligible, links, link_steps; unsigned bad; };
// the segments and their rows, as the fill left them
struct FkRows { const int4* seg; const int* segrow; const unsigned* rfirst; long long S, nrows, row1; int xmajor[2]; long long reach; };

// found(b) for every segment b on the line after a's whose START is in reach of a's END: each once, in a fixed order
template <class F> __device__ __forceinline__ void fk_probe(const FkRows& L, long long a, F&& found) {
    const long long q = L.segrow[a];
    if (q < 0 || q + 1 >= L.nrows || q + 1 == L.row1) return;                        // the last line of its family has no next one
    const long long f0 = L.rfirst[q + 1], f1 = L.rfirst[q + 2];
    if (f0 >= f1 || f1 > L.S) return;
    const int xm = L.xmajor[q >= L.row1 ? 1 : 0];
    const int4 me = L.seg[a];
    const long long em = xm ? me.z : me.w, cnt = f1 - f0;
    auto start_major = [&](long long i) { const int4 o = L.seg[i]; return (long long)(xm ? o.x : o.y); };
    const bool asc = start_major(f0) <= start_major(f1 - 1);                          // i-th START in ascending major order: f0 + i, or f1 - 1 - i
    long long lo = 0, hi = cnt;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (start_major(asc ? f0 + mid : f1 - 1 - mid) < em - L.reach) lo = mid + 1; else hi = mid; }
    for (long long i = lo; i < cnt; i++) {
        const long long b = asc ? f0 + i : f1 - 1 - i;
        const int4 o = L.seg[b];
        if ((long long)(xm ? o.x : o.y) > em + L.reach) break;
        const long long dx = (long long)o.x - me.z, dy = (long long)o.y - me.w;
        if (dx > L.reach || dx < -L.reach || dy > L.reach || dy < -L.reach || dx * dx + dy * dy > L.reach * L.reach) continue;
        found(b);
    }
}

// ------------------------------------------------------------------------------------------------ 1. pairs in reach
__global__ __launch_bounds__(256) void k_fk_count(FkRows L, u64* __restrict__ cnt) {
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    if (a > L.S) return;
    u64 k = 0;
    if (a < L.S) fk_probe(L, a, [&](long long) { k++; });
    cnt[a] = k;
}
__global__ __launch_bounds__(256) void k_fk_list(FkRows L, const u64* __restrict__ cnt, const u64* __restrict__ base, u64 P, uint2* __restrict__ pairs, FkCounters* cn) {
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    if (a >= L.S) return;
    const u64 at = base[a], k1 = cnt[a];
    if (at > P || k1 > P - at) { atomicOr(&cn->bad, FK_BAD_LIST); return; }
    u64 k = 0;
    fk_probe(L, a, [&](long long b) { if (k < k1) pairs[at + k] = make_uint2((unsigned)a, (unsigned)b); k++; });
    if (k != k1) atomicOr(&cn->bad, FK_BAD_LIST);
}

// ------------------------------------------------------------------------------------------------ 2. eligibility, and the best partner per END and per START
__global__ __launch_bounds__(256) void k_fk_elig(u64 P, const uint2* __restrict__ pairs, long long S, const int4* __restrict__ seg, FlInk g, u64* best, FkCounters* cn) {
    const int lane = threadIdx.x & 63;
    for (u64 q = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); q < P; q += (u64)gridDim.x * 4) {     // q, and with it the pair, is the same in the whole wave
        const uint2 pr = pairs[q];
        if (pr.x >= (u64)S || pr.y >= (u64)S) { if (lane == 0) atomicOr(&cn->bad, FK_BAD_LIST); continue; }
        const int4 la = seg[pr.x], lb = seg[pr.y];
        const long long dx = (long long)lb.x - la.z, dy = (long long)lb.y - la.w, ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, n = ax > ay ? ax : ay;
        const bool xm = ax >= ay;
        const long long dmaj = xm ? dx : dy, dmin = xm ? dy : dx, sgn = dmaj < 0 ? -1 : 1;
        bool hole = false;
        for (long long t0 = 0; t0 <= n; t0 += 64) {
            const long long t = t0 + lane;
            if (t <= n) {
                const long long mj = (xm ? la.z : la.w) + sgn * t, mn = (xm ? la.w : la.z) + (n > 0 ? fl_floordiv(2 * t * dmin + n, 2 * n) : 0);
                hole = !(xm ? fl_ink(g, mj, mn) : fl_ink(g, mn, mj));
            }
            if (__ballot(hole)) break;                                                // no lane goes on once a block of 64 has a hole
        }
        if (__ballot(hole) == 0 && lane == 0) {
            const u64 d2 = (u64)(dx * dx + dy * dy);                                  // in reach: at most 2^30
            atomicMin(&best[pr.x], (d2 << 32) | pr.y);
            atomicMin(&best[(size_t)S + pr.y], (d2 << 32) | pr.x);
            atomicAdd(&cn->eligible, 1ull);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 3. mutual
__global__ __launch_bounds__(256) void k_fk_mutual(long long S, const int4* __restrict__ seg, const u64* __restrict__ best, int* __restrict__ link, FkCounters* cn) {
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    if (a >= S) return;
    const u64 out = best[a];
    if (out == ~0ull) return;
    const u64 b = out & 0xffffffffull;
    if (b >= (u64)S || (long long)b <= a) { atomicOr(&cn->bad, FK_BAD_LIST); return; }
    if (best[(size_t)S + b] != ((out & ~0xffffffffull) | (u64)a)) return;
    link[a] = (int)b; link[(size_t)S + b] = (int)a;                                   // next, prev: only a is b's best, so nobody else writes prev[b]
    const int4 la = seg[a], lb = seg[b];
    const long long dx = (long long)lb.x - la.z, dy = (long long)lb.y - la.w, x = dx < 0 ? -dx : dx, y = dy < 0 ? -dy : dy;
    atomicAdd(&cn->links, 1ull); atomicAdd(&cn->link_steps, (u64)(x > y ? x : y));
}

// ------------------------------------------------------------------------------------------------ 4. chains
__global__ __launch_bounds__(256) void k_fk_chain0(long long S, const int* __restrict__ link, const int* __restrict__ segrow, int* __restrict__ head, FkCounters* cn) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    int p = link[(size_t)S + j];
    if (p >= 0 && (p >= j || segrow[p] + 1 != segrow[j])) { atomicOr(&cn->bad, FK_BAD_CHAIN); p = -1; }      // a link advances one row
    head[j] = p >= 0 ? p : (int)j;
}
__global__ __launch_bounds__(256) void k_fk_jump(const int* __restrict__ A, int* __restrict__ B, long long S) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    const int h = A[j];
    B[j] = (unsigned)h < (u64)S ? A[h] : (int)j;
}
__global__ __launch_bounds__(256) void k_fk_heads(long long S, const int* __restrict__ link, const int* __restrict__ segrow, const int* __restrict__ head, int* __restrict__ len,
                                                  FkCounters* cn) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    const int h = head[j];
    if ((unsigned)h >= (u64)S || link[(size_t)S + h] >= 0 || segrow[j] < segrow[h]) { atomicOr(&cn->bad, FK_BAD_CHAIN); return; }
    if (link[j] < 0) len[h] = segrow[j] - segrow[h] + 1;                             // one tail per chain
}

// ------------------------------------------------------------------------------------------------ 5. emit
__global__ __launch_bounds__(256) void k_fk_sizes(long long S, const int* __restrict__ link, const int* __restrict__ len, u64* __restrict__ cs, FkCounters* cn) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j > S) return;
    u64 v = 0;
    if (j < S && link[(size_t)S + j] < 0) {
        if (len[j] < 1) atomicOr(&cn->bad, FK_BAD_CHAIN); else v = ((u64)(2 * (unsigned)len[j]) << 32) | 1ull;
    }
    cs[j] = v;
}
__global__ __launch_bounds__(256) void k_fk_emit(long long S, const int4* __restrict__ seg, const int* __restrict__ segrow, const int* __restrict__ link, const int* __restrict__ head,
                                                 const u64* __restrict__ sc, long long* __restrict__ off, int2* __restrict__ pts, FkCounters* cn) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j > S) return;
    if (j == S) {                                                                     // the closing offset
        if ((sc[S] & 0xffffffffull) <= (u64)S) off[sc[S] & 0xffffffffull] = (long long)(sc[S] >> 32); else atomicOr(&cn->bad, FK_BAD_PLACE);
        return;
    }
    const int h = head[j];
    if ((unsigned)h >= (u64)S) return;                                                // said by k_fk_heads
    const long long at = (long long)(sc[h] >> 32) + 2ll * ((long long)segrow[j] - segrow[h]), sid = (long long)(sc[h] & 0xffffffffull);
    if (at < 0 || at + 2 > 2 * S || sid >= S) { atomicOr(&cn->bad, FK_BAD_PLACE); return; }
    const int4 me = seg[j];
    pts[at] = make_int2(me.x, me.y); pts[at + 1] = make_int2(me.z, me.w);
    if (link[(size_t)S + j] < 0) off[sid] = at;
}
}  // namespace

// include/orip.h states the rule; the strokes wait in c->fk_out for the fetch
extern "C" int orip_fill_link(orip_ctx* c, const uint8_t* mask, int layer, int h, int w, int32_t num, int32_t den, int32_t dx, int32_t dy, int32_t reach, int64_t* stats) {
    orip_enter(c);
    constexpr int TOP = ORIP_FILL_COORD_MAX;
    if (!stats) ORIP_FAIL(c, "bad arguments");
    if (c->fl_segs < 0) ORIP_FAIL(c, "no segments: orip_fill_mask has not succeeded since the last failure");
    if (h < 1 || w < 1 || h > TOP || w > TOP || (long long)h * w >= (1ll << 31)) ORIP_FAIL(c, "mask %d x %d: each side in 1..2^20, fewer than 2^31 pixels", w, h);
    if (num < 1 || num > TOP || den < 1 || den > TOP) ORIP_FAIL(c, "placement scale %d / %d: both in 1..2^20", num, den);
    if (dx < -TOP || dx > TOP || dy < -TOP || dy > TOP) ORIP_FAIL(c, "placement offset (%d, %d): both in -2^20..2^20", dx, dy);
    if (reach < 1 || reach > ORIP_FILL_LINK_REACH_MAX) ORIP_FAIL(c, "reach %d: 1..2^15", reach);
    if (!mask) {
        if (!c->masks.p || layer < 0 || layer >= c->K) ORIP_FAIL(c, "no mask resident for layer %d", layer);
        if (h != c->H || w != c->W) ORIP_FAIL(c, "mask %d x %d given, the resident masks are %d x %d", w, h, c->W, c->H);
    }
    for (int k = 0; k < ORIP_FILL_LINK_STATS; k++) stats[k] = 0;
    const long long S = c->fl_segs;
    if (S == 0) { c->fk_paths = 0; c->fk_segs = 0; return 0; }                  // nothing to launch: the list of no strokes
    c->fk_paths = -1;                                                         // no link result from here to the last read-back
    hipStream_t s = LN(c).stream;
    const size_t Z = (size_t)S;
    u8* d_mask; u64 *cnt, *base, *best, *cs, *sc; int *link, *head, *len; FkCounters* cn;
    { Carve L; L.take(d_mask, mask ? (size_t)h * w : 0); L.take(cnt, Z + 1); L.take(base, Z + 1); L.take(best, 2 * Z); L.take(link, 2 * Z); L.take(head, 2 * Z); L.take(len, Z);
      L.take(cs, Z + 1); L.take(sc, Z + 1); L.take(cn, 1); HIPC(c, L.commit(c->fk_tmp, 64)); }
    long long* off; int2* pts;
    { Carve L; L.take(off, Z + 1); L.take(pts, 2 * Z); HIPC(c, L.commit(c->fk_out, 64)); }
    if (mask) HIPC(c, hipMemcpyAsync(d_mask, mask, (size_t)h * w, hipMemcpyHostToDevice, s));
    const FlInk g = {mask ? d_mask : c->masks.as<u8>() + (size_t)h * w * (size_t)layer, h, w, num, den, dx, dy};
    const int4* seg = c->fl_out.as<int4>();
    int* segrow; unsigned* rfirst;                                                    // the layout the fill carved; the buffer already holds it, so nothing grows
    { Carve Lr; Lr.take(segrow, Z); Lr.take(rfirst, (size_t)c->fl_nrows + 1); HIPC(c, Lr.commit(c->fl_rows, 64)); }
    const FkRows L = {seg, segrow, rfirst, S, c->fl_nrows, c->fl_row1, {c->fl_xmajor[0], c->fl_xmajor[1]}, reach};
    HIPC(c, hipMemsetAsync(cn, 0, sizeof(FkCounters), s));
    HIPC(c, hipMemsetAsync(best, 0xFF, 2 * Z * 8, s));
    HIPC(c, hipMemsetAsync(link, 0xFF, 2 * Z * 4, s));
    HIPC(c, hipMemsetAsync(len, 0, Z * 4, s));
    const dim3 b(256), gs(cdiv(S, 256)), gs1(cdiv(S + 1, 256));
    { ProfScope ps(c, "fk_count");
      hipLaunchKernelGGL(k_fk_count, gs1, b, 0, s, L, cnt);
      HIPC(c, gc_scan_u64(c, cnt, base, Z + 1)); }
    HIPC(c, hipGetLastError());
    u64 P = 0;
    HIPC(c, hipMemcpyAsync(&P, base + Z, 8, hipMemcpyDeviceToHost, s));              // first read-back: the pairs in reach
    HIPC(c, hipStreamSynchronize(s));
    if (P >= FK_MAX_PAIRS) ORIP_FAIL(c, "%llu pairs in reach: fewer than 2^28", P);
    if (P) {
        uint2* pairs;
        { Carve Lp; Lp.take(pairs, (size_t)P); HIPC(c, Lp.commit(c->fk_pair, 64)); }
        hipLaunchKernelGGL(k_fk_list, gs, b, 0, s, L, cnt, base, P, pairs, cn);
        { ProfScope ps(c, "fk_elig");
          hipLaunchKernelGGL(k_fk_elig, dim3((unsigned)std::min<u64>((P + 3) / 4, FK_BLOCKS)), b, 0, s, P, pairs, S, seg, g, best, cn); }
        hipLaunchKernelGGL(k_fk_mutual, gs, b, 0, s, S, seg, best, link, cn);
    }
    int rounds = 0; while ((1ll << rounds) < c->fl_nrows) rounds++;                   // a chain has a member per row at the most
    int *src = head, *dst = head + Z;
    { ProfScope ps(c, "fk_chain");
      hipLaunchKernelGGL(k_fk_chain0, gs, b, 0, s, S, link, segrow, src, cn);
      for (int r = 0; r < rounds; r++) { hipLaunchKernelGGL(k_fk_jump, gs, b, 0, s, src, dst, S); std::swap(src, dst); }
      hipLaunchKernelGGL(k_fk_heads, gs, b, 0, s, S, link, segrow, src, len, cn); }
    { ProfScope ps(c, "fk_emit");
      hipLaunchKernelGGL(k_fk_sizes, gs1, b, 0, s, S, link, len, cs, cn);
      HIPC(c, gc_scan_u64(c, cs, sc, Z + 1));
      hipLaunchKernelGGL(k_fk_emit, gs1, b, 0, s, S, seg, segrow, link, src, sc, off, pts, cn); }
    HIPC(c, hipGetLastError());
    struct { u64 tot; FkCounters cn; } hb;                                             // second read-back: the totals and the counters
    HIPC(c, hipMemcpyAsync(&hb.tot, sc + Z, 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&hb.cn, cn, sizeof(FkCounters), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    const long long paths = (long long)(hb.tot & 0xffffffffull), points = (long long)(hb.tot >> 32);
    if (hb.cn.bad || paths != S - (long long)hb.cn.links || points != 2 * S || hb.cn.eligible > P || hb.cn.links > hb.cn.eligible)
        ORIP_FAIL(c, "the chains do not add up (internal error %u)", hb.cn.bad);
    c->fk_paths = paths; c->fk_segs = S;
    stats[0] = S; stats[1] = (int64_t)P; stats[2] = (int64_t)hb.cn.eligible; stats[3] = (int64_t)hb.cn.links; stats[4] = paths; stats[5] = points; stats[6] = (int64_t)hb.cn.link_steps;
    return 0;
}

extern "C" int orip_fill_link_fetch(orip_ctx* c, int64_t* off, int32_t* pts) {
    orip_enter(c);
    if (c->fk_paths < 0) ORIP_FAIL(c, "no result: the fill link has not succeeded since the last failure or the last fill");
    if (!off || (c->fk_segs > 0 && !pts)) ORIP_FAIL(c, "bad arguments");
    if (c->fk_segs == 0) { off[0] = 0; return 0; }
    hipStream_t s = LN(c).stream;
    const size_t Z = (size_t)c->fk_segs;
    long long* r_off; int2* r_pts;                                                    // the layout orip_fill_link carved; the buffer already holds it, so nothing grows
    { Carve L; L.take(r_off, Z + 1); L.take(r_pts, 2 * Z); HIPC(c, L.commit(c->fk_out, 64)); }
    HIPC(c, hipMemcpyAsync(off, r_off, (size_t)(c->fk_paths + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(pts, r_pts, 2 * Z * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
