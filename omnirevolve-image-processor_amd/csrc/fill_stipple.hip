// csrc/fill_stipple.hip -- fill_layers' second fill: a colour mask is filled with DOTS on one lattice for the whole canvas, their density following the
// darkness of the source image inside the mask through an ordered dither (orip_fill_stipple, orip_fill_stipple_fetch; the rule is stated in
// include/orip.h, is exact in integers and has one answer for every input).  Ours: the reference has no such pass.
//
// A ROW is a lattice row j = 0 .. NJ - 1 (Y = j row < H).  A BLOCK is 64 consecutive lattice columns i of one row: the work of one wave, one candidate a
// lane; every row has NW = ceil(NI / 64) blocks, NI the candidates of an even row (an odd row, moved by `shift`, has as many or one fewer: the lanes
// beyond its last candidate do not exist), and block z = j NW + i / 64, so the blocks ascend as the dots leave: j, then X.
//
// 1. k_fs_verdict, one WAVE per block: every lane computes its candidate, whether it exists and whether it is INK (fl_ink: one ballot); then CLEAR (the
//    square of clear_rad around its source pixel is inside the image and set) and, only with a tone image, C and S over the set pixels of the clipped
//    square of tone_rad, and the verdict 64 E > T R C.  A window of at most FS_LANE_WINDOW pixels is walked by the candidate's own lane; a larger one is
//    walked by the WAVE: it visits the set bits of the ballot one after the other, and for each all 64 lanes stride over the window row-major (byte reads
//    of M and G that lie side by side), a ballot finds the first hole of the clearance and ends it there, and C and S are reduced across the wave.  The
//    verdicts of the block are one ballot, dot[z], and its popcount cnt[z]; the five counts are summed per wave and added once.
//    Without a tone image G = 0: then S = 0 and E = min((255 - lo) C, R C) = R C because hi <= 255, so 64 E > T R C holds for every T < 64: every clear
//    candidate is a dot and the tone window is not read at all.
// 2. One scan (gc_cut.h: gc_scan_u64) of cnt places the dots; the host reads their number (first read-back: 2^26 or more is refused).
// 3. k_fs_emit, one wave per block with a dot: a lane whose bit is set writes (X, Y) at sc[z] + its rank in the word; under ORIP_FILL_STIPPLE_SERPENTINE a
//    dot of a row with j & 1 counts from the row's other end (the row's first and last place are sc at its first block and at the next row's): an index
//    computation, not a second pass.
// A launch over the blocks has at most FS_BLOCKS workgroups of four waves; the waves stride over the blocks.  Everything on the raster stages' stream,
// where the resident masks are written.
//
// Scratch (orip_ctx.h states the buffers).  c->fs_tmp, ONE Carve: mask u8[h w] (explicit form only); tone u8[h w] (only with a tone image); dot u64[Z];
// cnt u64[Z + 1]; sc u64[Z + 1]; FsCounters.  Resident until the next call that passes its argument checks: c->fs_out = xy int2[fs_dots].
#include "orip_ctx.h"
#include "fill_common.h"
#include <algorithm>

namespace {
typedef unsigned long long u64;
constexpr int FS_BLOCKS = 4096;                                                       // of four waves each; the waves stride over the blocks
constexpr int FS_LANE_WINDOW = 64;                                                    // a window of more pixels than this is walked by the wave, not by the lane
constexpr u64 FS_MAX_BLOCKS = 1ull << 26, FS_MAX_DOTS = 1ull << 26;
constexpr unsigned FS_BAD_PLACE = 1;
struct FsCounters { u64 candidates, ink, near, light, dots; unsigned bad; };
struct FsGrid { FlInk ink; const u8* G; int W, pitch, row, shift, NW, cr, tr, lo, hi; u64 Z; };

__host__ __device__ __forceinline__ bool fs_by_wave(int rad) { return (2 * rad + 1) * (2 * rad + 1) > FS_LANE_WINDOW; }

// ------------------------------------------------------------------------------------------------ the windows, by one lane
__device__ __forceinline__ bool fs_lane_clear(const FlInk& k, int c, int r, int rad) {
    if (c - rad < 0 || r - rad < 0 || c + rad >= k.w || r + rad >= k.h) return false;                      // the outside of the image is not set
    for (int rr = r - rad; rr <= r + rad; rr++) {
        const u8* line = k.M + (size_t)rr * (size_t)k.w;
        for (int cc = c - rad; cc <= c + rad; cc++) if (!line[cc]) return false;
    }
    return true;
}
__device__ __forceinline__ void fs_lane_tone(const FsGrid& g, int c, int r, int& C, int& S) {
    const int r0 = max(r - g.tr, 0), r1 = min(r + g.tr, g.ink.h - 1), c0 = max(c - g.tr, 0), c1 = min(c + g.tr, g.ink.w - 1);
    C = 0; S = 0;
    for (int rr = r0; rr <= r1; rr++) {
        const size_t at = (size_t)rr * (size_t)g.ink.w;
        for (int cc = c0; cc <= c1; cc++) if (g.ink.M[at + cc]) { C++; S += g.G[at + cc]; }
    }
}
// ------------------------------------------------------------------------------------------------ the windows, by the wave: c and r are the same in all lanes
__device__ __forceinline__ bool fs_wave_clear(const FlInk& k, int c, int r, int rad, int lane) {
    if (c - rad < 0 || r - rad < 0 || c + rad >= k.w || r + rad >= k.h) return false;
    const int side = 2 * rad + 1, n = side * side, dr = 64 / side, dc = 64 % side;
    int wr = lane / side, wc = lane % side;                                           // pixel base + lane of the window, row-major
    for (int base = 0; base < n; base += 64) {
        const bool hole = base + lane < n && !k.M[(size_t)(r - rad + wr) * (size_t)k.w + (size_t)(c - rad + wc)];
        if (__ballot(hole)) return false;                                             // the first hole ends it
        wr += dr; wc += dc;
        if (wc >= side) { wc -= side; wr++; }
    }
    return true;
}
__device__ __forceinline__ void fs_wave_tone(const FsGrid& g, int c, int r, int lane, int& C, int& S) {
    const int r0 = max(r - g.tr, 0), r1 = min(r + g.tr, g.ink.h - 1), c0 = max(c - g.tr, 0), c1 = min(c + g.tr, g.ink.w - 1);
    const int ww = c1 - c0 + 1, n = ww * (r1 - r0 + 1), dr = 64 / ww, dc = 64 % ww;
    int wr = lane / ww, wc = lane % ww, cnt = 0, sum = 0;
    for (int base = 0; base < n; base += 64) {
        if (base + lane < n) {
            const size_t at = (size_t)(r0 + wr) * (size_t)g.ink.w + (size_t)(c0 + wc);
            if (g.ink.M[at]) { cnt++; sum += g.G[at]; }
        }
        wr += dr; wc += dc;
        if (wc >= ww) { wc -= ww; wr++; }
    }
    for (int d = 32; d; d >>= 1) { cnt += __shfl_xor(cnt, d); sum += __shfl_xor(sum, d); }
    C = cnt; S = sum;
}

// ------------------------------------------------------------------------------------------------ 1. the verdicts
__global__ __launch_bounds__(256) void k_fs_verdict(FsGrid g, u64* __restrict__ dot, u64* __restrict__ cnt, FsCounters* cn) {
    const int lane = threadIdx.x & 63;
    const bool wave_clear = fs_by_wave(g.cr), wave_tone = fs_by_wave(g.tr);
    u64 n_cand = 0, n_ink = 0, n_near = 0, n_light = 0, n_dots = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[g.Z] = 0;
    for (u64 z = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); z < g.Z; z += (u64)gridDim.x * 4) {      // z is the same in the whole wave
        const long long j = (long long)(z / (u64)g.NW), i = (long long)(z % (u64)g.NW) * 64 + lane;
        const long long X = i * g.pitch + ((j & 1) ? g.shift : 0), Y = j * g.row;
        const bool ex = X < g.W;
        const bool ink = ex && fl_ink(g.ink, X, Y);
        // the source pixel of an ink candidate: inside the mask, so it fits an int
        const int c = ink ? (int)fl_floordiv((X - g.ink.dx) * g.ink.den, g.ink.num) : 0, r = ink ? (int)fl_floordiv((Y - g.ink.dy) * g.ink.den, g.ink.num) : 0;
        const u64 me = __ballot(ex), mi = __ballot(ink);
        bool clear = false;
        if (wave_clear) {
            for (u64 m = mi; m; m &= m - 1) {
                const int src = __ffsll((long long)m) - 1;
                const bool ok = fs_wave_clear(g.ink, __shfl(c, src), __shfl(r, src), g.cr, lane);
                if (lane == src) clear = ok;
            }
        } else clear = ink && fs_lane_clear(g.ink, c, r, g.cr);
        const u64 mc = __ballot(clear);
        bool isdot = clear;                                                           // without a tone image every clear candidate is a dot (see above)
        if (g.G) {
            int C = 1, S = 0;
            if (wave_tone) {
                for (u64 m = mc; m; m &= m - 1) {
                    const int src = __ffsll((long long)m) - 1;
                    int wC, wS;
                    fs_wave_tone(g, __shfl(c, src), __shfl(r, src), lane, wC, wS);
                    if (lane == src) { C = wC; S = wS; }
                }
            } else if (clear) fs_lane_tone(g, c, r, C, S);
            const int R = g.hi - g.lo, E = min(max(255 * C - S - g.lo * C, 0), R * C);
            const int x = (int)(i & 7), y = (int)(j & 7), v = x ^ y;
            const int T = ((v & 1) << 5) | ((y & 1) << 4) | ((v & 2) << 2) | ((y & 2) << 1) | ((v & 4) >> 1) | ((y & 4) >> 2);
            isdot = clear && 64 * E > T * R * C;
        }
        const u64 md = __ballot(isdot);
        n_cand += (u64)__popcll(me); n_ink += (u64)__popcll(mi); n_near += (u64)__popcll(mi & ~mc); n_light += (u64)__popcll(mc & ~md); n_dots += (u64)__popcll(md);
        if (lane == 0) { dot[z] = md; cnt[z] = (u64)__popcll(md); }
    }
    if (lane == 0 && n_cand) {
        atomicAdd(&cn->candidates, n_cand); atomicAdd(&cn->ink, n_ink); atomicAdd(&cn->near, n_near); atomicAdd(&cn->light, n_light); atomicAdd(&cn->dots, n_dots);
    }
}

// ------------------------------------------------------------------------------------------------ 3. emit
__global__ __launch_bounds__(256) void k_fs_emit(FsGrid g, u64 D, const u64* __restrict__ dot, const u64* __restrict__ sc, int serpentine, int2* __restrict__ xy, FsCounters* cn) {
    const int lane = threadIdx.x & 63;
    const u64 below = (1ull << lane) - 1;
    for (u64 z = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); z < g.Z; z += (u64)gridDim.x * 4) {
        const u64 w = dot[z];
        if (!((w >> lane) & 1)) continue;
        const u64 j = z / (u64)g.NW;
        const long long i = (long long)(z % (u64)g.NW) * 64 + lane;
        u64 at = sc[z] + (u64)__popcll(w & below);
        if (serpentine && (j & 1)) {                                                  // from the row's other end: its dots are [d0, d1)
            const u64 z0 = j * (u64)g.NW, d0 = sc[z0], d1 = sc[z0 + (u64)g.NW];
            at = d0 + d1 - 1 - at;
        }
        if (at >= D) { atomicOr(&cn->bad, FS_BAD_PLACE); continue; }
        xy[at] = make_int2((int)(i * g.pitch + ((j & 1) ? g.shift : 0)), (int)((long long)j * g.row));
    }
}
}  // namespace

// include/orip.h states the rule; the dots wait in c->fs_out for the fetch
extern "C" int orip_fill_stipple(orip_ctx* c, const uint8_t* mask, int layer, const uint8_t* tone, int h, int w, int W, int H, int32_t num, int32_t den, int32_t dx, int32_t dy,
                                 int32_t pitch, int32_t row, int32_t shift, int32_t clear_rad, int32_t tone_rad, int32_t lo, int32_t hi, int32_t flags, int64_t* stats) {
    orip_enter(c);
    constexpr int TOP = ORIP_FILL_COORD_MAX;
    if (!stats) ORIP_FAIL(c, "bad arguments");
    if (flags & ~ORIP_FILL_STIPPLE_SERPENTINE) ORIP_FAIL(c, "unknown flags %d", flags);
    if (h < 1 || w < 1 || h > TOP || w > TOP || (long long)h * w >= (1ll << 31)) ORIP_FAIL(c, "mask %d x %d: each side in 1..2^20, fewer than 2^31 pixels", w, h);
    if (W < 1 || H < 1 || W > TOP || H > TOP) ORIP_FAIL(c, "canvas %d x %d: each side in 1..2^20", W, H);
    if (num < 1 || num > TOP || den < 1 || den > TOP) ORIP_FAIL(c, "placement scale %d / %d: both in 1..2^20", num, den);
    if (dx < -TOP || dx > TOP || dy < -TOP || dy > TOP) ORIP_FAIL(c, "placement offset (%d, %d): both in -2^20..2^20", dx, dy);
    if (pitch < 2 || pitch > ORIP_FILL_LEN_MAX) ORIP_FAIL(c, "pitch %d: 2..2^15", pitch);
    if (row < 1 || row > ORIP_FILL_LEN_MAX) ORIP_FAIL(c, "row %d: 1..2^15", row);
    if (shift < 0 || shift >= pitch) ORIP_FAIL(c, "shift %d: 0..pitch - 1", shift);
    if (clear_rad < 0 || clear_rad > ORIP_FILL_STIPPLE_RAD_MAX) ORIP_FAIL(c, "clear_rad %d: 0..%d", clear_rad, ORIP_FILL_STIPPLE_RAD_MAX);
    if (tone_rad < 0 || tone_rad > ORIP_FILL_STIPPLE_RAD_MAX) ORIP_FAIL(c, "tone_rad %d: 0..%d", tone_rad, ORIP_FILL_STIPPLE_RAD_MAX);
    if (lo < 0 || hi > 255 || lo >= hi) ORIP_FAIL(c, "lo %d, hi %d: 0 <= lo < hi <= 255", lo, hi);
    if (!mask) {
        if (!c->masks.p || layer < 0 || layer >= c->K) ORIP_FAIL(c, "no mask resident for layer %d", layer);
        if (h != c->H || w != c->W) ORIP_FAIL(c, "mask %d x %d given, the resident masks are %d x %d", w, h, c->W, c->H);
    }
    FsGrid g{};
    g.ink = FlInk{nullptr, h, w, num, den, dx, dy};
    g.W = W; g.pitch = pitch; g.row = row; g.shift = shift; g.cr = clear_rad; g.tr = tone_rad; g.lo = lo; g.hi = hi;
    const long long NI = (W - 1) / pitch + 1, NJ = (H - 1) / row + 1;                 // the candidates of an even row; the rows
    g.NW = (int)((NI + 63) / 64);
    g.Z = (u64)NJ * (u64)g.NW;
    if (g.Z >= FS_MAX_BLOCKS) ORIP_FAIL(c, "%llu blocks of 64 candidates over %lld rows: fewer than 2^26", g.Z, NJ);

    for (int k = 0; k < ORIP_FILL_STIPPLE_STATS; k++) stats[k] = 0;
    c->fs_dots = -1;                                                          // no dot list from here to the last read-back
    hipStream_t s = LN(c).stream;
    const size_t Z = (size_t)g.Z, px = (size_t)h * w;
    u8 *d_mask, *d_tone; u64 *dot, *cnt, *sc; FsCounters* cn;
    { Carve L; L.take(d_mask, mask ? px : 0); L.take(d_tone, tone ? px : 0); L.take(dot, Z); L.take(cnt, Z + 1); L.take(sc, Z + 1); L.take(cn, 1); HIPC(c, L.commit(c->fs_tmp, 64)); }
    if (mask) HIPC(c, hipMemcpyAsync(d_mask, mask, px, hipMemcpyHostToDevice, s));
    if (tone) HIPC(c, hipMemcpyAsync(d_tone, tone, px, hipMemcpyHostToDevice, s));
    g.ink.M = mask ? d_mask : c->masks.as<u8>() + px * (size_t)layer;
    g.G = tone ? d_tone : nullptr;
    HIPC(c, hipMemsetAsync(cn, 0, sizeof(FsCounters), s));
    const dim3 b(256), gw((unsigned)std::min<u64>((g.Z + 3) / 4, FS_BLOCKS));
    { ProfScope ps(c, "fs_verdict");
      hipLaunchKernelGGL(k_fs_verdict, gw, b, 0, s, g, dot, cnt, cn);
      HIPC(c, gc_scan_u64(c, cnt, sc, Z + 1)); }
    HIPC(c, hipGetLastError());
    u64 D = 0;
    FsCounters hc;
    HIPC(c, hipMemcpyAsync(&D, sc + Z, 8, hipMemcpyDeviceToHost, s));                // first read-back: the dots
    HIPC(c, hipMemcpyAsync(&hc, cn, sizeof(FsCounters), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (D >= FS_MAX_DOTS) ORIP_FAIL(c, "%llu dots: fewer than 2^26", D);
    if (hc.dots != D || hc.near + hc.light + hc.dots != hc.ink) ORIP_FAIL(c, "the dots do not add up (%llu placed, %llu counted)", D, hc.dots);
    if (D) {
        int2* xy;
        { Carve L; L.take(xy, (size_t)D); HIPC(c, L.commit(c->fs_out, 64)); }
        { ProfScope ps(c, "fs_emit");
          hipLaunchKernelGGL(k_fs_emit, gw, b, 0, s, g, D, dot, sc, (flags & ORIP_FILL_STIPPLE_SERPENTINE) ? 1 : 0, xy, cn); }
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(&hc, cn, sizeof(FsCounters), hipMemcpyDeviceToHost, s));      // second read-back: the place check
        HIPC(c, hipStreamSynchronize(s));
        if (hc.bad) ORIP_FAIL(c, "the dots do not add up (internal error %u)", hc.bad);
    }
    c->fs_dots = (int64_t)D;
    stats[0] = (int64_t)hc.candidates; stats[1] = (int64_t)hc.ink; stats[2] = (int64_t)hc.near; stats[3] = (int64_t)hc.light; stats[4] = (int64_t)hc.dots;
    return 0;
}

extern "C" int orip_fill_stipple_fetch(orip_ctx* c, int32_t* xy) {
    orip_enter(c);
    if (c->fs_dots < 0) ORIP_FAIL(c, "no result: the fill stipple has not succeeded since the last failure");
    if (c->fs_dots == 0) return 0;
    if (!xy) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(xy, c->fs_out.p, (size_t)c->fs_dots * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
