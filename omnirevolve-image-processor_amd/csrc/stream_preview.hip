// csrc/stream_preview.hip -- 14_preview_stream.py headless (shared/omnirevolve_plotter_stream_previewer.py -o out.png): decode plot_stream.bin,
// replay it command by command and draw what the pen draws, plus the previewer's statistics (StreamDecoder._decode, PlotterPreview._process_one,
// _steps_to_px, _rebuild_render_surface, _print_stats).
//
// Decoding is a prefix scan.  Every byte's effect on the replay state is an element of a monoid: (commands, dx, dy, last pen event, last colour
// event, first EOF); the product of two is "the left one if it holds an EOF, else sums / the right's last events".  A tile is 256 threads x 16
// bytes; four launches whose count does not depend on the stream length, with no spin-waits between workgroups:
//   k_sp_reduce   per tile: the product of its bytes (block scan in LDS)
//   k_sp_scan     ONE workgroup: exclusive scan of the tile products -> the state entering every tile; the totals; clears the counters
//   k_sp_draw     per tile again: the state entering every thread (tile prefix x block exclusive scan), then each thread replays its 16 bytes in
//                 order: statistics (block-reduced, one atomic add per counter and tile) and the raster.  A pixel holds the 64-bit key
//                 4 * (command ordinal, 1-based) + palette index of the last command to draw it (atomicMax: "last writer wins" across threads
//                 and workgroups); a thread only issues the atomic when its walk moves to another pixel (at step_scale 0.076, the reference
//                 stage's, about 13 consecutive steps land on one pixel), or for every pixel of a tap disc
//   k_sp_resolve  key -> RGB (palette[min(idx, 3)], background where no command drew)
//
// Geometry in IEEE double in the previewer's order (no fused multiply-add: -ffp-contract=off and explicit _rn intrinsics):
//   px = int(offset_x + x * step_scale), py = int(offset_y + (H - 1 - y) * step_scale) (invert_y) or int(offset_y + y * step_scale); int()
//   truncates toward zero.  Clip: the workspace rect, or the surface under --no-clip.
// PARITY UNPINNED (pygame's scan conversion; tests/stream_preview_double.py restates exactly this):
//   * a 1-px line p0 -> p1: n = max(|dx|, |dy|), pixels p0 + floor((2 j d + n) / (2 n)), j = 0..n.  At step_scale <= 1 (the stage's 1200 x 900
//     default and every render up to the canvas size) consecutive steps land at most one pixel apart and this is exactly {p0, p1}, which is
//     what pygame draws too; above 1 it is a stand-in
//   * a tap: the disc (px + i, py + j), i^2 + j^2 <= r^2, r = max(1, 10 // 2)
#include "orip_ctx.h"
#include <algorithm>

namespace {
constexpr int SP_T = 256, SP_B = 16, SP_TILE = SP_T * SP_B;
enum { C_SERVICE, C_STEPB, C_SINGLE, C_DOUBLE, C_PENSEG, C_TAPS, C_COLOR, C_SPEED, C_OFF, C_UNKNOWN, SP_NCNT };

struct Agg {
    long long cmds;     // commands
    long long eof;      // byte index of the first EOF, -1: none (nothing after it counts)
    int dx, dy;
    int pen;            // last pen event: 0 none, 1 up (0x01, and 0x03 which lifts the pen), 2 down
    int col;            // last colour event, -1: none
};
__device__ __forceinline__ Agg agg_id() { Agg a; a.cmds = 0; a.eof = -1; a.dx = a.dy = 0; a.pen = 0; a.col = -1; return a; }
__device__ __forceinline__ Agg agg_mul(const Agg& a, const Agg& b) {
    if (a.eof >= 0) return a;
    Agg r; r.cmds = a.cmds + b.cmds; r.eof = b.eof; r.dx = a.dx + b.dx; r.dy = a.dy + b.dy;
    r.pen = b.pen ? b.pen : a.pen; r.col = b.col >= 0 ? b.col : a.col;
    return r;
}
// STEP_DIRS 0 +Y, 1 NE, 2 +X, 3 SE, 4 -Y, 5 SW, 6 -X, 7 NW as 2-bit fields of d + 1
__device__ __forceinline__ int dir_dx(int c) { return (int)((0x1a9u >> (2 * c)) & 3u) - 1; }
__device__ __forceinline__ int dir_dy(int c) { return (int)((0x901au >> (2 * c)) & 3u) - 1; }

__device__ __forceinline__ void agg_byte(Agg& a, unsigned b, long long g) {
    if (a.eof >= 0) return;
    if (b & 0x80u) {
        const int c1 = (b >> 3) & 7;
        a.dx += dir_dx(c1); a.dy += dir_dy(c1); a.cmds++;
        if (b & 0x40u) { const int c2 = b & 7; a.dx += dir_dx(c2); a.dy += dir_dy(c2); a.cmds++; }
    } else if (b == 0x3Fu) a.eof = g;
    else if (b >= 1u && b <= 3u) { a.pen = b == 2u ? 2 : 1; a.cmds++; }
    else if (b >= 8u && b <= 15u) { a.col = (int)(b & 7u); a.cmds++; }
    else if ((b & 0xC0u) == 0x40u) a.cmds++;
}
__device__ __forceinline__ unsigned byte_of(const uint4& v, int i) {
    const unsigned w = i < 4 ? v.x : i < 8 ? v.y : i < 12 ? v.z : v.w;
    return (w >> (8 * (i & 3))) & 0xffu;
}
// the 16 bytes of thread t of tile `tile` (the device copy is padded to whole tiles) and their product
__device__ __forceinline__ Agg thread_agg(const uint8_t* __restrict__ data, int64_t n, int64_t first, uint4& v) {
    v = *reinterpret_cast<const uint4*>(data + first);
    Agg a = agg_id();
    const int cnt = (int)min((int64_t)SP_B, n - first);
    for (int i = 0; i < cnt; i++) agg_byte(a, byte_of(v, i), first + i);
    return a;
}
// inclusive scan of one Agg per thread over the block (Hillis-Steele in LDS); s[SP_T - 1] is the block product afterwards
__device__ __forceinline__ Agg block_scan(Agg a, Agg* s) {
    const int t = threadIdx.x;
    s[t] = a;
    __syncthreads();
    for (int off = 1; off < SP_T; off <<= 1) {
        Agg v = s[t];
        if (t >= off) v = agg_mul(s[t - off], v);
        __syncthreads();
        s[t] = v;
        __syncthreads();
    }
    return s[t];
}

__global__ __launch_bounds__(SP_T) void k_sp_reduce(const uint8_t* __restrict__ data, int64_t n, Agg* __restrict__ tile_agg) {
    __shared__ Agg s[SP_T];
    const int64_t first = (int64_t)blockIdx.x * SP_TILE + (int64_t)threadIdx.x * SP_B;
    uint4 v;
    block_scan(thread_agg(data, n, first, v), s);
    if (threadIdx.x == SP_T - 1) tile_agg[blockIdx.x] = s[SP_T - 1];
}

__global__ __launch_bounds__(SP_T) void k_sp_scan(const Agg* __restrict__ tile_agg, int ntiles, Agg* __restrict__ tile_pre, Agg* __restrict__ total,
                                                 unsigned long long* __restrict__ counters) {
    __shared__ Agg s[SP_T];
    const int t = threadIdx.x;
    if (t < SP_NCNT) counters[t] = 0;
    Agg carry = agg_id();
    for (int base = 0; base < ntiles; base += SP_T) {
        const bool in = base + t < ntiles;
        block_scan(in ? tile_agg[base + t] : agg_id(), s);
        if (in) tile_pre[base + t] = agg_mul(carry, t ? s[t - 1] : agg_id());
        const Agg blk = s[SP_T - 1];
        __syncthreads();
        carry = agg_mul(carry, blk);
    }
    if (t == 0) *total = carry;
}

struct Geo {
    double scale;
    int W, H, ox, oy;          // canvas in steps, workspace offset
    int cx0, cy0, cx1, cy1;    // clip rect [cx0, cx1) x [cy0, cy1)
    int rw, invert, taps, r;   // surface width, invert_y, render taps, tap radius
};
__device__ __forceinline__ long long to_px(const Geo& g, int x) { return (long long)__dadd_rn((double)g.ox, __dmul_rn((double)x, g.scale)); }
__device__ __forceinline__ long long to_py(const Geo& g, int y) {
    const long long yy = g.invert ? (long long)g.H - 1 - y : (long long)y;
    return (long long)__dadd_rn((double)g.oy, __dmul_rn((double)yy, g.scale));
}
__device__ __forceinline__ long long floor_div(long long a, long long b) {   // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
struct Pending {             // the pixel a thread's walk is on and the largest key it has for it
    long long x = 0, y = 0; unsigned long long key = 0; bool on = false;
};
__device__ __forceinline__ void flush(Pending& p, const Geo& g, unsigned long long* __restrict__ keys) {
    if (p.on) atomicMax(&keys[(size_t)p.y * g.rw + p.x], p.key);
    p.on = false;
}
__device__ __forceinline__ void plot(Pending& p, const Geo& g, unsigned long long* __restrict__ keys, long long x, long long y, unsigned long long key) {
    if (x < g.cx0 || x >= g.cx1 || y < g.cy0 || y >= g.cy1) return;
    if (p.on && p.x == x && p.y == y) { p.key = key; return; }
    flush(p, g, keys);
    p.x = x; p.y = y; p.key = key; p.on = true;
}
__device__ void draw_line(Pending& p, const Geo& g, unsigned long long* __restrict__ keys, long long x0, long long y0, long long x1, long long y1,
                          unsigned long long key) {
    const long long dx = x1 - x0, dy = y1 - y0;
    const long long n = max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy), nn = n > 0 ? n : 1;
    for (long long j = 0; j <= n; j++) plot(p, g, keys, x0 + floor_div(2 * j * dx + nn, 2 * nn), y0 + floor_div(2 * j * dy + nn, 2 * nn), key);
}
__device__ void draw_disc(const Geo& g, unsigned long long* __restrict__ keys, long long cx, long long cy, unsigned long long key) {
    for (int j = -g.r; j <= g.r; j++) {
        const long long y = cy + j;
        if (y < g.cy0 || y >= g.cy1) continue;
        for (int i = -g.r; i <= g.r; i++) {
            const long long x = cx + i;
            if (i * i + j * j <= g.r * g.r && x >= g.cx0 && x < g.cx1) atomicMax(&keys[(size_t)y * g.rw + x], key);
        }
    }
}

__global__ __launch_bounds__(SP_T) void k_sp_draw(const uint8_t* __restrict__ data, int64_t n, const Agg* __restrict__ tile_pre, Geo g,
                                                 unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counters) {
    __shared__ Agg s[SP_T];
    __shared__ unsigned long long cnt_s[SP_NCNT];
    const int t = threadIdx.x;
    if (t < SP_NCNT) cnt_s[t] = 0;
    const int64_t first = (int64_t)blockIdx.x * SP_TILE + (int64_t)t * SP_B;
    uint4 v;
    const Agg mine = thread_agg(data, n, first, v);
    block_scan(mine, s);
    const Agg in = agg_mul(tile_pre[blockIdx.x], t ? s[t - 1] : agg_id());
    unsigned c[SP_NCNT] = {0};
    if (in.eof < 0) {
        int x = in.dx, y = in.dy, col = in.col < 0 ? 0 : in.col;
        bool down = in.pen == 2;
        unsigned long long ord = (unsigned long long)in.cmds;
        long long px = to_px(g, x), py = to_py(g, y);
        Pending p;
        const int cntb = (int)min((int64_t)SP_B, n - first);
        for (int i = 0; i < cntb; i++) {
            const unsigned b = byte_of(v, i);
            if (b & 0x80u) {
                c[C_STEPB]++;
                const int ns = (b & 0x40u) ? 2 : 1;
                if (ns == 2) c[C_DOUBLE]++; else c[C_SINGLE]++;
                for (int k = 0; k < ns; k++) {
                    const int code = k == 0 ? (int)((b >> 3) & 7u) : (int)(b & 7u);
                    ord++;
                    x += dir_dx(code); y += dir_dy(code);
                    if (!(x >= 0 && x < g.W && y >= 0 && y < g.H)) c[C_OFF]++;
                    const long long nx = to_px(g, x), ny = to_py(g, y);
                    if (down) draw_line(p, g, keys, px, py, nx, ny, (ord << 2) | (unsigned long long)min(col, 3));
                    px = nx; py = ny;
                }
                continue;
            }
            c[C_SERVICE]++;
            if (b == 0x3Fu) break;
            if (b >= 1u && b <= 3u) {
                ord++;
                if (b == 1u) down = false;
                else if (b == 2u) { if (!down) c[C_PENSEG]++; down = true; }
                else {
                    c[C_TAPS]++;
                    if (g.taps) draw_disc(g, keys, px, py, (ord << 2) | (unsigned long long)min(col, 3));
                    down = false;
                }
            } else if (b >= 8u && b <= 15u) { ord++; col = (int)(b & 7u); c[C_COLOR]++; }
            else if ((b & 0xC0u) == 0x40u) { ord++; c[C_SPEED]++; }
            else c[C_UNKNOWN]++;
        }
        flush(p, g, keys);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SP_NCNT; k++) if (c[k]) atomicAdd(&cnt_s[k], (unsigned long long)c[k]);
    __syncthreads();
    if (t < SP_NCNT && cnt_s[t]) atomicAdd(&counters[t], cnt_s[t]);
}

struct Pal { uint8_t rgb[15]; };   // palette 0..3, then the background
__global__ __launch_bounds__(256) void k_sp_resolve(const unsigned long long* __restrict__ keys, int64_t npx, Pal pal, uint8_t* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    const unsigned long long k = keys[i];
    const int e = k ? (int)(k & 3ull) : 4;
    rgb[3 * i] = pal.rgb[3 * e]; rgb[3 * i + 1] = pal.rgb[3 * e + 1]; rgb[3 * i + 2] = pal.rgb[3 * e + 2];
}
}  // namespace

extern "C" int orip_stream_preview(orip_ctx* c, const uint8_t* data, int64_t n, int W, int H, int rw, int rh, int flags, const uint8_t* palette_rgb,
                                   int tap_radius, int64_t* stats) {
    orip_enter(c);
    c->sp_ready = false;
    if (n < 0 || (n > 0 && !data) || !palette_rgb || !stats) ORIP_FAIL(c, "bad arguments");
    if (n > (int64_t)(INT32_MAX / 2)) ORIP_FAIL(c, "stream of %lld bytes: step positions are int32, at most %d bytes", (long long)n, INT32_MAX / 2);
    if (W < 1 || H < 1) ORIP_FAIL(c, "canvas %d x %d steps: must be positive", W, H);
    if (rw < 1 || rh < 1 || rw > ORIP_PREVIEW_MAX_SIDE || rh > ORIP_PREVIEW_MAX_SIDE) ORIP_FAIL(c, "render size %d x %d: each side must be in 1..%d", rw, rh, ORIP_PREVIEW_MAX_SIDE);
    if (tap_radius < 1 || tap_radius > 1024 || (flags & ~15)) ORIP_FAIL(c, "bad arguments (tap_radius %d, flags 0x%x)", tap_radius, flags);
    hipStream_t s = LN(c).stream;
    const int64_t ntiles = n > 0 ? (n + SP_TILE - 1) / SP_TILE : 1;     // one (empty) tile for an empty stream: the launch count stays fixed
    const int64_t npx = (int64_t)rw * rh;
    HIPC(c, hipStreamSynchronize(s));                                    // buffers only grow, and a regrow frees: nothing may still use them
    HIPC(c, c->sp_data.ensure((size_t)ntiles * SP_TILE + 64));
    HIPC(c, c->sp_agg.ensure((size_t)(2 * ntiles + 1) * sizeof(Agg) + SP_NCNT * 8 + 64));
    HIPC(c, c->sp_keys.ensure((size_t)npx * 8 + 64));
    HIPC(c, c->sp_rgb.ensure((size_t)npx * 3 + 64));
    Agg* tile_agg = c->sp_agg.as<Agg>();
    Agg* tile_pre = tile_agg + ntiles;
    Agg* total = tile_pre + ntiles;
    unsigned long long* counters = reinterpret_cast<unsigned long long*>(total + 1);
    // _rebuild_render_surface with the render size granted as asked
    Geo g;
    g.scale = std::min((double)rw / (double)W, (double)rh / (double)H);
    const int used_w = (int)((double)W * g.scale), used_h = (int)((double)H * g.scale);
    g.W = W; g.H = H; g.ox = (rw - used_w) / 2; g.oy = (rh - used_h) / 2;          // rw >= used_w: floor division == truncation
    const bool clip = (flags & 2) != 0;
    g.cx0 = clip ? std::max(g.ox, 0) : 0; g.cy0 = clip ? std::max(g.oy, 0) : 0;
    g.cx1 = clip ? std::min(g.ox + used_w, rw) : rw; g.cy1 = clip ? std::min(g.oy + used_h, rh) : rh;
    g.rw = rw; g.invert = (flags & 1) != 0; g.taps = (flags & 4) != 0; g.r = tap_radius;
    Pal pal;
    memcpy(pal.rgb, palette_rgb, 12);
    memset(pal.rgb + 12, (flags & 8) ? 255 : 0, 3);
    if (n > 0) HIPC(c, hipMemcpyAsync(c->sp_data.p, data, (size_t)n, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(c->sp_keys.p, 0, (size_t)npx * 8, s));
    { ProfScope ps(c, "k_sp_reduce");
      hipLaunchKernelGGL(k_sp_reduce, dim3((unsigned)ntiles), dim3(SP_T), 0, s, c->sp_data.as<uint8_t>(), n, tile_agg); }
    { ProfScope ps(c, "k_sp_scan");
      hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(SP_T), 0, s, tile_agg, (int)ntiles, tile_pre, total, counters); }
    { ProfScope ps(c, "k_sp_draw");
      hipLaunchKernelGGL(k_sp_draw, dim3((unsigned)ntiles), dim3(SP_T), 0, s, c->sp_data.as<uint8_t>(), n, tile_pre, g, c->sp_keys.as<unsigned long long>(), counters); }
    { ProfScope ps(c, "k_sp_resolve");
      hipLaunchKernelGGL(k_sp_resolve, dim3((unsigned)cdiv(npx, 256)), dim3(256), 0, s, c->sp_keys.as<unsigned long long>(), npx, pal, c->sp_rgb.as<uint8_t>()); }
    HIPC(c, hipGetLastError());
    struct { Agg tot; unsigned long long cnt[SP_NCNT]; } h;
    static_assert(sizeof(h) == sizeof(Agg) + SP_NCNT * 8, "totals and counters are adjacent on the device");
    HIPC(c, hipMemcpyAsync(&h, total, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    const unsigned long long* k = h.cnt;
    const int64_t out[ORIP_STREAM_STATS] = {n, (int64_t)k[C_SERVICE], (int64_t)k[C_STEPB], (int64_t)k[C_SINGLE], (int64_t)k[C_DOUBLE],
                                            (int64_t)(k[C_SINGLE] + 2 * k[C_DOUBLE]), (int64_t)k[C_PENSEG], (int64_t)k[C_TAPS], (int64_t)k[C_COLOR],
                                            (int64_t)k[C_SPEED], h.tot.eof >= 0 ? 1 : 0, h.tot.eof >= 0 ? n - (h.tot.eof + 1) : 0, (int64_t)k[C_OFF],
                                            h.tot.dx, h.tot.dy, (int64_t)k[C_UNKNOWN], h.tot.cmds};
    memcpy(stats, out, sizeof(out));
    c->sp_rw = rw; c->sp_rh = rh; c->sp_ready = true;
    return 0;
}

extern "C" int orip_stream_preview_fetch(orip_ctx* c, uint8_t* rgb) {
    orip_enter(c);
    if (!rgb) ORIP_FAIL(c, "bad arguments");
    if (!c->sp_ready) ORIP_FAIL(c, "no preview: orip_stream_preview has not succeeded since the last failure");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(rgb, c->sp_rgb.p, (size_t)c->sp_rw * c->sp_rh * 3, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
