// csrc/fill_common.h -- what fill.hip (orip_fill_mask) and fill_link.hip (orip_fill_link) share: the floor division and INK, each stated once.
#pragma once
#include "orip_ctx.h"

__host__ __device__ __forceinline__ long long fl_floordiv(long long a, long long b) { const long long q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }     // b > 0

// the mask on the canvas: M u8[h w] on the device, placed by (num, den, dx, dy)
struct FlInk { const u8* M; int h, w; long long num, den, dx, dy; };
// canvas pixel (X, Y) is INK (include/orip.h: orip_fill_mask); every integer (X, Y) has an answer, and no index leaves the mask
__device__ __forceinline__ bool fl_ink(const FlInk& g, long long X, long long Y) {
    const long long c = fl_floordiv((X - g.dx) * g.den, g.num), r = fl_floordiv((Y - g.dy) * g.den, g.num);
    return c >= 0 && c < g.w && r >= 0 && r < g.h && g.M[(size_t)r * (size_t)g.w + (size_t)c] != 0;
}
