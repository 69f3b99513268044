// csrc/gc_convert.h -- what the gcode units share.  The arithmetic of mm_to_steps (gcode2stream.py :79-110) up to the rounding, stated once for the two
// conversions that must agree in every bit: orip_gcode_to_steps (gcode.hip), which then clamps to the sheet, and orip_gcode_to_steps_clip (gcode_clip.hip),
// which cuts there instead; the path of a point; the check of an offsets array.
#pragma once
#include "orip_ctx.h"

constexpr int GC_COORD_MAX = 1 << 30;            // step coordinates are int32 in [0, 2^30]

// (v * scale + offset) * steps_per_mm in IEEE double, the three operations kept apart, (H - 1) - y under invert_y, round half to even (Python's round());
// false when a coordinate is not finite afterwards.  Nothing is clamped and nothing is cast here.
__device__ __forceinline__ bool gc_round_mm(const orip_gcode_map& g, double xm, double ym, double& xf, double& yf) {
    xf = __dmul_rn(__dadd_rn(__dmul_rn(xm, g.scale_x), g.offset_x_mm), g.steps_per_mm);
    yf = __dmul_rn(__dadd_rn(__dmul_rn(ym, g.scale_y), g.offset_y_mm), g.steps_per_mm);
    if (g.invert_y) yf = __dsub_rn((double)(g.H - 1), yf);
    xf = rint(xf); yf = rint(yf);
    return isfinite(xf) && isfinite(yf);
}

// last p with off[p] <= i (paths without points are skipped by the search)
__device__ __forceinline__ int64_t gc_path_of(const long long* __restrict__ off, int64_t n, int64_t i) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

// the offsets of n explicit paths: off[0] == 0, nowhere decreasing; the message names the entry point `who`
static inline int gc_check_offsets(orip_ctx* c, const char* who, const int64_t* off, int64_t n) {
    if (off[0] != 0) ORIP_FAIL_AS(c, who, "offsets must start at 0");
    for (int64_t p = 0; p < n; p++) if (off[p + 1] < off[p]) ORIP_FAIL_AS(c, who, "offsets must not decrease (path %lld)", (long long)p);
    return 0;
}
