// csrc/gc_convert.h -- what the gcode units share.  The arithmetic of mm_to_steps (gcode2stream.py :79-110) up to the rounding, stated once for the two
// conversions that must agree in every bit: orip_gcode_to_steps (gcode.hip), which then clamps to the sheet, and orip_gcode_to_steps_clip (gcode_clip.hip),
// which cuts there instead; the path of a point; the host side of the resident step polylines: the intake of both input forms, the hand-over, the orders' checks.
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

// A ring point of the passes whose shapes are resident fitted paths (the occlusion, the hatch link): the conversion above, clamped to the sheet as
// orip_gcode_to_steps clamps when `clamp` is set, and nothing else: no point is dropped.  0, or why there is no point: the coordinate is not finite, or it
// lies outside +-2^30 (o is then (0, 0))
constexpr unsigned GC_RING_NOT_FINITE = 1, GC_RING_RANGE = 2;
__device__ __forceinline__ unsigned gc_ring_step(const orip_gcode_map& g, const double2 mm, int clamp, int2& o) {
    double xf, yf;
    o = make_int2(0, 0);
    if (!gc_round_mm(g, mm.x, mm.y, xf, yf)) return GC_RING_NOT_FINITE;
    if (clamp) {
        const double xmax = (double)(g.W - 1), ymax = (double)(g.H - 1);
        xf = xf < 0.0 ? 0.0 : (xf > xmax ? xmax : xf);
        yf = yf < 0.0 ? 0.0 : (yf > ymax ? ymax : yf);
    }
    const double top = (double)GC_COORD_MAX;
    if (xf < -top || xf > top || yf < -top || yf > top) return GC_RING_RANGE;
    o = make_int2((int)xf, (int)yf);
    return 0;
}

// last p with off[p] <= i (paths without points are skipped by the search)
__device__ __forceinline__ int64_t gc_path_of(const long long* __restrict__ off, int64_t n, int64_t i) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

// ---- host helpers, defined in gcode.hip; `who` is the entry point's __func__, which every message names.  orip_ctx.h states the contract they keep
// mm paths, explicit or (off == pts_mm == NULL, n > 0) the n fitted paths of svg.hip: the form (others_ok: the entry point's own pointers), the resident
// count, the map, fewer than 2^30 paths, the offsets; then, behind the caller's Carve of d_off[n + 1] and d_mm[total] (0 of each when resident), the upload
int gc_mm_check(orip_ctx* c, const char* who, const int64_t* off, const double* pts_mm, int64_t n, const orip_gcode_map* map, bool others_ok, bool& resident, int64_t& total);
int gc_mm_upload(orip_ctx* c, const char* who, const int64_t* off, const double* pts_mm, int64_t n, int64_t total, bool resident, long long*& d_off, double2*& d_mm);
// step polylines, explicit or (off == pts == NULL) the n resident ones, at most 2^26, of fewer than 2^max_log2 points (looked at before any point is): every
// check of the form, no state touched (no_repeats: no point equals the one before it); then the upload that makes a checked explicit input the resident list.  gc_merged is the caller's, here and below
int gc_steps_check(orip_ctx* c, const char* who, const int64_t* off, const int32_t* pts, int64_t n, bool no_repeats, int64_t& total, int max_log2 = 30);
int gc_steps_upload(orip_ctx* c, const char* who, const int64_t* off, const int32_t* pts, int64_t n, int64_t total);
void gc_drop(orip_ctx* c);                                                              // no list: every reader fails until a writer succeeds
int gc_publish_empty(orip_ctx* c, const char* who);                                     // the list of no polylines
void gc_publish(orip_ctx* c, DBuf& off, DBuf& pts, int64_t n, int64_t total);           // a result in (off, pts) becomes the list: the buffers are swapped
void gc_publish_src(orip_ctx* c, DBuf& src);                                            // the sources of the list just published, gathered by its writer: swapped in
// the orders' checks: n polylines resident; n_groups in 1..64 and every path's group in range, counted into paths[] when given; the start point
int gc_check_resident(orip_ctx* c, const char* who, int64_t n);
int gc_check_groups(orip_ctx* c, const char* who, const int32_t* group, int64_t n, int32_t n_groups, int64_t* paths);
int gc_check_start(orip_ctx* c, const char* who, const int32_t* start_xy, int& sx, int& sy);
