// csrc/gcode.hip -- the device side of svg_to_stream/gcode2stream.py's conversion: pen-down paths in mm -> step polylines (convert_polylines_to_steps :305-341
// with mm_to_steps :79-110), resident for what follows.  Parsing and the speed plan stay on the host; the nearest-neighbour order of the paths is
// gcode_order.hip, the bytes of the finished stream are stream.hip (orip_stream_pack).
//
// Paths to steps.  One thread per point: (v * scale + offset) * steps_per_mm in IEEE double, the three operations kept apart (_rn intrinsics, and the
// tree builds with -ffp-contract=off), (H - 1) - y under invert_y, round half to even, clamp to the sheet.  A point is kept when its step position differs
// from its predecessor's (the reference compares with the last point it appended, which is always the predecessor's position).  A scan compacts the
// points, a second one drops the paths left with fewer than two.  A non-finite coordinate in a path of two or more points is an error, as it is for the
// reference (int(round(inf)) raises).
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>

namespace {
// ------------------------------------------------------------------------------------------------ paths to steps
__device__ __forceinline__ bool gc_step(const orip_gcode_map& g, double xm, double ym, int2& o) {
    double xf, yf;
    o = make_int2(0, 0);
    if (!gc_round_mm(g, xm, ym, xf, yf)) return false;                // gc_convert.h: the arithmetic and Python's round(), shared with gcode_clip.hip
    const double xmax = (double)(g.W - 1), ymax = (double)(g.H - 1);
    xf = xf < 0.0 ? 0.0 : (xf > xmax ? xmax : xf);
    yf = yf < 0.0 ? 0.0 : (yf > ymax ? ymax : yf);
    o = make_int2((int)xf, (int)yf);
    return true;
}

__global__ __launch_bounds__(256) void k_gc_points(const long long* __restrict__ off, int64_t n, const double2* __restrict__ mm, int64_t total, orip_gcode_map g,
                                                   int2* __restrict__ xy, unsigned* __restrict__ keep, unsigned* __restrict__ pid, int* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > total) return;
    if (i == total) { keep[i] = 0; return; }
    const int64_t p = gc_path_of(off, n, i);
    const bool first = i == off[p];
    const double2 a = mm[i];
    int2 me, pv;
    bool ok = gc_step(g, a.x, a.y, me), k = true;
    if (!first) { const double2 b = mm[i - 1]; ok = gc_step(g, b.x, b.y, pv) && ok; k = pv.x != me.x || pv.y != me.y; }
    if (!ok && off[p + 1] - off[p] >= 2) atomicOr(err, 1);
    xy[i] = me; keep[i] = k ? 1u : 0u; pid[i] = (unsigned)p;
}

__global__ __launch_bounds__(256) void k_gc_paths(const long long* __restrict__ off, int64_t n, const unsigned* __restrict__ kpos, unsigned* __restrict__ pc,
                                                  unsigned* __restrict__ pk) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    unsigned cnt = 0;
    if (p < n) cnt = kpos[off[p + 1]] - kpos[off[p]];
    pc[p] = cnt >= 2 ? cnt : 0u; pk[p] = cnt >= 2 ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_gc_emit(const long long* __restrict__ off, int64_t n, int64_t total, const int2* __restrict__ xy, const unsigned* __restrict__ keep,
                                                 const unsigned* __restrict__ pid, const unsigned* __restrict__ kpos, const unsigned* __restrict__ pk,
                                                 const unsigned* __restrict__ noff, const unsigned* __restrict__ nidx, int2* __restrict__ out_pts, long long* __restrict__ out_off, int* __restrict__ out_src) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) {                                                       // offsets of the kept paths and the closing one; where each kept path came from
        if (i == n) out_off[nidx[n]] = (long long)noff[n];
        else if (pk[i]) { out_off[nidx[i]] = (long long)noff[i]; out_src[nidx[i]] = (int)i; }
    }
    if (i >= total || !keep[i]) return;
    const unsigned p = pid[i];
    if (pk[p]) out_pts[noff[p] + (kpos[i] - kpos[off[p]])] = xy[i];
}
}  // namespace

// ------------------------------------------------------------------------------------------------ the cutting passes' compaction (gc_cut.h)
__global__ __launch_bounds__(256) void k_gc_cut_compact(int64_t S, const unsigned* __restrict__ rec, const int2* __restrict__ sinfo, unsigned long long* __restrict__ cs) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > S) return;
    unsigned long long out = 0;
    if (g < S) {
        const unsigned r = rec[g], np = r & GC_CUT_NP;
        if (np) {
            bool cont = false;
            if ((r & GC_CUT_FA) && g > 0 && sinfo[g - 1].y == sinfo[g].y) { const unsigned rp = rec[g - 1]; cont = (rp & GC_CUT_NP) && (rp & GC_CUT_FB); }
            const unsigned starts = np - (cont ? 1u : 0u);
            out = ((unsigned long long)(np + starts) << 32) | starts;
        }
    }
    cs[g] = out;
}

// ------------------------------------------------------------------------------------------------ the resident list's host side (gc_convert.h)
static int gc_check_offsets(orip_ctx* c, const char* who, const int64_t* off, int64_t n) {
    if (off[0] != 0) ORIP_FAIL_AS(c, who, "offsets must start at 0");
    for (int64_t p = 0; p < n; p++) if (off[p + 1] < off[p]) ORIP_FAIL_AS(c, who, "offsets must not decrease (path %lld)", (long long)p);
    return 0;
}
int gc_mm_check(orip_ctx* c, const char* who, const int64_t* off, const double* pts_mm, int64_t n, const orip_gcode_map* map, bool others_ok, bool& resident, int64_t& total) {
    resident = !off && !pts_mm && n > 0;                    // the fitted paths orip_svg_flatten / orip_svg_fit left on the device (svg.hip)
    if (!map || !others_ok || n < 0 || (n > 0 && !off && !resident)) ORIP_FAIL_AS(c, who, "bad arguments");
    if (resident && (!c->sv_ready || n != c->sv_n)) ORIP_FAIL_AS(c, who, "%lld paths asked for, %lld fitted paths resident", (long long)n, (long long)(c->sv_ready ? c->sv_n : -1));
    if (map->W < 1 || map->H < 1 || map->W > GC_COORD_MAX || map->H > GC_COORD_MAX)
        ORIP_FAIL_AS(c, who, "target size %d x %d steps: each side must be in 1..2^30 (step coordinates are int32 on the device)", map->W, map->H);
    if (n >= INT32_MAX / 2) ORIP_FAIL_AS(c, who, "%lld paths: at most 2^30", (long long)n);         // before off[n] is looked at
    total = resident ? c->sv_total : n > 0 ? off[n] : 0;
    if (!resident && n > 0) ORIP_TRY(gc_check_offsets(c, who, off, n));
    if (total > 0 && !pts_mm && !resident) ORIP_FAIL_AS(c, who, "bad arguments");
    return 0;
}
int gc_mm_upload(orip_ctx* c, const char* who, const int64_t* off, const double* pts_mm, int64_t n, int64_t total, bool resident, long long*& d_off, double2*& d_mm) {
    if (resident) { d_off = c->sv_off.as<long long>(); d_mm = c->sv_pts.as<double2>(); return 0; }
    HIPC_AS(c, who, hipMemcpyAsync(d_off, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, LN(c).stream));
    HIPC_AS(c, who, hipMemcpyAsync(d_mm, pts_mm, (size_t)total * 16, hipMemcpyHostToDevice, LN(c).stream));
    return 0;
}
int gc_steps_check(orip_ctx* c, const char* who, const int64_t* off, const int32_t* pts, int64_t n, bool no_repeats, int64_t& total, int max_log2) {
    if (n < 0 || n > (1 << 26)) ORIP_FAIL_AS(c, who, "%lld paths: 0..2^26", (long long)n);
    if (!off != !pts) ORIP_FAIL_AS(c, who, "off and pts: both or neither");
    if (!off) {
        ORIP_TRY(gc_check_resident(c, who, n));
        total = c->gc_total;
        if (total >= (int64_t)1 << max_log2) ORIP_FAIL_AS(c, who, "%lld points: fewer than 2^%d", (long long)total, max_log2);
        return 0;
    }
    ORIP_TRY(gc_check_offsets(c, who, off, n));
    for (int64_t p = 0; p < n; p++) if (off[p + 1] - off[p] < 2) ORIP_FAIL_AS(c, who, "path %lld has fewer than two points", (long long)p);
    total = off[n];
    if (total >= (int64_t)1 << max_log2) ORIP_FAIL_AS(c, who, "%lld points: fewer than 2^%d", (long long)total, max_log2);
    for (int64_t i = 0; i < 2 * total; i++) if (pts[i] < 0 || pts[i] > GC_COORD_MAX) ORIP_FAIL_AS(c, who, "point %lld: coordinate %d outside 0..2^30", (long long)(i / 2), pts[i]);
    for (int64_t p = 0; no_repeats && p < n; p++)
        for (int64_t i = off[p] + 1; i < off[p + 1]; i++)
            if (pts[2 * i] == pts[2 * i - 2] && pts[2 * i + 1] == pts[2 * i - 1]) ORIP_FAIL_AS(c, who, "path %lld: point %lld equals the point before it", (long long)p, (long long)i);
    return 0;
}
int gc_steps_upload(orip_ctx* c, const char* who, const int64_t* off, const int32_t* pts, int64_t n, int64_t total) {
    c->gc_ready = false;
    HIPC_AS(c, who, c->gc_off.ensure((size_t)(n + 1) * 8 + 64)); HIPC_AS(c, who, c->gc_pts.ensure((size_t)total * 8 + 64));
    HIPC_AS(c, who, hipMemcpyAsync(c->gc_off.p, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, LN(c).stream));
    if (total) HIPC_AS(c, who, hipMemcpyAsync(c->gc_pts.p, pts, (size_t)total * 8, hipMemcpyHostToDevice, LN(c).stream));
    c->gc_n = n; c->gc_total = total; c->gc_ready = true;
    return 0;
}
void gc_drop(orip_ctx* c) { c->gc_n = 0; c->gc_total = 0; c->gc_ready = false; c->gc_merged = false; }
int gc_publish_empty(orip_ctx* c, const char* who) { static const int64_t zero = 0; return gc_steps_upload(c, who, &zero, nullptr, 0, 0); }
void gc_publish(orip_ctx* c, DBuf& off, DBuf& pts, int64_t n, int64_t total) { std::swap(c->gc_off, off); std::swap(c->gc_pts, pts); c->gc_n = n; c->gc_total = total; }
void gc_publish_src(orip_ctx* c, DBuf& src) { std::swap(c->gc_src, src); }
// the cutting passes' frame (gc_cut.h)
hipError_t gc_scan_u64(orip_ctx* c, unsigned long long* in, unsigned long long* out, size_t count) {
    return orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, in, out, 0ull, count, rocprim::plus<unsigned long long>(), LN(c).stream); });
}
static bool gc_same_count(const orip_ctx* c, int64_t n) { return c->gc_ready && c->gc_n == n; }      // as many as the sources name: taken for the polylines a fetch gave out
int gc_cut_empty(orip_ctx* c, const char* who, GcCut& r, bool explicit_in) {
    const bool same_count = gc_same_count(c, 0);
    if (explicit_in) { ORIP_TRY(gc_publish_empty(c, who)); if (!same_count) c->gc_merged = true; }
    r.paths = 0;
    return 0;
}
int gc_cut_intake(orip_ctx* c, const char* who, GcCut& r, const int64_t* off, const int32_t* pts, int64_t n, int64_t total, bool& sources) {
    const bool same_count = gc_same_count(c, n);                              // of the list in front of the upload
    r.paths = -1;
    if (off) ORIP_TRY(gc_steps_upload(c, who, off, pts, n, total));           // checked by the caller: from here on the input is the resident list
    if (off && !same_count) c->gc_merged = true;                              // the sources do not name these polylines
    sources = !c->gc_merged;                                                  // gc_src names the input strokes: gathered through origin by the pass
    return 0;
}
int gc_cut_ensure(orip_ctx* c, const char* who, GcCut& r, long long cap_paths, long long cap_pts) {
    HIPC_AS(c, who, r.off.ensure(((size_t)cap_paths + 1) * 8 + 64)); HIPC_AS(c, who, r.pts.ensure((size_t)cap_pts * 8 + 64));
    HIPC_AS(c, who, r.res.ensure((size_t)cap_paths * 4 + 64)); HIPC_AS(c, who, r.src.ensure((size_t)cap_paths * 4 + 64));
    return 0;
}
GcCutOut gc_cut_out(orip_ctx* c, const GcCut& r, bool sources, long long cap_pts, long long cap_paths) {
    return {r.pts.as<int2>(), r.off.as<long long>(), r.res.as<int>(), r.src.as<int>(), sources ? c->gc_src.as<int>() : nullptr, cap_pts, cap_paths};
}
void gc_cut_publish(orip_ctx* c, GcCut& r, bool sources, int64_t paths, int64_t points) {
    gc_publish(c, r.off, r.pts, paths, points);
    if (sources) gc_publish_src(c, r.src);
    r.paths = paths;
}
int gc_cut_fetch(orip_ctx* c, const char* who, const GcCut& r, const char* pass, int32_t* origin) {
    orip_enter(c);
    ORIP_LANE_AS(c, who, ORIP_LANE_CROSS);
    if (r.paths < 0) ORIP_FAIL_AS(c, who, "no result: %s has not succeeded since the last failure", pass);
    if (r.paths == 0) return 0;
    if (!origin) ORIP_FAIL_AS(c, who, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC_AS(c, who, hipMemcpyAsync(origin, r.res.p, (size_t)r.paths * 4, hipMemcpyDeviceToHost, s));
    HIPC_AS(c, who, hipStreamSynchronize(s));
    return 0;
}
int gc_check_resident(orip_ctx* c, const char* who, int64_t n) {
    if (!c->gc_ready || n != c->gc_n) ORIP_FAIL_AS(c, who, "%lld paths asked for, %lld step polylines resident", (long long)n, (long long)(c->gc_ready ? c->gc_n : -1));
    return 0;
}
int gc_check_groups(orip_ctx* c, const char* who, const int32_t* group, int64_t n, int32_t n_groups, int64_t* paths) {
    if (n_groups < 1 || n_groups > ORIP_ORDER_MAX_GROUPS) ORIP_FAIL_AS(c, who, "%d groups: 1..%d", n_groups, ORIP_ORDER_MAX_GROUPS);
    for (int64_t p = 0; group && p < n; p++) {
        if (group[p] < 0 || group[p] >= n_groups) ORIP_FAIL_AS(c, who, "path %lld: group %d of %d", (long long)p, group[p], n_groups);
        if (paths) paths[group[p]]++;
    }
    return 0;
}
int gc_check_start(orip_ctx* c, const char* who, const int32_t* start_xy, int& sx, int& sy) {
    sx = start_xy ? start_xy[0] : 0; sy = start_xy ? start_xy[1] : 0;
    if (sx < 0 || sy < 0 || sx > GC_COORD_MAX || sy > GC_COORD_MAX) ORIP_FAIL_AS(c, who, "start (%d, %d) outside 0..2^30", sx, sy);
    return 0;
}

// mm paths -> resident step polylines; *n_out paths with *total_out points remain.  off == NULL and pts_mm == NULL: the n resident fitted paths of svg.hip
extern "C" int orip_gcode_to_steps(orip_ctx* c, const int64_t* off, const double* pts_mm, int64_t n, const orip_gcode_map* map, int64_t* n_out, int64_t* total_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    gc_drop(c);                                             // the one writer that drops the list before it looks at its arguments
    bool resident; int64_t total;
    ORIP_TRY(gc_mm_check(c, __func__, off, pts_mm, n, map, n_out && total_out, resident, total));
    *n_out = 0; *total_out = 0;
    if (total >= INT32_MAX / 2) ORIP_FAIL(c, "%lld paths, %lld points: at most 2^30 of each", (long long)n, (long long)total);
    if (total == 0) return gc_publish_empty(c, __func__);
    hipStream_t s = LN(c).stream;
    long long* d_off; double2* d_mm; int2* xy; unsigned *keep, *kpos, *pid, *pc, *pk, *noff, *nidx; int* err;
    Carve L;
    L.take(d_off, resident ? 0 : (size_t)n + 1); L.take(d_mm, resident ? 0 : (size_t)total); L.take(xy, (size_t)total); L.take(keep, (size_t)total + 1); L.take(kpos, (size_t)total + 1);
    L.take(pid, (size_t)total); L.take(pc, (size_t)n + 1); L.take(pk, (size_t)n + 1); L.take(noff, (size_t)n + 1); L.take(nidx, (size_t)n + 1); L.take(err, 1);
    HIPC(c, L.commit(c->gc_tmp, 64));
    HIPC(c, c->gc_off.ensure((size_t)(n + 1) * 8 + 64)); HIPC(c, c->gc_pts.ensure((size_t)total * 8 + 64));     // the output is never larger than the input
    HIPC(c, c->gc_src.ensure((size_t)n * 4 + 64));
    HIPC(c, hipMemsetAsync(c->gc_off.p, 0, 8, s));
    ORIP_TRY(gc_mm_upload(c, __func__, off, pts_mm, n, total, resident, d_off, d_mm));
    HIPC(c, hipMemsetAsync(err, 0, 4, s));
    { ProfScope ps(c, "k_gc_points");
      hipLaunchKernelGGL(k_gc_points, dim3(cdiv(total + 1, 256)), dim3(256), 0, s, d_off, n, d_mm, total, *map, xy, keep, pid, err); }
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, keep, kpos, 0u, (size_t)total + 1, rocprim::plus<unsigned>(), s); }));
    hipLaunchKernelGGL(k_gc_paths, dim3(cdiv(n + 1, 256)), dim3(256), 0, s, d_off, n, kpos, pc, pk);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, pc, noff, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), s); }));
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, pk, nidx, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), s); }));
    { ProfScope ps(c, "k_gc_emit");
      hipLaunchKernelGGL(k_gc_emit, dim3(cdiv(std::max(total, n + 1), 256)), dim3(256), 0, s, d_off, n, total, xy, keep, pid, kpos, pk, noff, nidx, c->gc_pts.as<int2>(),
                         c->gc_off.as<long long>(), c->gc_src.as<int>()); }
    HIPC(c, hipGetLastError());
    struct { unsigned tot, cnt; int err; } h = {0, 0, 0};
    HIPC(c, hipMemcpyAsync(&h.tot, noff + n, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.cnt, nidx + n, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.err, err, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (h.err) ORIP_FAIL(c, "a path holds a coordinate that is not finite after the conversion to steps");
    c->gc_n = h.cnt; c->gc_total = h.tot; c->gc_ready = true;
    *n_out = h.cnt; *total_out = h.tot;
    return 0;
}

extern "C" int orip_gcode_steps_fetch(orip_ctx* c, int64_t* off_out, int32_t* pts_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!off_out) ORIP_FAIL(c, "bad arguments");
    if (!c->gc_ready) ORIP_FAIL(c, "no step polylines: orip_gcode_to_steps has not succeeded since the last failure");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(off_out, c->gc_off.p, (size_t)(c->gc_n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (c->gc_total && pts_out) HIPC(c, hipMemcpyAsync(pts_out, c->gc_pts.p, (size_t)c->gc_total * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}

// src_out[k] = the input path step polyline k came from
extern "C" int orip_gcode_steps_source_fetch(orip_ctx* c, int32_t* src_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!c->gc_ready) ORIP_FAIL(c, "no step polylines: orip_gcode_to_steps has not succeeded since the last failure");
    if (c->gc_merged) ORIP_FAIL(c, "the step polylines have been merged: ask for the sources before orip_gcode_merge");
    if (c->gc_n == 0) return 0;
    if (!src_out) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(src_out, c->gc_src.p, (size_t)c->gc_n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
