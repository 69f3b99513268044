// csrc/gcode_clip.hip -- --clip of gcode2stream.py / svg2stream.py: paths in mm -> step polylines CUT at a rectangle of the sheet instead of clamped to it
// (orip_gcode_to_steps_clip; the rule is stated in include/orip.h and is exact in integers).  Ours: the reference clamps (mm_to_steps / clamp_xy), which
// draws a line along the edge of the paper for every part of a drawing that leaves it.
//
// Thread i owns point i and, unless i is the first point of its path, SEGMENT i: the one from point i - 1 to point i.  The gap between two paths is
// therefore never a segment, and arrays over segments are arrays over points whose first-of-a-path entries stay zero.
//
// 1. k_cl_segments.  Both ends are converted with gc_round_mm (gc_convert.h: the arithmetic of orip_gcode_to_steps without its clamp) and checked: not
//    finite, or beyond +-2^30 after the rounding, in a path of two points or more, sets an error bit and the segment counts as empty (the call fails).
//    The part of v0 + t (v1 - v0), t in [0, 1], inside the closed rectangle is [t0, t1] with
//        t0 = max(0, entry_x, entry_y)    t1 = min(1, exit_x, exit_y)       entry / exit = num / den, den = |d| > 0 on an axis with d != 0
//    and an axis with d == 0 empties it when v lies outside.  Coordinates are in +-2^30, a rectangle bound in 0 .. 2^30: |num| <= 2^31, den <= 2^31, and
//    every comparison of two rationals is a comparison of two products of at most 2^62.  A = P(t0), B = P(t1): the coordinate of the side that was hit is
//    v -+ num, exact; the other one is v + (num * d_other) / den (|num * d_other| <= 2^62 because t <= 1), rounded through quotient and remainder --
//    floor, then + 1 iff 2 rem >= den -- since 2 num + den would not fit.  t0 = 0 gives A = v0 and t1 = 1 gives B = v1, untouched.
//    Segment i CONTINUES the stroke of segment i - 1 iff that one exists and their shared vertex, point i - 1, lies in the rectangle: that is "t1 = 1
//    there, t0 = 0 here, both non-empty".  A non-empty segment that does not continue STARTS a stroke.  Its candidates are A (only when it starts; a
//    continuing segment's A is the B before it) and B, and B is dropped when it equals A -- its predecessor among the candidates, kept or not, which is
//    all "a point equal to its predecessor is dropped" asks: a dropped point equals the last kept one.  cs[i] = (points emitted << 32) | starts.
// 2. One 64-bit exclusive scan of cs: the high word places the candidates (kpos), the low word numbers the strokes (sid).
// 3. k_cl_starts scatters the segment at which every stroke starts (sstart[ns] = total closes the list); k_cl_strokes takes a stroke's points as the
//    difference of kpos between two starts and keeps it with two points or more; a second 64-bit scan places the kept strokes' points and numbers them.
// 4. k_cl_emit writes the points, and per kept stroke its offset and the input path of its first segment.
// Six launches and the scans' own; one host synchronisation at the end, for the totals, the error bits and the three segment counts (a block sums them in
// LDS and adds once per counter).  Every index is a scan value of this call's own counts: candidates <= 2 per segment, strokes <= segments.
//
// Scratch in c->gc_tmp, free between calls: off long long[n + 1] and mm double2[total] (explicit form only), ab int4[total] = (A, B), cs and scan
// unsigned long long[total + 1], sstart unsigned[total + 1], ps and pscan unsigned long long[total + 1] = (points << 32 | kept) per stroke, ClCounters.
// Resident afterwards, as after orip_gcode_to_steps: c->gc_off, c->gc_pts, c->gc_src (orip_ctx.h states the contract; this writer checks before it drops).
#include "orip_ctx.h"
#include "gc_convert.h"

namespace {
constexpr int CL_ERR_NOT_FINITE = 1, CL_ERR_RANGE = 2;
struct ClCounters { unsigned long long inside, cut, outside; int err; };
struct ClRect { int x0, y0, x1, y1; };
typedef unsigned long long u64;

// the interval so far: t0 = n0 / d0 reached on axis a0 (-1: t0 = 0), t1 = n1 / d1 on axis a1 (-1: t1 = 1); d0, d1 > 0
struct ClT { long long n0, d0, n1, d1; int a0, a1; };
// one axis: lo <= v + t d <= hi.  false when d == 0 and v lies outside: nothing of the segment is inside.  Products are at most 2^31 * 2^31
__device__ __forceinline__ bool cl_axis(long long v, long long d, long long lo, long long hi, int axis, ClT& t) {
    if (d == 0) return v >= lo && v <= hi;
    const long long den = d > 0 ? d : -d;
    const long long ne = d > 0 ? lo - v : v - hi, nx = d > 0 ? hi - v : v - lo;          // entry = ne / den, exit = nx / den
    if (ne * t.d0 > t.n0 * den) { t.n0 = ne; t.d0 = den; t.a0 = axis; }
    if (nx * t.d1 < t.n1 * den) { t.n1 = nx; t.d1 = den; t.a1 = axis; }
    return true;
}
// v + num / den to the nearest integer, halves toward +inf; den > 0, |num| <= 2^62
__device__ __forceinline__ long long cl_round(long long v, long long num, long long den) {
    long long q = num / den, r = num % den;
    if (r < 0) { q--; r += den; }
    return v + q + (2 * r >= den ? 1 : 0);
}
// P(num / den), reached on `axis`
__device__ __forceinline__ int2 cl_point(int2 v, long long dx, long long dy, long long num, long long den, int axis) {
    if (axis == 0) return make_int2((int)(v.x + (dx > 0 ? num : -num)), (int)cl_round(v.y, num * dy, den));
    return make_int2((int)cl_round(v.x, num * dx, den), (int)(v.y + (dy > 0 ? num : -num)));
}
__device__ __forceinline__ bool cl_in(const ClRect& r, int2 v) { return v.x >= r.x0 && v.x <= r.x1 && v.y >= r.y0 && v.y <= r.y1; }

// the rounded point in int32, or the error bits of what keeps it from being one
__device__ __forceinline__ int cl_convert(const orip_gcode_map& g, double2 mm, int2& o) {
    double xf, yf;
    o = make_int2(0, 0);
    if (!gc_round_mm(g, mm.x, mm.y, xf, yf)) return CL_ERR_NOT_FINITE;
    const double top = (double)GC_COORD_MAX;
    if (xf < -top || xf > top || yf < -top || yf > top) return CL_ERR_RANGE;
    o = make_int2((int)xf, (int)yf);
    return 0;
}

__global__ __launch_bounds__(256) void k_cl_segments(const long long* __restrict__ off, int64_t n, const double2* __restrict__ mm, int64_t total, orip_gcode_map g, ClRect R,
                                                     int4* __restrict__ ab, u64* __restrict__ cs, ClCounters* cn) {
    __shared__ unsigned s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= total) {
        u64 out = 0;
        if (i < total) {
            const int64_t p = gc_path_of(off, n, i);
            const int64_t first = off[p];
            int2 v1;
            int bad = cl_convert(g, mm[i], v1);
            if (bad && off[p + 1] - first >= 2) atomicOr(&cn->err, bad);
            if (i > first) {                                                      // segment i: point i - 1 -> point i
                int2 v0;
                bad |= cl_convert(g, mm[i - 1], v0);
                int kind = 2;                                                     // 0 inside, 1 cut, 2 outside
                if (!bad) {
                    const long long dx = (long long)v1.x - v0.x, dy = (long long)v1.y - v0.y;
                    ClT t = {0, 1, 1, 1, -1, -1};
                    if (cl_axis(v0.x, dx, R.x0, R.x1, 0, t) && cl_axis(v0.y, dy, R.y0, R.y1, 1, t) && t.n0 * t.d1 <= t.n1 * t.d0) {
                        const int2 A = t.a0 < 0 ? v0 : cl_point(v0, dx, dy, t.n0, t.d0, t.a0);
                        const int2 B = t.a1 < 0 ? v1 : cl_point(v0, dx, dy, t.n1, t.d1, t.a1);
                        kind = t.a0 < 0 && t.a1 < 0 ? 0 : 1;
                        const bool continues = i - 1 > first && cl_in(R, v0);     // segment i - 1 exists and ends inside: one stroke
                        const unsigned start = continues ? 0u : 1u, nb = (A.x != B.x || A.y != B.y) ? 1u : 0u;
                        ab[i] = make_int4(A.x, A.y, B.x, B.y);
                        out = ((u64)(start + nb) << 32) | start;
                    }
                }
                atomicAdd(&s_cnt[kind], 1u);
            }
        }
        cs[i] = out;
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(threadIdx.x == 0 ? &cn->inside : threadIdx.x == 1 ? &cn->cut : &cn->outside, (u64)s_cnt[threadIdx.x]);
}

// sstart[k] = the segment at which stroke k starts; sstart[ns] = total.  ns <= total - 1, so the list fits total + 1 entries
__global__ __launch_bounds__(256) void k_cl_starts(const u64* __restrict__ cs, const u64* __restrict__ scan, int64_t total, unsigned* __restrict__ sstart) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > total) return;
    const unsigned k = (unsigned)scan[i];
    if (k > (unsigned)total) return;
    if (i == total || (cs[i] & 1u)) sstart[k] = (unsigned)i;
}
// ps[k] = (points << 32) | 1 for a stroke of two points or more, else 0; zero behind the last stroke
__global__ __launch_bounds__(256) void k_cl_strokes(const u64* __restrict__ scan, int64_t total, const unsigned* __restrict__ sstart, u64* __restrict__ ps) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > total) return;
    const unsigned ns = (unsigned)scan[total];
    u64 out = 0;
    if (k < ns && ns <= (unsigned)total) {
        const unsigned a = sstart[k], b = sstart[k + 1];
        if (a <= (unsigned)total && b <= (unsigned)total) {
            const unsigned cnt = (unsigned)(scan[b] >> 32) - (unsigned)(scan[a] >> 32);
            if (cnt >= 2) out = ((u64)cnt << 32) | 1u;
        }
    }
    ps[k] = out;
}
__global__ __launch_bounds__(256) void k_cl_emit(const long long* __restrict__ off, int64_t n, int64_t total, const int4* __restrict__ ab, const u64* __restrict__ cs,
                                                 const u64* __restrict__ scan, const unsigned* __restrict__ sstart, const u64* __restrict__ ps, const u64* __restrict__ pscan,
                                                 int64_t cap_pts, int2* __restrict__ out_pts, long long* __restrict__ out_off, int* __restrict__ out_src) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > total) return;
    const unsigned ns = (unsigned)scan[total];
    if (ns > (unsigned)total) return;
    // as stroke i: the offset of a kept stroke and the input path it came from; the closing offset
    if ((unsigned)i == ns) out_off[(unsigned)pscan[ns]] = (long long)(pscan[ns] >> 32);
    else if ((unsigned)i < ns && (ps[i] & 1u)) {
        const unsigned k = (unsigned)pscan[i];
        out_off[k] = (long long)(pscan[i] >> 32);
        out_src[k] = (int)gc_path_of(off, n, (int64_t)sstart[i]);
    }
    // as segment i: its candidates, into its stroke
    if (i == total) return;
    const u64 c = cs[i];
    const unsigned cnt = (unsigned)(c >> 32), start = (unsigned)c & 1u;
    if (!cnt) return;
    const unsigned k = (unsigned)scan[i] + start - 1u;                             // the strokes started before this segment, itself included
    if (k >= ns || !(ps[k] & 1u)) return;
    const unsigned a = sstart[k];
    if (a > (unsigned)total) return;
    int64_t at = (int64_t)(pscan[k] >> 32) + ((int64_t)(scan[i] >> 32) - (int64_t)(scan[a] >> 32));
    if (at < 0 || at + cnt > cap_pts) return;
    const int4 s = ab[i];
    if (start) out_pts[at++] = make_int2(s.x, s.y);
    if (cnt > start) out_pts[at] = make_int2(s.z, s.w);
}
}  // namespace

// include/orip.h states the rule; the clipped strokes become the resident step polylines, as orip_gcode_to_steps' result does
extern "C" int orip_gcode_to_steps_clip(orip_ctx* c, const int64_t* off, const double* pts_mm, int64_t n, const orip_gcode_map* map, const int32_t* rect, int64_t* n_out,
                                        int64_t* total_out, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    bool resident; int64_t total;
    ORIP_TRY(gc_mm_check(c, __func__, off, pts_mm, n, map, n_out && total_out && stats && rect, resident, total));
    if (rect[0] < 0 || rect[1] < 0 || rect[0] > rect[2] || rect[1] > rect[3] || rect[2] > map->W - 1 || rect[3] > map->H - 1)
        ORIP_FAIL(c, "clip rectangle [%d, %d] x [%d, %d]: must be 0 <= x0 <= x1 <= %d, 0 <= y0 <= y1 <= %d", rect[0], rect[2], rect[1], rect[3], map->W - 1, map->H - 1);
    if (total >= (int64_t)1 << 29) ORIP_FAIL(c, "%lld points: fewer than 2^29 (a cut can double the points)", (long long)total);
    gc_drop(c);                                                               // checked: from here on the resident step polylines are this call's
    *n_out = 0; *total_out = 0;
    for (int k = 0; k < 6; k++) stats[k] = 0;
    if (total == 0) return gc_publish_empty(c, __func__);
    hipStream_t s = LN(c).stream;
    long long* d_off; double2* d_mm; int4* ab; u64 *cs, *scan, *ps, *pscan; unsigned* sstart; ClCounters* cn;
    Carve L;
    L.take(d_off, resident ? 0 : (size_t)n + 1); L.take(d_mm, resident ? 0 : (size_t)total); L.take(ab, (size_t)total); L.take(cs, (size_t)total + 1); L.take(scan, (size_t)total + 1);
    L.take(sstart, (size_t)total + 1); L.take(ps, (size_t)total + 1); L.take(pscan, (size_t)total + 1); L.take(cn, 1);
    HIPC(c, L.commit(c->gc_tmp, 64));
    // at most one stroke per segment and two points per segment; total bounds the segments from above by one at least
    const int64_t cap_pts = 2 * total;
    HIPC(c, c->gc_off.ensure((size_t)(total + 1) * 8 + 64)); HIPC(c, c->gc_pts.ensure((size_t)cap_pts * 8 + 64)); HIPC(c, c->gc_src.ensure((size_t)total * 4 + 64));
    HIPC(c, hipMemsetAsync(c->gc_off.p, 0, 8, s));
    ORIP_TRY(gc_mm_upload(c, __func__, off, pts_mm, n, total, resident, d_off, d_mm));
    HIPC(c, hipMemsetAsync(cn, 0, sizeof(ClCounters), s));
    HIPC(c, hipMemsetAsync(sstart, 0xFF, ((size_t)total + 1) * 4, s));          // an entry nobody writes fails every bound check
    const ClRect R = {rect[0], rect[1], rect[2], rect[3]};
    const dim3 g1(cdiv(total + 1, 256)), b(256);
    { ProfScope ps_(c, "k_cl_segments");
      hipLaunchKernelGGL(k_cl_segments, g1, b, 0, s, d_off, n, d_mm, total, *map, R, ab, cs, cn); }
    HIPC(c, gc_scan_u64(c, cs, scan, (size_t)total + 1));
    hipLaunchKernelGGL(k_cl_starts, g1, b, 0, s, cs, scan, total, sstart);
    hipLaunchKernelGGL(k_cl_strokes, g1, b, 0, s, scan, total, sstart, ps);
    HIPC(c, gc_scan_u64(c, ps, pscan, (size_t)total + 1));
    { ProfScope ps_(c, "k_cl_emit");
      hipLaunchKernelGGL(k_cl_emit, g1, b, 0, s, d_off, n, total, ab, cs, scan, sstart, ps, pscan, cap_pts, c->gc_pts.as<int2>(), c->gc_off.as<long long>(), c->gc_src.as<int>()); }
    HIPC(c, hipGetLastError());
    struct { u64 tot; ClCounters cn; } h = {0, {0, 0, 0, 0}};
    HIPC(c, hipMemcpyAsync(&h.tot, pscan + total, 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.cn, cn, sizeof(ClCounters), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));                                         // the one sync
    if (h.cn.err & CL_ERR_NOT_FINITE) ORIP_FAIL(c, "a path holds a coordinate that is not finite after the conversion to steps");
    if (h.cn.err & CL_ERR_RANGE) ORIP_FAIL(c, "a path holds a point more than 2^30 steps off the sheet after the conversion to steps: the drawing is that far off the sheet");
    const int64_t paths = (int64_t)(h.tot & 0xFFFFFFFFu), points = (int64_t)(h.tot >> 32), segments = (int64_t)(h.cn.inside + h.cn.cut + h.cn.outside);
    if (paths > segments || points > 2 * segments || points < 2 * paths) ORIP_FAIL(c, "the strokes do not add up (internal error)");
    c->gc_n = paths; c->gc_total = points; c->gc_ready = true;
    *n_out = paths; *total_out = points;
    stats[0] = segments; stats[1] = (int64_t)h.cn.inside; stats[2] = (int64_t)h.cn.cut; stats[3] = (int64_t)h.cn.outside; stats[4] = paths; stats[5] = points;
    return 0;
}
