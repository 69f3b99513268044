// csrc/svg.hip -- the device side of svg_to_stream/svg2stream.py's first step (svg2gcode.py): the segments of an SVG (lines, quadratic and cubic Beziers in
// user units, each with the index of its 2 x 3 matrix; parsed on the host, orip/svg.py) -> polylines in raw units, their bounding box (compute_gcode_bbox,
// svg2gcode.py:111-141) and the fit onto the page with its 4-decimal rounding (scale_and_offset_gcode :144-172), all resident.  orip_gcode_to_steps takes the
// fitted paths from here when it is called without pointers, so the geometry stays on the device from the control points to the stream bytes.
//
// 1. Flatten.  One thread per segment applies the segment's matrix to its control points, x' = (a * x + c * y) + e and y' = (b * x + d * y) + f, every
//    operation on its own (_rn intrinsics; the tree builds with -ffp-contract=off), and chooses the number of pieces n from the second differences of the
//    transformed control polygon (Wang's bound): with q = the largest |Pi - 2 Pi+1 + Pi+2|^2 (dx * dx + dy * dy), k = 4 * tol and w = 1 for a quadratic, 9
//    for a cubic, n is the smallest integer >= 1 with  (n * n * k) * (n * n * k) >= w * q  -- n^2 >= |d| / (4 tol), resp. 3 |d| / (4 tol), squared so that
//    no square root decides.  A candidate comes from sqrt(); the two loops behind it settle n with that comparison alone, so the candidate's last bit is
//    irrelevant and a numpy restatement repeats n exactly.  Lines have n = 1.  An exclusive scan of n gives every segment the place of its first point.
//    One thread per output point then finds its segment by binary search and evaluates it at t = i / n by de Casteljau, each step a + (b - a) * t:
//    q_j = P_j + (P_j+1 - P_j) * t, r_j = q_j + (q_j+1 - q_j) * t, B = r_0 + (r_1 - r_0) * t.  The point i == n is the transformed end point itself, and the
//    first point of a subpath is the transformed first control point of its first segment: joints between the segments of a subpath are emitted once.
//    A curve that needs more than 2^16 pieces, a control point or matrix entry that is not finite (before or after the matrix) and a total beyond 2^30 - 1
//    points are errors; nothing is written outside its buffer for any input (every index below is bounded by the scanned counts).
// 2. Bounding box.  Min and max of x and y over the resident points: per-block reduction, then one block over the partial results.  Exact in any order.
// 3. Fit.  v' = v * s + o per axis, unfused, then what float(f"{v':.4f}") gives: the integer k nearest to the EXACT v' * 10^4, ties to even, divided by
//    10^4 in one correctly rounded division.  p = v' * 1e4 rounded, e = fma(v', 1e4, -p) is the exact rest; k = rint(p), and only when p - k is exactly
//    +-0.5 does the sign of e decide (v' = 5e-05: p is exactly 0.5, e > 0, so k = 1).  When p is no tie, e is too small to cross one.
#include "vec_common.h"
#include "sv_round.h"
#include "sv_place.h"       // k_svg_off, k_svg_first

namespace {
constexpr int SV_MAX_PIECES = 1 << 16;
constexpr int64_t SV_MAX_POINTS = (1ll << 30) - 1;        // what orip_gcode_to_steps accepts
constexpr double SV_FIT_LIMIT = 1e9;
constexpr int SV_BOX_BLOCKS = 256;

__device__ __forceinline__ double sv_lerp(double a, double b, double t) { return sv_add(a, sv_mul(sv_sub(b, a), t)); }
// |a - 2 b + c|^2 as (a - b) + (c - b), squared and summed
__device__ __forceinline__ double sv_dd2(double2 a, double2 b, double2 c) {
    const double dx = sv_add(sv_sub(a.x, b.x), sv_sub(c.x, b.x)), dy = sv_add(sv_sub(a.y, b.y), sv_sub(c.y, b.y));
    return sv_add(sv_mul(dx, dx), sv_mul(dy, dy));
}
__device__ __forceinline__ bool sv_enough(long long n, double k, double wq) { const double a = sv_mul((double)(n * n), k); return sv_mul(a, a) >= wq; }

// transformed control points of every segment and its piece count; err bit 0: not finite, bit 1: more than SV_MAX_PIECES pieces
__global__ __launch_bounds__(256) void k_svg_count(const int* __restrict__ kind, const double2* __restrict__ ctrl, const int* __restrict__ mi, const double* __restrict__ mats,
                                                   int64_t S, double tol, double2* __restrict__ tc, long long* __restrict__ cnt, int* __restrict__ err) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > S) return;
    if (s == S) { cnt[s] = 0; return; }
    const double* m = mats + 6 * (int64_t)mi[s];
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5];
    double2 P[4];
    bool fin = true;
    for (int j = 0; j < 4; j++) {
        const double2 u = ctrl[4 * s + j];
        P[j].x = sv_add(sv_add(sv_mul(a, u.x), sv_mul(c, u.y)), e);
        P[j].y = sv_add(sv_add(sv_mul(b, u.x), sv_mul(d, u.y)), f);
        fin = fin && isfinite(P[j].x) && isfinite(P[j].y);
        tc[4 * s + j] = P[j];
    }
    const int kd = kind[s];
    long long n = 1;
    if (fin && kd >= 2) {
        const double q = kd == 2 ? sv_dd2(P[0], P[1], P[2]) : fmax(sv_dd2(P[0], P[1], P[2]), sv_dd2(P[1], P[2], P[3]));
        const double wq = kd == 2 ? q : sv_mul(9.0, q), k = sv_mul(4.0, tol);
        if (!isfinite(wq)) fin = false;
        else {
            const double cand = ceil(sqrt(sqrt(wq) / k));
            n = cand >= 1.0 ? (cand <= (double)SV_MAX_PIECES + 1.0 ? (long long)cand : (long long)SV_MAX_PIECES + 1) : 1;     // a NaN candidate gives 1
            while (n > 1 && sv_enough(n - 1, k, wq)) n--;
            while (n <= SV_MAX_PIECES && !sv_enough(n, k, wq)) n++;
            if (n > SV_MAX_PIECES) { atomicOr(err, 2); n = 1; }
        }
    }
    if (!fin) { atomicOr(err, 1); n = 1; }
    cnt[s] = n;
}

__global__ __launch_bounds__(256) void k_svg_emit(const int* __restrict__ kind, const double2* __restrict__ tc, const long long* __restrict__ cnt, const long long* __restrict__ first,
                                                  int64_t S, int64_t total, double2* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    int64_t lo = -1, hi = S;                                                 // last s with first[s] <= j, -1: none
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (first[mid] <= j) lo = mid; else hi = mid; }
    if (lo < 0 || j - first[lo] >= cnt[lo]) {                                // the first point of a subpath: segment lo + 1 opens it
        out[j] = tc[4 * min(lo + 1, S - 1)];
        return;
    }
    const long long n = cnt[lo], i = j - first[lo] + 1;
    const int kd = kind[lo];
    const double2* P = tc + 4 * lo;
    if (i == n) { out[j] = P[kd <= 1 ? 1 : kd]; return; }
    const double t = (double)i / (double)n;
    double2 q0 = P[0], q1 = P[1], q2 = P[2], r;
    if (kd == 2) {
        const double2 a = make_double2(sv_lerp(q0.x, q1.x, t), sv_lerp(q0.y, q1.y, t)), b = make_double2(sv_lerp(q1.x, q2.x, t), sv_lerp(q1.y, q2.y, t));
        r = make_double2(sv_lerp(a.x, b.x, t), sv_lerp(a.y, b.y, t));
    } else {
        const double2 q3 = P[3];
        const double2 a = make_double2(sv_lerp(q0.x, q1.x, t), sv_lerp(q0.y, q1.y, t)), b = make_double2(sv_lerp(q1.x, q2.x, t), sv_lerp(q1.y, q2.y, t)),
                      c = make_double2(sv_lerp(q2.x, q3.x, t), sv_lerp(q2.y, q3.y, t));
        const double2 u = make_double2(sv_lerp(a.x, b.x, t), sv_lerp(a.y, b.y, t)), v = make_double2(sv_lerp(b.x, c.x, t), sv_lerp(b.y, c.y, t));
        r = make_double2(sv_lerp(u.x, v.x, t), sv_lerp(u.y, v.y, t));
    }
    out[j] = r;
}

// (min x, min y, max x, max y) of pts[0 .. n): nb blocks leave partial results, then one block reduces those in place into part[0 .. 4)
__global__ __launch_bounds__(256) void k_svg_box(const double2* __restrict__ pts, int64_t n, double* __restrict__ part) {
    __shared__ double sh[4][256];
    double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double2 p = pts[i];
        x0 = fmin(x0, p.x); y0 = fmin(y0, p.y); x1 = fmax(x1, p.x); y1 = fmax(y1, p.y);
    }
    sh[0][threadIdx.x] = x0; sh[1][threadIdx.x] = y0; sh[2][threadIdx.x] = x1; sh[3][threadIdx.x] = y1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[0][threadIdx.x] = fmin(sh[0][threadIdx.x], sh[0][threadIdx.x + w]); sh[1][threadIdx.x] = fmin(sh[1][threadIdx.x], sh[1][threadIdx.x + w]);
            sh[2][threadIdx.x] = fmax(sh[2][threadIdx.x], sh[2][threadIdx.x + w]); sh[3][threadIdx.x] = fmax(sh[3][threadIdx.x], sh[3][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) part[4 * blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
}
__global__ __launch_bounds__(256) void k_svg_box_final(double* __restrict__ part, int nb) {
    __shared__ double sh[4][256];
    const int t = threadIdx.x;
    for (int k = 0; k < 4; k++) sh[k][t] = t < nb ? part[4 * t + k] : (k < 2 ? INFINITY : -INFINITY);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            sh[0][t] = fmin(sh[0][t], sh[0][t + w]); sh[1][t] = fmin(sh[1][t], sh[1][t + w]);
            sh[2][t] = fmax(sh[2][t], sh[2][t + w]); sh[3][t] = fmax(sh[3][t], sh[3][t + w]);
        }
        __syncthreads();
    }
    if (t < 4) part[t] = sh[t][0];
}

__host__ __device__ __forceinline__ double sv_fit_value(double v, double s, double o) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dadd_rn(__dmul_rn(v, s), o);
#else
    volatile double m = v * s; return m + o;
#endif
}
__global__ __launch_bounds__(256) void k_svg_fit(double2* __restrict__ pts, int64_t n, double sx, double sy, double ox, double oy) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 p = pts[i];
    pts[i] = make_double2(sv_round4(sv_fit_value(p.x, sx, ox)), sv_round4(sv_fit_value(p.y, sy, oy)));
}

int sv_box(orip_ctx* c, double* box) {
    hipStream_t s = LN(c).stream;
    if (!c->sv_box_ok) {
        double* part; { Carve L; L.take(part, (size_t)4 * SV_BOX_BLOCKS); HIPC(c, L.commit(c->sv_tmp2, 64)); }
        const int nb = (int)std::min<int64_t>(SV_BOX_BLOCKS, cdiv(c->sv_total, 256));
        hipLaunchKernelGGL(k_svg_box, dim3(nb), dim3(256), 0, s, c->sv_pts.as<double2>(), c->sv_total, part);
        hipLaunchKernelGGL(k_svg_box_final, dim3(1), dim3(256), 0, s, part, nb);
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(c->sv_box, part, 32, hipMemcpyDeviceToHost, s));
        HIPC(c, hipStreamSynchronize(s));
        c->sv_box_ok = true;
    }
    memcpy(box, c->sv_box, 32);
    return 0;
}
}  // namespace

extern "C" int orip_svg_flatten(orip_ctx* c, const int32_t* kind, const double* ctrl, const int32_t* mat, int64_t n_seg, const int64_t* sub_off, int64_t n_sub,
                                const double* mats, int64_t n_mat, double tol, int64_t* total_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    c->sv_ready = false; c->sv_box_ok = false; c->sv_n = 0; c->sv_total = 0; c->sv_fitted = false; c->sv_hatched = false;
    if (!total_out || n_seg < 0 || n_sub < 0 || n_mat < 0 || (n_seg > 0 && (!kind || !ctrl || !mat || !mats || !sub_off))) ORIP_FAIL(c, "bad arguments");
    *total_out = 0;
    if (!(tol > 0.0) || !std::isfinite(tol)) ORIP_FAIL(c, "the tolerance must be a positive finite number");
    if (n_seg >= SV_MAX_POINTS || n_sub >= SV_MAX_POINTS) ORIP_FAIL(c, "%lld segments in %lld subpaths: at most 2^30 - 2 of each", (long long)n_seg, (long long)n_sub);
    if ((n_sub == 0) != (n_seg == 0)) ORIP_FAIL(c, "%lld segments in %lld subpaths", (long long)n_seg, (long long)n_sub);
    if (n_sub > 0 && (sub_off[0] != 0 || sub_off[n_sub] != n_seg)) ORIP_FAIL(c, "the subpaths' segment ranges must start at 0 and end at the segment count");
    for (int64_t p = 0; p < n_sub; p++) if (sub_off[p + 1] <= sub_off[p]) ORIP_FAIL(c, "subpath %lld holds no segment", (long long)p);
    for (int64_t i = 0; i < 6 * n_mat; i++) if (!std::isfinite(mats[i])) ORIP_FAIL(c, "matrix %lld holds an entry that is not finite", (long long)(i / 6));
    for (int64_t s = 0; s < n_seg; s++) {
        if (kind[s] < 1 || kind[s] > 3) ORIP_FAIL(c, "segment %lld: kind %d (1 line, 2 quadratic, 3 cubic)", (long long)s, kind[s]);
        if (mat[s] < 0 || mat[s] >= n_mat) ORIP_FAIL(c, "segment %lld: matrix %d of %lld", (long long)s, mat[s], (long long)n_mat);
        for (int j = 0; j < 8; j++) if (!std::isfinite(ctrl[8 * s + j])) ORIP_FAIL(c, "segment %lld holds a control point that is not finite", (long long)s);
    }
    hipStream_t s = LN(c).stream;
    HIPC(c, c->sv_off.ensure(64)); HIPC(c, hipMemsetAsync(c->sv_off.p, 0, 8, s));
    if (n_seg == 0) { HIPC(c, hipStreamSynchronize(s)); c->sv_ready = true; return 0; }
    int *d_kind, *d_mi, *err; double2 *d_ctrl, *tc; double* d_mats; long long *d_sub, *cnt, *ex, *first;
    { Carve L; L.take(d_kind, (size_t)n_seg); L.take(d_mi, (size_t)n_seg); L.take(d_ctrl, (size_t)4 * n_seg); L.take(tc, (size_t)4 * n_seg); L.take(d_mats, (size_t)6 * n_mat);
      L.take(d_sub, (size_t)n_sub + 1); L.take(cnt, (size_t)n_seg + 1); L.take(ex, (size_t)n_seg + 1); L.take(first, (size_t)n_seg); L.take(err, 1); HIPC(c, L.commit(c->sv_tmp, 64)); }
    HIPC(c, hipMemcpyAsync(d_kind, kind, (size_t)n_seg * 4, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_mi, mat, (size_t)n_seg * 4, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(d_ctrl, ctrl, (size_t)n_seg * 64, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_mats, mats, (size_t)n_mat * 48, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(d_sub, sub_off, (size_t)(n_sub + 1) * 8, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(err, 0, 4, s));
    { ProfScope ps(c, "k_svg_count");
      hipLaunchKernelGGL(k_svg_count, dim3(cdiv(n_seg + 1, 256)), dim3(256), 0, s, d_kind, d_ctrl, d_mi, d_mats, n_seg, tol, tc, cnt, err); }
    ORIP_TRY(vscan_excl<int64_t>(c, (const int64_t*)cnt, (int64_t*)ex, (size_t)n_seg + 1));
    struct { long long pieces; int err; } h = {0, 0};
    HIPC(c, hipMemcpyAsync(&h.pieces, ex + n_seg, 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.err, err, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (h.err & 1) ORIP_FAIL(c, "a control point is not finite after its matrix, or the second differences of a curve overflow");
    if (h.err & 2) ORIP_FAIL(c, "a curve needs more than 2^16 pieces at this tolerance");
    const int64_t total = (int64_t)h.pieces + n_sub;
    if (h.pieces < 0 || total > SV_MAX_POINTS) ORIP_FAIL(c, "%lld points: at most 2^30 - 1", (long long)total);
    HIPC(c, c->sv_off.ensure((size_t)(n_sub + 1) * 8 + 64)); HIPC(c, c->sv_pts.ensure((size_t)total * 16 + 64));
    hipLaunchKernelGGL(k_svg_off, dim3(cdiv(n_sub + 1, 256)), dim3(256), 0, s, d_sub, n_sub, ex, c->sv_off.as<long long>());
    hipLaunchKernelGGL(k_svg_first, dim3(cdiv(n_seg, 256)), dim3(256), 0, s, d_sub, n_sub, n_seg, ex, first);
    { ProfScope ps(c, "k_svg_emit");
      hipLaunchKernelGGL(k_svg_emit, dim3(cdiv(total, 256)), dim3(256), 0, s, d_kind, tc, cnt, first, n_seg, total, c->sv_pts.as<double2>()); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    c->sv_n = n_sub; c->sv_total = total; c->sv_ready = true;
    *total_out = total;
    return 0;
}

extern "C" int orip_svg_paths_fetch(orip_ctx* c, int64_t* off_out, double* pts_out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!off_out) ORIP_FAIL(c, "bad arguments");
    if (!c->sv_ready) ORIP_FAIL(c, "no paths: orip_svg_flatten has not succeeded since the last failure");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(off_out, c->sv_off.p, (size_t)(c->sv_n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (c->sv_total && pts_out) HIPC(c, hipMemcpyAsync(pts_out, c->sv_pts.p, (size_t)c->sv_total * 16, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}

extern "C" int orip_svg_bbox(orip_ctx* c, double* box) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!box) ORIP_FAIL(c, "bad arguments");
    if (!c->sv_ready) ORIP_FAIL(c, "no paths: orip_svg_flatten has not succeeded since the last failure");
    if (c->sv_total == 0) ORIP_FAIL(c, "no points: an empty drawing has no bounding box");
    return sv_box(c, box);
}

extern "C" int orip_svg_fit(orip_ctx* c, double sx, double sy, double ox, double oy) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!c->sv_ready) ORIP_FAIL(c, "no paths: orip_svg_flatten has not succeeded since the last failure");
    if (c->sv_total == 0) { c->sv_fitted = true; return 0; }
    // v * s + o is monotonic in v, so the box's corners bound every fitted value: a drawing outside the limit is refused before a kernel touches it
    double box[4];
    ORIP_TRY(sv_box(c, box));
    const double ext[4] = {sv_fit_value(box[0], sx, ox), sv_fit_value(box[2], sx, ox), sv_fit_value(box[1], sy, oy), sv_fit_value(box[3], sy, oy)};
    for (double v : ext) if (!(std::fabs(v) < SV_FIT_LIMIT)) ORIP_FAIL(c, "a fitted coordinate is %g: not finite, or 1e9 and beyond", v);
    hipStream_t s = LN(c).stream;
    { ProfScope ps(c, "k_svg_fit");
      hipLaunchKernelGGL(k_svg_fit, dim3(cdiv(c->sv_total, 256)), dim3(256), 0, s, c->sv_pts.as<double2>(), c->sv_total, sx, sy, ox, oy); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    c->sv_box_ok = false; c->sv_fitted = true;
    return 0;
}
