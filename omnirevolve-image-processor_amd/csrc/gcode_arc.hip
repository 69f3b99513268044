// csrc/gcode_arc.hip -- orip_gcode_flatten: the lines and circular arcs (G2 / G3) of a G-code text, parsed on the host (orip/gcode.py: parse_gcode_arcs), ->
// polylines in mm, resident exactly as orip_svg_flatten leaves its own (sv_off, sv_pts, sv_n, sv_total, sv_ready), so that orip_svg_paths_fetch,
// orip_gcode_to_steps(ctx, NULL, NULL, ...) and orip_gcode_to_steps_clip(ctx, NULL, NULL, ...) take them unchanged.  include/orip.h states the rule in full;
// tests/arc_double.py restates it in Python floats and repeats every bit.
//
// The structure is svg.hip's.  k_arc_count: one thread per segment works out the arc's radii, unit vectors, spans and depth (steps 1-3 of the rule), leaves
// them in geo / meta, counts the pieces and raises the error bits.  An exclusive scan of the counts places every segment and subpath (sv_place.h).
// k_arc_emit: one thread per output point finds its segment by binary search and computes its point alone (steps 4-5): at most 16 bisections, each a sum
// per component, one square root and two divisions.  Every operation is one _rn intrinsic; no sin, cos or atan2.  No thread writes outside the scanned
// counts for any input: every index below is bounded by them.
#include "vec_common.h"
#include "sv_round.h"
#include "sv_place.h"       // k_svg_off, k_svg_first

namespace {
constexpr int ARC_MAX_DEPTH = ORIP_ARC_MAX_DEPTH;
constexpr int64_t ARC_MAX_POINTS = (1ll << 30) - 1;       // what orip_gcode_to_steps accepts
enum { ARC_ERR_FINITE = 1, ARC_ERR_RADIUS = 2, ARC_ERR_DEPTH = 4 };
// meta[s]: the depth m in bits 0-4, the spans S (0..4) in bits 8-10, bit 16: the last joint is uB (otherwise it is the quarter turn q_S)
__device__ __forceinline__ int arc_meta(int m, int S, bool last_is_b) { return m | (S << 8) | (last_is_b ? 1 << 16 : 0); }

__device__ __forceinline__ double sv_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ double sv_sqrt(double a) { return __dsqrt_rn(a); }
__device__ __forceinline__ double sv_norm(double x, double y) { return sv_sqrt(sv_add(sv_mul(x, x), sv_mul(y, y))); }
// u turned by i quarter turns in direction dir (+1 counter-clockwise, -1 clockwise): exact, signs of zero included
__device__ __forceinline__ double2 arc_turn(double2 u, int i, int dir) {
    switch (i & 3) {
        case 1: return dir > 0 ? make_double2(-u.y, u.x) : make_double2(u.y, -u.x);
        case 2: return make_double2(-u.x, -u.y);
        case 3: return dir > 0 ? make_double2(u.y, -u.x) : make_double2(-u.y, u.x);
        default: return u;
    }
}

// steps 1-3.  geo[6 s ..]: rA, rB, uA, uB.  A line, and a segment in error, count one piece
__global__ __launch_bounds__(256) void k_arc_count(const int* __restrict__ kind, const double* __restrict__ seg, int64_t S, double tol, double* __restrict__ geo, int* __restrict__ meta,
                                                   long long* __restrict__ cnt, int* __restrict__ err) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > S) return;
    if (s == S) { cnt[s] = 0; return; }
    const double* g = seg + 6 * s;
    const double Ax = g[0], Ay = g[1], Bx = g[2], By = g[3], Cx = g[4], Cy = g[5];
    const int kd = kind[s];
    long long n = 1;
    int mt = 0, e = 0;
    double rA = 0.0, rB = 0.0; double2 uA = make_double2(0.0, 0.0), uB = uA;
    if (!(isfinite(Ax) && isfinite(Ay) && isfinite(Bx) && isfinite(By))) e = ARC_ERR_FINITE;
    else if (kd >= 2) {
        const int dir = kd == 3 ? 1 : -1;
        const double ax = sv_sub(Ax, Cx), ay = sv_sub(Ay, Cy), bx = sv_sub(Bx, Cx), by = sv_sub(By, Cy);
        rA = sv_norm(ax, ay); rB = sv_norm(bx, by);
        if (!(isfinite(Cx) && isfinite(Cy) && isfinite(rA) && isfinite(rB))) e = ARC_ERR_FINITE;
        else if (rA == 0.0 || rB == 0.0) e = ARC_ERR_RADIUS;
        else {
            uA = make_double2(sv_div(ax, rA), sv_div(ay, rA)); uB = make_double2(sv_div(bx, rB), sv_div(by, rB));
            const double r = fmax(rA, rB);
            int Sp; bool quarter, last_is_b = false;
            if (Ax == Bx && Ay == By) { Sp = 4; quarter = true; }            // a full circle: the fourth quarter turn of uA is uA
            else {
                double k = sv_sub(sv_mul(ax, by), sv_mul(ay, bx));
                if (dir < 0) k = -k;
                const double d = sv_add(sv_mul(ax, bx), sv_mul(ay, by));
                const int j = k > 0.0 ? (d > 0.0 ? 0 : 1) : k < 0.0 ? (d >= 0.0 ? 3 : 2) : (d >= 0.0 ? 0 : 2);
                const double2 q = arc_turn(uA, j, dir);
                last_is_b = !(uB.x == q.x && uB.y == q.y);
                Sp = j + (last_is_b ? 1 : 0); quarter = j >= 1;
            }
            int m = 0;
            if (Sp > 0) {
                double c = quarter ? sv_sqrt(0.5) : sv_sqrt(sv_div(sv_add(1.0, sv_add(sv_mul(uA.x, uB.x), sv_mul(uA.y, uB.y))), 2.0));
                while (!(sv_mul(r, sv_sub(1.0, c)) <= tol)) {
                    if (++m > ARC_MAX_DEPTH) break;
                    c = sv_sqrt(sv_div(sv_add(1.0, c), 2.0));
                }
            }
            if (m > ARC_MAX_DEPTH) e = ARC_ERR_DEPTH;
            else { mt = arc_meta(m, Sp, last_is_b); n = Sp > 0 ? (long long)Sp << m : 1; }      // no span left (uB is uA, yet B is not A): one piece, to B
        }
    }
    if (e) atomicOr(err, e);
    double* o = geo + 6 * s;
    o[0] = rA; o[1] = rB; o[2] = uA.x; o[3] = uA.y; o[4] = uB.x; o[5] = uB.y;
    meta[s] = mt; cnt[s] = n;
}

// steps 4-5
__global__ __launch_bounds__(256) void k_arc_emit(const int* __restrict__ kind, const double* __restrict__ seg, const double* __restrict__ geo, const int* __restrict__ meta,
                                                  const long long* __restrict__ cnt, const long long* __restrict__ first, int64_t S, int64_t total, double2* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    int64_t lo = -1, hi = S;                                                 // last s with first[s] <= j, -1: none
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (first[mid] <= j) lo = mid; else hi = mid; }
    if (lo < 0 || j - first[lo] >= cnt[lo]) {                                // the first point of a subpath: segment lo + 1 opens it
        const double* a = seg + 6 * min(lo + 1, S - 1);
        out[j] = make_double2(a[0], a[1]);
        return;
    }
    const long long N = cnt[lo], g = j - first[lo] + 1;
    const double* sg = seg + 6 * lo;
    if (g == N) { out[j] = make_double2(sg[2], sg[3]); return; }             // B as given; a line has N == 1
    const double* ge = geo + 6 * lo;
    const double rA = ge[0], rB = ge[1];
    const double2 uA = make_double2(ge[2], ge[3]), uB = make_double2(ge[4], ge[5]);
    const int mt = meta[lo], m = mt & 31, Sp = (mt >> 8) & 7, dir = kind[lo] == 3 ? 1 : -1;
    const int sp = (int)(g >> m), i = (int)(g & ((1ll << m) - 1));
    double2 uL = arc_turn(uA, sp, dir), uR = sp + 1 == Sp && (mt >> 16 & 1) ? uB : arc_turn(uA, sp + 1, dir), u = uL;
    int l = 0, h = 1 << m;
    while (i != l) {
        const int mid = (l + h) >> 1;
        const double sx = sv_add(uL.x, uR.x), sy = sv_add(uL.y, uR.y), nn = sv_norm(sx, sy);
        u = make_double2(sv_div(sx, nn), sv_div(sy, nn));
        if (i == mid) break;
        if (i < mid) { uR = u; h = mid; } else { uL = u; l = mid; }
    }
    const double t = sv_div((double)g, (double)N);
    const double rho = sv_add(rA, sv_mul(sv_sub(rB, rA), t));
    out[j] = make_double2(sv_add(sg[4], sv_mul(rho, u.x)), sv_add(sg[5], sv_mul(rho, u.y)));
}
}  // namespace

extern "C" int orip_gcode_flatten(orip_ctx* c, const int32_t* kind, const double* seg, int64_t n_seg, const int64_t* sub_off, int64_t n_sub, double tol, int64_t* total_out,
                                  int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    c->sv_ready = false; c->sv_box_ok = false; c->sv_n = 0; c->sv_total = 0; c->sv_fitted = false; c->sv_hatched = false;
    if (!total_out || !stats || n_seg < 0 || n_sub < 0 || (n_seg > 0 && (!kind || !seg || !sub_off))) ORIP_FAIL(c, "bad arguments");
    *total_out = 0; stats[0] = stats[1] = stats[2] = 0;
    if (!(tol > 0.0) || !std::isfinite(tol)) ORIP_FAIL(c, "the tolerance must be a positive finite number");
    if (n_seg >= ARC_MAX_POINTS || n_sub >= ARC_MAX_POINTS) ORIP_FAIL(c, "%lld segments in %lld subpaths: at most 2^30 - 2 of each", (long long)n_seg, (long long)n_sub);
    if ((n_sub == 0) != (n_seg == 0)) ORIP_FAIL(c, "%lld segments in %lld subpaths", (long long)n_seg, (long long)n_sub);
    if (n_sub > 0 && (sub_off[0] != 0 || sub_off[n_sub] != n_seg)) ORIP_FAIL(c, "the subpaths' segment ranges must start at 0 and end at the segment count");
    for (int64_t p = 0; p < n_sub; p++) if (sub_off[p + 1] <= sub_off[p]) ORIP_FAIL(c, "subpath %lld holds no segment", (long long)p);
    int64_t arcs = 0, full = 0;
    for (int64_t s = 0; s < n_seg; s++) {
        if (kind[s] < 1 || kind[s] > 3) ORIP_FAIL(c, "segment %lld: kind %d (1 line, 2 arc clockwise, 3 arc counter-clockwise)", (long long)s, kind[s]);
        if (kind[s] >= 2) { arcs++; full += seg[6 * s] == seg[6 * s + 2] && seg[6 * s + 1] == seg[6 * s + 3]; }
    }
    for (int64_t p = 0; p < n_sub; p++)
        for (int64_t s = sub_off[p] + 1; s < sub_off[p + 1]; s++)
            if (!(seg[6 * s] == seg[6 * s - 4] && seg[6 * s + 1] == seg[6 * s - 3])) ORIP_FAIL(c, "segment %lld does not start where its predecessor ends", (long long)s);
    hipStream_t s = LN(c).stream;
    HIPC(c, c->sv_off.ensure(64)); HIPC(c, hipMemsetAsync(c->sv_off.p, 0, 8, s));
    if (n_seg == 0) { HIPC(c, hipStreamSynchronize(s)); c->sv_ready = true; return 0; }
    int *d_kind, *meta, *err; double *d_seg, *geo; long long *d_sub, *cnt, *ex, *first;
    { Carve L; L.take(d_kind, (size_t)n_seg); L.take(meta, (size_t)n_seg); L.take(d_seg, (size_t)6 * n_seg); L.take(geo, (size_t)6 * n_seg); L.take(d_sub, (size_t)n_sub + 1);
      L.take(cnt, (size_t)n_seg + 1); L.take(ex, (size_t)n_seg + 1); L.take(first, (size_t)n_seg); L.take(err, 1); HIPC(c, L.commit(c->sv_tmp, 64)); }
    HIPC(c, hipMemcpyAsync(d_kind, kind, (size_t)n_seg * 4, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_seg, seg, (size_t)n_seg * 48, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(d_sub, sub_off, (size_t)(n_sub + 1) * 8, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(err, 0, 4, s));
    { ProfScope ps(c, "k_arc_count");
      hipLaunchKernelGGL(k_arc_count, dim3(cdiv(n_seg + 1, 256)), dim3(256), 0, s, d_kind, d_seg, n_seg, tol, geo, meta, cnt, err); }
    ORIP_TRY(vscan_excl<int64_t>(c, (const int64_t*)cnt, (int64_t*)ex, (size_t)n_seg + 1));
    struct { long long pieces; int err; } h = {0, 0};
    HIPC(c, hipMemcpyAsync(&h.pieces, ex + n_seg, 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.err, err, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (h.err & ARC_ERR_FINITE) ORIP_FAIL(c, "a coordinate or a radius is not finite");
    if (h.err & ARC_ERR_RADIUS) ORIP_FAIL(c, "an arc starts or ends on its centre: a radius of 0");
    if (h.err & ARC_ERR_DEPTH) ORIP_FAIL(c, "an arc needs more than 2^18 pieces at this tolerance");
    const int64_t total = (int64_t)h.pieces + n_sub;
    if (h.pieces < 0 || total > ARC_MAX_POINTS) ORIP_FAIL(c, "%lld points: at most 2^30 - 1", (long long)total);
    HIPC(c, c->sv_off.ensure((size_t)(n_sub + 1) * 8 + 64)); HIPC(c, c->sv_pts.ensure((size_t)total * 16 + 64));
    hipLaunchKernelGGL(k_svg_off, dim3(cdiv(n_sub + 1, 256)), dim3(256), 0, s, d_sub, n_sub, ex, c->sv_off.as<long long>());
    hipLaunchKernelGGL(k_svg_first, dim3(cdiv(n_seg, 256)), dim3(256), 0, s, d_sub, n_sub, n_seg, ex, first);
    { ProfScope ps(c, "k_arc_emit");
      hipLaunchKernelGGL(k_arc_emit, dim3(cdiv(total, 256)), dim3(256), 0, s, d_kind, d_seg, geo, meta, cnt, first, n_seg, total, c->sv_pts.as<double2>()); }
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    c->sv_n = n_sub; c->sv_total = total; c->sv_ready = true;
    *total_out = total;
    stats[0] = arcs; stats[1] = h.pieces - (n_seg - arcs); stats[2] = full;
    return 0;
}
