// csrc/vec_common.h -- interface of the building blocks the vector stages (05, 07, 08, 10, 12) share: the types and the device-inline helpers here,
// the functions and every kernel behind them in three units:
//   vector_common.hip    the rocPRIM wrappers (vscan_excl, vsort_pairs), vsrc_of, the gather family (vgather*, orip_polys_materialize), orip_runs_to_polys
//   vector_features.hip  the per-polyline features with numpy's pairwise tree (vfeatures*, vlen_order, vwalk_arcs)
//   vector_greedy.hip    the greedy nearest-neighbour order (vreorder: the brute-force kernel, the grid kernel with its asm step)
#pragma once
#include "orip_ctx.h"
#include "vec_serial.h"
#include "vsrc.h"
#include <algorithm>
#include <chrono>
#include <string>

// ---- rocPRIM wrappers (temporary storage in ctx->tmpF), on the lane's stream.  Instantiated in vector_common.hip for the types in use:
// vscan_excl<int64_t | unsigned>, vsort_pairs<unsigned | float | unsigned long long, unsigned>.  in == out is fine for the scan.
template <class T> int vscan_excl(orip_ctx* c, const T* in, T* out, size_t n);
template <class K, class V> int vsort_pairs(orip_ctx* c, const K* kin, K* kout, const V* vin, V* vout, size_t n, int begin_bit, int end_bit, bool desc = false);
template <class T>
static inline int vread(orip_ctx* c, T* host, const T* dev, size_t n = 1) {
    HIPC(c, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    return 0;
}
// ORIP_TIME08 / ORIP_TIME10 (debug): wall times of a call's phases.  Every lap waits for the lane's stream, so a timed run is not a concurrent one.
struct PhaseTimer {
    orip_ctx* c; const bool on; std::string log; std::chrono::steady_clock::time_point prev;
    PhaseTimer(orip_ctx* ctx, const char* env) : c(ctx), on(getenv(env) != nullptr), prev(std::chrono::steady_clock::now()) {}
    double lap() {          // ms since the previous lap
        if (on) hipStreamSynchronize(LN(c).stream);
        const auto t = std::chrono::steady_clock::now(); const double ms = std::chrono::duration<double, std::milli>(t - prev).count(); prev = t;
        return ms;
    }
    void tick(const char* name) { if (on) { char b[64]; snprintf(b, sizeof b, " %s %.2f", name, lap()); log += b; } }
};

// ---- per-polyline features ----
struct PolyFeat {
    int32_t x0, y0, x1, y1;     // bbox
    int32_t sx, sy, ex, ey;     // first / last point (of the OPEN view when open_view)
    int64_t n;                  // points (of the open view when open_view)
    float per;                  // numpy pairwise float32 perimeter (VF_PER) or 12:_poly_len (VF_PER_HYPOT)
    double arc;                 // cv::arcLength (closed flag given by caller), exact double sum
    uint8_t closed;             // first == last on the ORIGINAL polyline (n >= 2)
};

// polylines above ORIP_LONG_POLY points get a block for their features (vfeatures); above ORIP_LONG_CUM points a wavefront for their cumulative lengths
// (stage 08-A: k_cumlen_long2).  Stage 08's prefetch keeps the segment lengths of the polylines above ORIP_LONG_CUM (k_seglen) and takes the
// perimeters of open views above ORIP_LONG_POLY from them.
#define ORIP_LONG_POLY 192
#define ORIP_LONG_CUM 128
static_assert(ORIP_LONG_POLY >= ORIP_LONG_CUM, "every polyline whose perimeter is summed from stored segment lengths must have had them stored");
// ---- where a list's points come from (vsrc.h): explicit array or the layer's walk records ----
static inline ESrc esrc_of(const DPolys& P) { return ESrc{P.off.as<int64_t>(), reinterpret_cast<const int2*>(P.pts.p)}; }
int vsrc_of(orip_ctx* c, const DPolys& P, VSrc& out);
// runs BODY once with SRC bound to the list's point source (VSrc for a walk-coded list whose points are not expanded, else ESrc)
#define ORIP_WITH_SRC(c, P, SRC, BODY)                                                         \
    do {                                                                                       \
        if (is_coded(P)) { VSrc SRC; ORIP_TRY(vsrc_of(c, P, SRC)); BODY }                      \
        else { const ESrc SRC = esrc_of(P); BODY }                                             \
    } while (0)
// last index in [0, n) whose offset is <= v (off ascending, off[0] <= v): the polyline that holds point v of a list
__device__ __forceinline__ int64_t last_le(const int64_t* off, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (off[mid] <= v) lo = mid; else hi = mid - 1; }
    return lo;
}
// first index in the ascending a[0 .. n) whose element is > v
__device__ __forceinline__ int64_t ub_u32(const unsigned* a, int64_t n, unsigned v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { int64_t mid = (lo + hi) >> 1; if (a[mid] <= v) lo = mid + 1; else hi = mid; }
    return lo;
}
// inclusive scans over the 64 lanes of a wave in six DPP steps: sum and running maximum (stage 08-A's cumulative lengths and tail replay, the grid greedy's wide rounds)
__device__ __forceinline__ unsigned wave_incl_scan_u32(unsigned v) {
#define ORIP_DPP_ADD(ctrl, rowmask) v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rowmask, 0xf, false);
    ORIP_DPP_ADD(0x111, 0xf) ORIP_DPP_ADD(0x112, 0xf) ORIP_DPP_ADD(0x114, 0xf) ORIP_DPP_ADD(0x118, 0xf)      // row_shr 1, 2, 4, 8
    ORIP_DPP_ADD(0x142, 0xa) ORIP_DPP_ADD(0x143, 0xc)                                                          // row_bcast 15, 31
#undef ORIP_DPP_ADD
    return v;
}
__device__ __forceinline__ unsigned wave_incl_scan_max_u32(unsigned v) {                  // running maximum over the lanes, the same six DPP steps
#define ORIP_DPP_MAX(ctrl, rowmask) { const unsigned t_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rowmask, 0xf, false); v = t_ > v ? t_ : v; }
    ORIP_DPP_MAX(0x111, 0xf) ORIP_DPP_MAX(0x112, 0xf) ORIP_DPP_MAX(0x114, 0xf) ORIP_DPP_MAX(0x118, 0xf)
    ORIP_DPP_MAX(0x142, 0xa) ORIP_DPP_MAX(0x143, 0xc)
#undef ORIP_DPP_MAX
    return v;
}
// a cursor as the point getter vec_serial.h's sums take
template <class Cur> struct CurPt {
    Cur& c;
    __device__ __forceinline__ vs::IPt operator()(int64_t i) const { const int2 p = c.at(i); return vs::IPt{p.x, p.y}; }
};
// features of every polyline of a list: short ones one lane each, long ones one block each.  `what` is a mask of
enum : int {
    VF_PER = 1,             // PolyFeat::per = numpy's pairwise float32 perimeter (vec_serial.h KIND 0)
    VF_PER_HYPOT = 2,       // PolyFeat::per = 12:_poly_len, the same tree over np.hypot lengths (KIND 1; stage 12's seed)
    VF_ARC_CLOSED = 4,      // PolyFeat::arc = cv::arcLength(closed = true)
    VF_ARC_OPEN = 8,        // PolyFeat::arc = cv::arcLength(closed = false)
    VF_OPEN_VIEW = 16,      // features of the open view (_ensure_open): a closed polyline without its last point
    VF_PER_REV = 32,        // with VF_PER: per_rev[i] = the same perimeter over the REVERSED open polyline (numpy's pairwise sum depends on the order)
    VF_LEAVES_DONE = 64,    // long polylines: the leaf sums are in place (k_perim_leaves_seg), only combine them; set by vfeatures_long_seg alone
};
int vfeatures(orip_ctx* c, const DPolys& P, int what, PolyFeat* feat);
// The same for stage 08's prefetch (vector08a.hip: orip_prefetch08), which runs them in three parts around its own kernels and events, each on LN(c).stream:
// the short polylines' features and every polyline's end points (what: as vfeatures, per_rev for VF_PER_REV);
// order = the polylines longest first (kin, kout, vin: scratch of n words each); then the long polylines' perimeters in both
// directions from STORED segment lengths (seg[k] = float32 length of segment k, the bounding boxes already in feat; leaves in the lane's vtmp[VT_LEAVES]).
void vfeatures_short(orip_ctx* c, const VSrc& src, int64_t n, int what, PolyFeat* feat, float* per_rev);
int vlen_order(orip_ctx* c, const int64_t* off, int64_t n, unsigned* kin, unsigned* kout, unsigned* vin, unsigned* order);
int vfeatures_long_seg(orip_ctx* c, const VSrc& src, int64_t n, int64_t total, PolyFeat* feat, const unsigned* order, float* per_rev, const float* seg);
// cv::arcLength(closed = true) of the long contours of a list of whole walks, from the walk records (k_walk_arcs); vfeatures_short has done the short ones
void vwalk_arcs(orip_ctx* c, const VSrc& src, int64_t n, PolyFeat* feat);

// ---- descriptor-driven gather: output polyline k = src points [begin[k], begin[k]+len[k]) (reversed if rev[k]) ----
struct GatherDesc { int64_t begin; int64_t len; int32_t rev; int32_t src; };     // src: index of the source polyline (walk-coded sources are addressed by polyline, not by point)
// Builds dst (DPolys) from descriptors (device array of n descs).  lens/off scratch in ctx->tmpE.
// known_total >= 0: the caller knows the number of points selected (e.g. a permutation of the whole source list): no host read
int vgather(orip_ctx* c, const GatherDesc* d, int64_t n, const int32_t* src, DPolys& dst, int64_t known_total = -1);
// The same selection over a walk-coded source moves no points: output polyline k is a VIEW (walker.h) of the walk behind source
// polyline d[k].src -- its first d[k].len points, reversed if d[k].rev -- composed with the view the source polyline already is.
int vgather_views(orip_ctx* c, const GatherDesc* d, int64_t n, const DPolys& src, DPolys& dst, int64_t known_total = -1);
// selection out of a list of either kind
int vgather_list(orip_ctx* c, const GatherDesc* d, int64_t n, const DPolys& src, DPolys& dst, int64_t known_total = -1);

// Runs of accepted slots -> polylines: per-slot flags (bit0 accepted, bit1 sequence start) -> dst, one polyline per run of >= 2 accepted slots, in slot
// order.  A run starts at an accepted slot s when bit 1 is set, s == 0, or slot s - 1 is not accepted.  The flags are read twice, ORIP_RUN_TILE slots per
// block (16 per lane and load); everything behind that is per run, and only the points of the kept runs are fetched from the caller's point source.
// Shared by stage 08-A (slots = samples) and stage 10 (slots = cut steps); instantiated in vector_common.hip for the two sources below.
#define ORIP_RUN_TILE 4096u
struct SlotPtsI2 { const int2* p; __device__ __forceinline__ int2 at(unsigned s) const { return p[s]; } };        // stage 10: the cut steps' points, stored densely
struct SlotPtsF64 {                                                                                                // stage 08-A: the samples' float64 positions, truncated toward zero
    const double* x; const double* y;
    __device__ __forceinline__ int2 at(unsigned s) const { return make_int2((int)x[s], (int)y[s]); }
};
template <class Pts> int orip_runs_to_polys(orip_ctx* c, Pts pts, const uint8_t* sflag, unsigned n_slots, DPolys& dst);

// Greedy reorder of a whole DPolys list into dst.  kind: 7 -> 07 rules (arcLength closed seed), 8 -> 08 (_poly_perimeter seed), 10 -> 10 (arcLength open seed)
// prefetch08 (optional, stage 07 only): stage 08's parameters; orip_prefetch08 is then called right after the greedy kernel has been enqueued, with the
// features of the source list (device array; complete once the lane's event ev2 has fired -- the host no longer waits in front of the chain, so the
// prefetch's stream must).  The chain of greedy steps keeps ONE wave busy for milliseconds, so stage 08's work that does not depend on the order is issued
// to the lane's side stream from there.
int vreorder(orip_ctx* c, DPolys& src, DPolys& dst, int kind, const orip_params08* prefetch08 = nullptr);
