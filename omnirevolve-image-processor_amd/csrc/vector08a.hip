// csrc/vector08a.hip -- stage 08-A (08_dedup_layer_basic.py _virtual_draw, 08:117-183, between the two _split_small_and_taps, 08:198-216) on gfx950,
// and orip_prefetch08: the order-independent part of it, taken under stage 07's greedy chain with the same resampling kernels.
//
// Stage A (greedy virtual draw, 08:117-183) is NOT sequential on the GPU.  In the reference every sample of every
// polyline is pushed to the tail and later popped (hash add + thick-line stamp) whether or not it was accepted, so the
// stamp sequence depends only on the resampled geometry and on the processing order (perimeter, descending).  Giving
// every popped sample its global sequence number g, sample (r, j) sees exactly the stamps with g < base[r] + npop(r, j).
// The canvas therefore stores, per pixel, the SMALLEST sequence number of any capsule covering it (atomicMin), and all
// samples of all polylines of the layer are tested in parallel.  Self-collision (_PointHash, 08:68-99) is a sorted
// (polyline, cell) bucket list scanned in pop order.
// Layout: the kernels phase by phase (A0 / A7, A2, A3, A4, A5), the prefetch, then the host side: split_small (A0 / A7), one function per phase
// (a1_order .. a56_accept) and dedup08_a, which calls them in order.  This is the one unit of stage 08 that calls rocPRIM directly (the last-in scan by key of
// A3, the segmented sort of A5).
#include "vec08.h"
#include "tail_window.h"
#include <rocprim/rocprim.hpp>
#include <type_traits>
#include <vector>

namespace {

// ================================================================= A0 / A7: _split_small_and_taps (08:198-216)
template <class Src>
__global__ __launch_bounds__(128) void k_split_small08(Src src, int64_t n_polys, orip_params08 P, const PolyFeat* __restrict__ feat,
                                                        unsigned* __restrict__ is_tap, unsigned* __restrict__ is_keep, int2* __restrict__ tap_xy, GatherDesc* __restrict__ kd) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_polys) return;
    if (i == n_polys) { is_tap[i] = 0; is_keep[i] = 0; return; }
    const int64_t n = src.len(i);
    unsigned tap = 0, keep = 0;
    GatherDesc g; g.begin = src.off[i]; g.len = n; g.rev = 0; g.src = (int32_t)i;
    if (n >= 2) {
        const int32_t x0 = feat[i].x0, x1 = feat[i].x1, y0 = feat[i].y0, y1 = feat[i].y1;      // bbox from vfeatures (long polylines: block-parallel)
        double d = (double)max(x1 - x0, y1 - y0);
        if (d <= P.tap_diam && d <= P.tap_max_dim && n <= (int64_t)P.tap_max_v) {      // the vertex test is evaluated last in the reference but decides alone
            double per; float cx, cy, r;
            if constexpr (std::is_same<Src, ESrc>::value) {
                const int32_t* p = reinterpret_cast<const int32_t*>(src.pts + src.off[i]);
                per = (double)vs::pairwise_seglen_sum<0>(p, n);
                if (per <= P.tap_max_per) vs::min_enclosing_circle(p, n, cx, cy, r);
            } else {                                  // a tap candidate has at most tap_max_v <= 64 vertices (checked by the host): private copy
                auto cu = src.cur(i);
                LocalPts<decltype(cu), 64> lp; lp.load(cu, (int)n);
                per = (double)vs::pairwise_seglen_sum<0>(lp.xy, n);
                if (per <= P.tap_max_per) vs::min_enclosing_circle(lp.xy, n, cx, cy, r);
            }
            if (per <= P.tap_max_per) { tap = 1; tap_xy[i] = make_int2((int)vs::round_half_even((double)cx), (int)vs::round_half_even((double)cy)); }
        }
        if (!tap && !(d < P.min_keep)) {
            keep = 1;
            if (feat[i].closed) g.len = n - 1;      // _ensure_open
        }
    }
    is_tap[i] = tap; is_keep[i] = keep; kd[i] = g;
}
// ordered compaction by flag and exclusive scan: out[scan[i]] = in[i] wherever flag[i] (split_small: the kept descriptors, the tap centres, the kept features)
template <class T>
__global__ __launch_bounds__(256) void k_compact(const unsigned* __restrict__ flag, const unsigned* __restrict__ scan, int64_t n, const T* __restrict__ in, T* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flag[i]) out[scan[i]] = in[i];
}

// ================================================================= A2: resample (08:53-64)
struct RsInfo { int64_t n_eff; double total; unsigned m; unsigned pass; };
// sequential float32 cumsum per polyline (np.cumsum): one lane per short polyline; long polylines (k_cumlen_long2) use one
// wavefront: 64 segment lengths are computed / loaded by the lanes and summed with the roundings of the sequential chain of
// float adds (cum_window below), so every partial sum is the reference's
__device__ __forceinline__ void rs_finish(RsInfo& r, float acc, int64_t n, double step) {
    r.total = (double)acc;
    if (r.total <= step) { r.pass = 1; r.m = (unsigned)n; }
    else r.m = (unsigned)ceil(r.total / step);
    if (r.m < 2) r.m = 0;                                                             // len(S) < 2 -> nothing is drawn or stamped (08:130)
}
template <class Src>
__global__ __launch_bounds__(128) void k_cumlen(Src src, int64_t n_polys, double step, float* __restrict__ cum, RsInfo* __restrict__ info) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_polys) return;
    auto cu = src.cur(i); int64_t n = src.len(i);
    float* s = cum + src.off[i];
    RsInfo r; r.n_eff = n; r.total = 0; r.m = 0; r.pass = 0;
    const int2 pf = cu.at(0);
    auto same_as_first = [&](int64_t k) { const int2 q = cu.at(k); return q.x == pf.x && q.y == pf.y; };
    if (n >= 2 && same_as_first(n - 1)) n -= 1;         // _ensure_open inside _virtual_draw (08:127)
    r.n_eff = n;
    if (n >= 2) {
        if (n > 2 && same_as_first(n - 1)) n -= 1;    // _is_closed inside _resample_arclen (08:56)
        r.n_eff = n;
        if (n <= ORIP_LONG_CUM) {
            const CurPt<decltype(cu)> pt{cu};
            float acc = 0.f; s[0] = 0.f;
            for (int64_t k = 0; k + 1 < n; k++) { float sl = vs::seg_len_f32_p(pt, k); acc = (k == 0) ? sl : acc + sl; s[k + 1] = acc; }
            rs_finish(r, acc, n, step);
        }
    }
    info[i] = r;
}

// ---- float32 np.cumsum without the serial chain (r03).  While the running sum p stays inside one binade [2^e, 2^(e+1)) its ulp u is fixed and
// p is a multiple of u, so fl(p + d) = p + R(d) with R(d) = d rounded to a multiple of u: an INTEGER increment that does not depend on p -- except
// (i) when d lies exactly half-way between two multiples of u (round-half-even looks at p's last bit) and (ii) when the sum reaches 2^(e+1) (the ulp
// doubles).  A window of 64 lengths is therefore one integer wave scan (vec_common.h: wave_incl_scan_u32); the first lane where (i) or (ii) happens does ONE real float add from its
// neighbour's exact sum, and the lanes behind it are scanned again in the new binade.  A polyline crosses a binade ~18 times and meets a tie only
// where the low bits of a length happen to be 10..0 at the current ulp; every other window costs one scan instead of 63 dependent adds.
// State: E = biased exponent of p (0: p == 0), M = 24-bit significand; both wave-uniform.  Lengths are finite and >= 0.
__device__ __forceinline__ float cum_window(float dval, int lane, unsigned& E, unsigned& M) {
    const unsigned b = __float_as_uint(dval);
    const unsigned Ed = b >> 23, Md = Ed ? ((b & 0x7fffffu) | 0x800000u) : 0u;
    unsigned out = 0u; int first = 0;                 // lanes below `first` are final
    for (;;) {
        const int sh = (int)E - (int)Ed;
        const unsigned sc = (unsigned)(sh < 0 ? 0 : (sh > 31 ? 31 : sh));
        const unsigned rem = Md & ((1u << sc) - 1u), half = (1u << sc) >> 1;
        const bool live = lane >= first;
        const bool ev = live && (sh < 0 || (sc > 0u && rem == half));                 // d >= 2p, or a tie at this ulp
        const unsigned r = (live && sh >= 0) ? (Md >> sc) + ((sc > 0u && rem > half) ? 1u : 0u) : 0u;
        const unsigned S = wave_incl_scan_u32(r);
        const unsigned long long em = __ballot(ev || (live && M + S >= 0x1000000u));
        const int f = em ? __builtin_ctzll(em) : 64;
        if (live && lane < f) out = (E << 23) | ((M + S) & 0x7fffffu);
        if (f == 64) { M += (unsigned)__builtin_amdgcn_readlane((int)S, 63); break; }
        const unsigned Mp = M + (f > first ? (unsigned)__builtin_amdgcn_readlane((int)S, f - 1) : 0u);
        const float pprev = __uint_as_float((E << 23) | (Mp & 0x7fffffu));             // E == 0: M == 0, p == +0
        const float pnew = __fadd_rn(pprev, __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)b, f)));
        const unsigned nb = __float_as_uint(pnew);
        if (lane == f) out = nb;
        E = nb >> 23; M = E ? ((nb & 0x7fffffu) | 0x800000u) : 0u;
        first = f + 1;
        if (first == 64) break;
    }
    return __uint_as_float(out);
}
__device__ __forceinline__ float cum_state_value(unsigned E, unsigned M) { return __uint_as_float((E << 23) | (M & 0x7fffffu)); }
// ---- both reading directions of every polyline in one launch (orip_prefetch08): the reversed polyline has the same segment lengths in
// reverse order, and its float32 running sum is a second, independent serial chain -- two chains interleave in one wavefront for the
// price of one (a dependent add waits ~10 cycles for its predecessor anyway).  Forward = the polyline as split_small keeps it (opened
// when closed); reversed = all its points backwards (stage 07 never flips a closed contour, so closed ones get no reversed entry).
// cum / info of the reversed reading live `rev_off` floats / `n_polys` entries behind the forward ones.
template <class Src>
__global__ __launch_bounds__(128) void k_cumlen2(Src src, const PolyFeat* __restrict__ feat07, int64_t n_polys, double step, float* __restrict__ cum, int64_t rev_off, RsInfo* __restrict__ info) {
    // one thread per polyline AND reading direction (the first n_polys threads read forwards): the launch is a few dozen blocks whose time is the longest
    // thread's loop, so two loops in a row per thread were twice that
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= 2 * n_polys) return;
    const int64_t i = gi < n_polys ? gi : gi - n_polys; const int dir0 = gi < n_polys ? 0 : 1;
    auto cu = src.cur(i); const int64_t nfull = src.len(i);
    const bool closed = feat07[i].closed != 0;
    for (int dir = dir0; dir <= dir0; dir++) {
        int64_t n = (dir == 0 && closed && nfull > 0) ? nfull - 1 : nfull;         // the view: opened forward, whole reversed
        float* s = cum + (dir ? rev_off : 0) + src.off[i];
        auto P = [&](int64_t k) { return dir ? cu.at(nfull - 1 - k) : cu.at(k); };
        RsInfo r; r.n_eff = n; r.total = 0; r.m = 0; r.pass = 0;
        if (dir == 1 && closed) { r.n_eff = 0; info[n_polys + i] = r; continue; }
        const int2 pf = P(0);
        auto same_as_first = [&](int64_t k) { const int2 q = P(k); return q.x == pf.x && q.y == pf.y; };
        if (n >= 2 && same_as_first(n - 1)) n -= 1;         // _ensure_open inside _virtual_draw (08:127)
        r.n_eff = n;
        if (n >= 2) {
            if (n > 2 && same_as_first(n - 1)) n -= 1;    // _is_closed inside _resample_arclen (08:56)
            r.n_eff = n;
            if (n <= ORIP_LONG_CUM) {
                float acc = 0.f; s[0] = 0.f;
                int2 a = P(0);
                for (int64_t k = 0; k + 1 < n; k++) {
                    const int2 b = P(k + 1);
                    float dx = (float)b.x - (float)a.x, dy = (float)b.y - (float)a.y; float qx = dx * dx, qy = dy * dy; const float sl = sqrtf(qx + qy);
                    acc = (k == 0) ? sl : acc + sl; s[k + 1] = acc; a = b;
                }
                rs_finish(r, acc, n, step);
            }
        }
        info[dir ? n_polys + i : i] = r;
    }
}
// lane j <- lane j + 1 of v; lane 63 <- `last` (the successor of a window's last point is the first point of the next window)
__device__ __forceinline__ int2 lane_succ(const int2 v, const int2 last, int lane) {
    int2 r;
    r.x = __builtin_amdgcn_update_dpp(0, v.x, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
    r.y = __builtin_amdgcn_update_dpp(0, v.y, 0x130, 0xf, 0xf, true);
    if (lane == 63) r = last;
    return r;
}
// One wavefront reads one long polyline in one direction: slot-th of n_slots waves of that direction, longest polylines first (ord).
// seg != nullptr (orip_prefetch08): the float32 length of every segment is already there (k_seglen), so a reading costs 4 bytes per segment instead of
// turning (polyline, index) into a point again (~25 instructions; the launches are bound by instruction issue).
template <class Src>
__device__ __forceinline__ void cumlen_long_wave(const Src& src, int64_t n_polys, double step, float* __restrict__ cum, int64_t rev_off, RsInfo* __restrict__ info,
                                                 const unsigned* __restrict__ ord, const bool rev, const float* __restrict__ seg, int64_t slot, int64_t n_slots, const int lane) {
    for (int64_t rr = slot; rr < n_polys; rr += n_slots) {
        const int64_t i = ord[rr];
        RsInfo r = info[rev ? n_polys + i : i];
        if (r.n_eff <= ORIP_LONG_CUM) continue;
        auto cu = src.cur(i); const int64_t nfull = src.len(i);
        float* s = cum + (rev ? rev_off : 0) + src.off[i];
        const int64_t ns = r.n_eff - 1;                                             // segments; points 0 .. ns of this reading
        const float* sg = seg ? seg + src.off[i] : nullptr;                         // sg[k]: segment k of the FORWARD polyline, k < nfull - 1
        const bool from_seg = sg != nullptr;
        float acc = 0.f; unsigned cE = 0u, cM = 0u;
        if (lane == 0) s[0] = 0.f;
        // A turn is 4 windows of 64 segment lengths.  Every point is fetched ONCE: the far end of segment k is the point in the next lane, the far end of a
        // window's last segment the first point of the next window, of a turn's last segment one extra point.  The points (or stored lengths) of the
        // next turn are requested before this turn's sums run.
        auto P = [&](int64_t k) { return cu.at(rev ? nfull - 1 - k : k); };
        auto request = [&](int64_t base, int2 (&p)[5], float (&fl)[4]) {
            if (from_seg) {
#pragma unroll
                for (int w = 0; w < 4; w++) { const int64_t k = base + 64 * w + lane; fl[w] = k < ns ? sg[rev ? nfull - 2 - k : k] : 0.f; }
            } else {
#pragma unroll
                for (int w = 0; w < 4; w++) { const int64_t k = base + 64 * w + lane; p[w] = k <= ns ? P(k) : make_int2(0, 0); }
                p[4] = base + 256 <= ns ? P(base + 256) : make_int2(0, 0);
            }
        };
        auto lengths = [&](int64_t base, const int2 (&p)[5], const float (&fl)[4], float (&sl)[4]) {
            if (from_seg) {
#pragma unroll
                for (int w = 0; w < 4; w++) sl[w] = fl[w];
                return;
            }
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int64_t k = base + 64 * w + lane;
                const int2 nx0 = w < 3 ? make_int2(__builtin_amdgcn_readlane(p[w + 1].x, 0), __builtin_amdgcn_readlane(p[w + 1].y, 0)) : p[4];
                const int2 b2 = lane_succ(p[w], nx0, lane);
                float dx = (float)b2.x - (float)p[w].x, dy = (float)b2.y - (float)p[w].y; float qx = dx * dx, qy = dy * dy;
                const float L = sqrtf(qx + qy);                                        // seg_len_f32
                sl[w] = k < ns ? L : 0.f;                                              // beyond the last segment of this reading: +0
            }
        };
        int2 rp[5]; float rf[4] = {0.f, 0.f, 0.f, 0.f}; float cur[4];
        request(0, rp, rf); lengths(0, rp, rf, cur);
        for (int64_t base = 0; base < ns; base += 256) {
            request(base + 256, rp, rf);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int64_t k = base + 64 * w + lane;
                const float pv = cum_window(cur[w], lane, cE, cM); acc = cum_state_value(cE, cM);
                if (k < ns) s[k + 1] = pv;
            }
            lengths(base + 256, rp, rf, cur);
        }
        if (lane == 0) { rs_finish(r, acc, r.n_eff, step); info[rev ? n_polys + i : i] = r; }
    }
}
template <class Src>
__global__ __launch_bounds__(64) void k_cumlen_long2(Src src, int64_t n_polys, double step, float* __restrict__ cum, int64_t rev_off, RsInfo* __restrict__ info, const unsigned* __restrict__ ord,
                                                     int dir0, const float* __restrict__ seg) {
    cumlen_long_wave<Src>(src, n_polys, step, cum, rev_off, info, ord, ((blockIdx.y + (unsigned)dir0) & 1u) != 0, seg, blockIdx.x, gridDim.x, threadIdx.x);
}
// orip_prefetch08: float32 length of EVERY segment of the long polylines (seg[off[i] + k] = |P(k + 1) - P(k)|, k < len(i) - 1) and the bounding box of their open
// views (points [0, bb[i].n); bb[i] holds the first point's box on entry: k_poly_features), fully parallel: a wave takes 64 windows of 64 consecutive points
// of the FLAT point list, advancing by 63, so the far end of a lane's segment is the point in the next lane and every lane's cursor stays on consecutive
// points of (mostly) one polyline.  Both readings' cumulative lengths then run side by side from these lengths (one launch) instead of
// the reversed reading behind the forward one, and so do the perimeter leaves (k_perim_leaves_seg).
template <class Src>
__global__ __launch_bounds__(256) void k_seglen(Src src, int64_t n_polys, int64_t total, float* __restrict__ seg, PolyFeat* __restrict__ bb) {
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (63 * 64);
    if (base >= total) return;                                 // (the whole wave)
    int64_t g = base + lane;
    int64_t i = 0;
    { const int64_t gg = g < total ? g : total - 1; int64_t hi = n_polys - 1;        // polyline of the lane's first point: the last i with off[i] <= g
      while (i < hi) { const int64_t mid = (i + hi + 1) >> 1; if (src.off[mid] <= gg) i = mid; else hi = mid - 1; } }
    int64_t o0 = src.off[i], o1 = src.off[i + 1];
    auto cu = src.cur(i);
    bool is_long = o1 - o0 > ORIP_LONG_CUM;
    int64_t vn = is_long ? bb[i].n : 0; if (vn <= ORIP_LONG_POLY) vn = 0;             // box wanted for points [0, vn) of this polyline
    int bx0 = 0x7fffffff, bx1 = -0x7fffffff, by0 = 0x7fffffff, by1 = -0x7fffffff; bool has = false;
    for (int t = 0; t < 64 && base + 63 * t < total; t++, g += 63) {
        const bool valid = g < total;
        if (valid && g >= o1) {                                // the lane enters another polyline (rare: the long ones hold thousands of points)
            if (has) { atomicMin(&bb[i].x0, bx0); atomicMax(&bb[i].x1, bx1); atomicMin(&bb[i].y0, by0); atomicMax(&bb[i].y1, by1); }
            bx0 = by0 = 0x7fffffff; bx1 = by1 = -0x7fffffff; has = false;
            do { i++; o0 = o1; o1 = src.off[i + 1]; } while (g >= o1);
            cu = src.cur(i); is_long = o1 - o0 > ORIP_LONG_CUM;
            vn = is_long ? bb[i].n : 0; if (vn <= ORIP_LONG_POLY) vn = 0;
        }
        const bool on = valid && is_long;
        int2 p = make_int2(0, 0);
        if (on) p = cu.at(g - o0);
        const int2 q = lane_succ(p, make_int2(0, 0), lane);
        if (on && lane < 63) {
            if (g + 1 < o1) { float dx = (float)q.x - (float)p.x, dy = (float)q.y - (float)p.y; float qx = dx * dx, qy = dy * dy; seg[g] = sqrtf(qx + qy); }     // seg_len_f32
            if (g - o0 < vn) { bx0 = min(bx0, p.x); bx1 = max(bx1, p.x); by0 = min(by0, p.y); by1 = max(by1, p.y); has = true; }
        }
    }
    if (__all(i == __shfl(i, 0, 64))) {                        // the usual case: one polyline under the whole wave at the end
        for (int o = 32; o > 0; o >>= 1) { bx0 = min(bx0, __shfl_xor(bx0, o, 64)); bx1 = max(bx1, __shfl_xor(bx1, o, 64)); by0 = min(by0, __shfl_xor(by0, o, 64)); by1 = max(by1, __shfl_xor(by1, o, 64)); }
        if (lane == 0 && bx0 <= bx1) { atomicMin(&bb[i].x0, bx0); atomicMax(&bb[i].x1, bx1); atomicMin(&bb[i].y0, by0); atomicMax(&bb[i].y1, by1); }
    } else if (has) { atomicMin(&bb[i].x0, bx0); atomicMax(&bb[i].x1, bx1); atomicMin(&bb[i].y0, by0); atomicMax(&bb[i].y1, by1); }
}
// any_out: set when a sampled polyline reaches beyond the canvas (its samples lie inside the box of its points): only then can a sample be
// off-canvas, and only then does "the previous in-canvas sample" (k_capprev) differ from "the previous sample"
__global__ __launch_bounds__(256) void k_rank_counts(const RsInfo* __restrict__ info, const unsigned* __restrict__ ord, int64_t n, unsigned* __restrict__ mr,
                                                      const PolyFeat* __restrict__ feat, int W, int H, unsigned* __restrict__ any_out, unsigned* __restrict__ redo) {
    int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= n) redo[r] = 0u;                                 // the n + 1 redo flags of A3 (A08::redo)
    if (r < n) {
        const unsigned i = ord[r]; const unsigned m = info[i].m;
        mr[r] = m;
        if (m) { const PolyFeat f = feat[i]; if (f.x0 < 0 || f.y0 < 0 || f.x1 >= W || f.y1 >= H) atomicOr(any_out, 1u); }
    }
    if (r == n) mr[r] = 0;
}
// One record per sample.  sx, sy: the float64 position; dprev: distance to the predecessor on the same polyline; rank: the polyline, in processing order.  (What a surviving
// sample contributes to the cleaned line is its position truncated to integers: orip_runs_to_polys takes it from sx, sy, for the survivors only.)
// pxy: the rounded pixel and one flag.  Inside the canvas (W, H <= 16383) x sits in bits 0-13, y in bits 16-29, and ORIP_PXY_FIRST (bit 15) is set on the first
// sample of its polyline; bits 14, 30 and 31 are zero.  Off the canvas the word is ORIP_PXY_OUT (all ones) and carries neither a pixel nor the flag: every
// consumer tests the sentinel first, then takes the coordinates with pxy_x / pxy_y.
// Sloc: the sum of dprev from the first sample of g's polyline -- or of g's 1024-sample block of k_samples (ORIP_SMP_BLOCK), whichever comes later -- up to g.
#define ORIP_PXY_OUT 0xffffffffu
#define ORIP_PXY_FIRST 0x8000u
#define ORIP_SMP_BLOCK 1024u
__device__ __forceinline__ int pxy_x(unsigned p) { return (int)(p & 0x3fffu); }
__device__ __forceinline__ int pxy_y(unsigned p) { return (int)((p >> 16) & 0x3fffu); }
struct SampleArrs { double* sx; double* sy; double* dprev; unsigned* pxy; unsigned* rank; double* Sloc; };
// rank (polyline) and segment of sample g, as k_samples needs them.  Both are monotone in g, so the values of the first sample of a
// 256-sample block and of the next block bound the searches of every sample in between: k_sample_hints does the two full binary
// searches once per block, k_samples only searches between the hints (mostly zero to a few steps instead of ~28 dependent loads).
__device__ __forceinline__ int64_t sample_rank(const unsigned* __restrict__ sbase, const RsInfo* __restrict__ info, const unsigned* __restrict__ ord, int64_t lo, int64_t hi, unsigned g) {
    while (lo < hi) { int64_t mid = (lo + hi) >> 1; if (sbase[mid] <= g) lo = mid + 1; else hi = mid; }      // first rank in [lo, hi) whose base is > g
    int64_t r = lo - 1;
    while (info[ord[r]].m == 0) r--;
    return r;
}
__device__ __forceinline__ float sample_t(unsigned j, double step) {
    float t0 = 0.0f, t1 = (float)(0.0 + step), delta = __fsub_rn(t1, t0);
    return j == 0 ? t0 : (j == 1 ? t1 : __fadd_rn(t0, __fmul_rn((float)j, delta)));
}
// searchsorted(s, t, 'right') - 1 on s[0..n_eff), clipped to [0, n_eff-2], given klo <= result <= khi
__device__ __forceinline__ int64_t sample_seg(const float* __restrict__ s, int64_t n_eff, double t, int64_t klo, int64_t khi) {
    int64_t lo = klo + 1, hi = khi + 2;
    while (lo < hi) { int64_t mid = (lo + hi) >> 1; if ((double)s[mid] <= t) lo = mid + 1; else hi = mid; }
    int64_t k = lo - 1; if (k < 0) k = 0; if (k > n_eff - 2) k = n_eff - 2;
    return k;
}
__global__ __launch_bounds__(256) void k_sample_hints(const int64_t* __restrict__ off /* where polyline i's cumulative lengths start in cum */, const float* __restrict__ cum, const RsInfo* __restrict__ info, const unsigned* __restrict__ ord,
                                                       const unsigned* __restrict__ sbase, int64_t n_rank, unsigned MS, double step, unsigned nb, int2* __restrict__ hints) {
    unsigned b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const unsigned g = b * 256u;
    int64_t r = sample_rank(sbase, info, ord, 0, n_rank, g);
    unsigned i = ord[r]; RsInfo ri = info[i];
    int64_t k = 0;
    if (!ri.pass) k = sample_seg(cum + off[i], ri.n_eff, (double)sample_t(g - sbase[r], step), -1, ri.n_eff - 2);
    hints[b] = make_int2((int)r, (int)k);
}
// LDS slot of a block's s-th staged sample.  A producer thread t writes samples 4t .. 4t + 3, so a wave's write of 8-byte values would fall on 8 banks' worth of
// addresses (threads t, t + 8, ... on the same bank), of 4-byte values on 16.  Exchanging the four slots of a thread by bits of t spreads them over all banks at
// no cost in space; the consumers' consecutive reads stay consecutive within every group of four.
__device__ __forceinline__ unsigned smp_slot8(unsigned s) { return s ^ ((s >> 5) & 3u); }      // t >> 3
__device__ __forceinline__ unsigned smp_slot4(unsigned s) { return s ^ ((s >> 6) & 3u); }      // t >> 4
// one step of a segmented inclusive wave scan of (f, a): f = a segment starts at or before this lane within the lanes combined so far, a = the sum since then.
// Lanes the DPP pattern leaves out receive (0, +0.0), the identity.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void wave_seg_step(double& a, unsigned& f) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(a), CTRL, ROWMASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(a), CTRL, ROWMASK, 0xf, false);
    const unsigned pf = (unsigned)__builtin_amdgcn_update_dpp(0, (int)f, CTRL, ROWMASK, 0xf, false);
    if (!f) a = __dadd_rn(__hiloint2double(hi, lo), a);
    f |= pf;
}
template <class Src>
__global__ __launch_bounds__(256) void k_samples(Src src, const int64_t* __restrict__ cumoff, const float* __restrict__ cum,
                                                  const RsInfo* __restrict__ info, const unsigned* __restrict__ ord, const unsigned* __restrict__ sbase, int64_t n_rank,
                                                  unsigned MS, double step, int W, int H, SampleArrs A,
                                                  const int2* __restrict__ hints, unsigned nhb, unsigned long long* __restrict__ pixbits, int Wq, unsigned* __restrict__ firstseq) {
    // FOUR consecutive samples per thread.  A sample costs a chain of ~18 dependent loads (rank, polyline, a bisection of its cumulative lengths, the
    // segment's end points), and with one sample per thread the kernel sat at 1.5 TB/s with every wave slot taken.  Consecutive samples of a polyline
    // lie a few segments apart (8 px of arc length against segments of 2 .. 3 px), so the second to fourth find their segment with ONE round of eight
    // independent loads from where the previous one stood.
    // The threads leave position and polyline of their samples in LDS; after the barrier thread t takes the block's samples t, t + 256, t + 512, t + 768, derives
    // the rest of the record (distance to the predecessor, pixel) from the staged positions and stores it: every store instruction of a wave
    // writes 64 consecutive elements (stored straight from the producers it wrote 64 elements at a stride of four).
    // Last, the block scans its 1024 distances by polyline (Sloc, see SampleArrs): k_tail_par forms its tail sums from them, no pass over the samples in between.
    constexpr int S = 4;
    constexpr unsigned NS = 256 * S;
    static_assert(NS == ORIP_SMP_BLOCK, "k_tail_par takes a block of k_samples for 1024 samples");
    __shared__ double shx[NS], shy[NS], shp[2], swa[4];    // swa, swf: sum and flag of each wave's 256 samples (the scan)
    __shared__ unsigned swf[4];            // [smp_slot8(s)]: sample s of the block; shp: the predecessor of sample 0
    __shared__ unsigned shr[NS];                           // [smp_slot4(s)]: its rank, bit 31: first sample of its polyline
    const unsigned g0 = (blockIdx.x * 256 + threadIdx.x) * S;
    if (g0 < MS) {
        const unsigned hb = g0 >> 8;                       // hints: rank and segment of every 256th sample (k_sample_hints)
        const int2 h0 = hints[hb];
        const bool last = hb + 1 == nhb;
        const int2 h1 = last ? make_int2((int)n_rank - 1, 0) : hints[hb + 1];
        int64_t r = sample_rank(sbase, info, ord, h0.x + 1, (int64_t)h1.x + 1, g0);      // sbase[h0.x] <= g0 already
        unsigned i = ord[r]; unsigned j = g0 - sbase[r];
        auto cu = src.cur(i); const float* s = cum + cumoff[i];
        RsInfo ri = info[i];
        int64_t kprev = -2;                                // segment of the previous sample of this polyline taken by this thread (-2: none)
        const unsigned j0 = j;
        // position of sample jj of the current polyline, its segment known to lie in [klo, khi]
        auto pos_at = [&](int64_t k, double t, double& ox, double& oy) {
            double sk = (double)s[k], sk1 = (double)s[k + 1];
            double u = __ddiv_rn(__dsub_rn(t, sk), fmax(1e-6, __dsub_rn(sk1, sk)));
            double a = __dsub_rn(1.0, u);
            const int2 p0 = cu.at(k), p1 = cu.at(k + 1);
            ox = __dadd_rn(__dmul_rn((double)(float)p0.x, a), __dmul_rn((double)(float)p1.x, u));
            oy = __dadd_rn(__dmul_rn((double)(float)p0.y, a), __dmul_rn((double)(float)p1.y, u));
        };
#pragma unroll 1
        for (int u = 0; u < S; u++) {
            const unsigned g = g0 + (unsigned)u;
            if (g >= MS) break;
            if (u > 0 && j >= ri.m) {                      // the polyline is used up: on to the next one that has samples
                do { r++; i = ord[r]; ri = info[i]; } while (ri.m == 0);
                j = 0; cu = src.cur(i); s = cum + cumoff[i]; kprev = -2;
            }
            double x, y;
            if (ri.pass) { const int2 q = cu.at(j); x = (double)(float)q.x; y = (double)(float)q.y; }
            else {
                const double t = (double)sample_t(j, step);
                int64_t k;
                if (kprev < -1) {
                    const bool first = u == 0;
                    k = sample_seg(s, ri.n_eff, t, (first && r == h0.x) ? h0.y : -1, (first && !last && r == h1.x) ? h1.y : ri.n_eff - 2);
                } else {
                    // searchsorted(s, t, 'right') - 1, clipped, from the previous sample's segment on: eight lengths per round
                    k = kprev < 0 ? 0 : kprev;
                    const int64_t kmax = ri.n_eff - 2;
                    while (k < kmax) {
                        float v[8];
#pragma unroll
                        for (int q = 0; q < 8; q++) v[q] = (k + 1 + q <= kmax + 1) ? s[k + 1 + q] : __int_as_float(0x7f800000);
                        int cnt = 0; bool run = true;
#pragma unroll
                        for (int q = 0; q < 8; q++) { run = run && ((double)v[q] <= t); cnt += run ? 1 : 0; }
                        k += cnt;
                        if (cnt < 8) break;
                    }
                    if (k > kmax) k = kmax;
                }
                kprev = k;
                pos_at(k, t, x, y);
            }
            const unsigned ls = threadIdx.x * S + (unsigned)u;
            shx[smp_slot8(ls)] = x; shy[smp_slot8(ls)] = y;
            shr[smp_slot4(ls)] = (unsigned)r | (j == 0 ? 0x80000000u : 0u);
            j++;
        }
        if (j0 > 0 && threadIdx.x == 0) {                  // the block's first sample continues a polyline: its predecessor, computed again
            // (the loop above has moved on: look the polyline of sample g0 up again)
            int64_t r2 = sample_rank(sbase, info, ord, h0.x + 1, (int64_t)h1.x + 1, g0);
            const unsigned i2 = ord[r2]; cu = src.cur(i2); s = cum + cumoff[i2]; ri = info[i2];
            double qx, qy;
            if (ri.pass) { const int2 q = cu.at(j0 - 1); qx = (double)(float)q.x; qy = (double)(float)q.y; }
            else { const double t = (double)sample_t(j0 - 1, step); pos_at(sample_seg(s, ri.n_eff, t, -1, ri.n_eff - 2), t, qx, qy); }
            shp[0] = qx; shp[1] = qy;
        }
    }
    __syncthreads();
    const unsigned b0 = blockIdx.x * NS;
    double dd[S] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < S; u++) {
        const unsigned ls = threadIdx.x + 256u * (unsigned)u, g = b0 + ls;
        if (g >= MS) break;
        const unsigned at = smp_slot8(ls);
        const double x = shx[at], y = shy[at];
        const unsigned rw = shr[smp_slot4(ls)];
        // distance to the predecessor on the same polyline, exactly as the tail bookkeeping evaluates it (08:141,147)
        double d = 0.0;
        if (!(rw >> 31)) { const unsigned before = smp_slot8(ls ? ls - 1u : 0u); d = vs::norm2_f64(x - (ls ? shx[before] : shp[0]), y - (ls ? shy[before] : shp[1])); }
        A.dprev[g] = d; dd[u] = d;
        A.sx[g] = x; A.sy[g] = y; A.rank[g] = rw & 0x7fffffffu;
        const long long xi = vs::round_half_even(x), yi = vs::round_half_even(y);
        const bool in = xi >= 0 && yi >= 0 && xi < W && yi < H;
        A.pxy[g] = in ? ((unsigned)xi | ((unsigned)yi << 16) | ((rw >> 31) ? ORIP_PXY_FIRST : 0u)) : ORIP_PXY_OUT;
        if (pixbits && in) {       // the canvas is read at sample pixels only (k_caps_stamp_bits): mark the pixel, give it its "never stamped" value
            unsigned long long* wp = &pixbits[(size_t)yi * Wq + (xi >> 6)]; const unsigned long long bit = 1ULL << (xi & 63);
            if (!(*wp & bit) && !(atomicOr(wp, bit) & bit)) firstseq[(size_t)yi * W + xi] = 0xffffffffu;      // whoever sets the bit initialises the pixel: one write per distinct pixel, not per sample
        }
    }
    // ---- Sloc: segmented inclusive scan of the block's distances; a segment starts at the first sample of a polyline (whose distance is 0).  The distances take
    // the place of the staged x once every thread has read its positions; thread t then owns samples 4t .. 4t + 3 again (the producers' layout): four serial
    // steps, a wave scan of the threads' sums, the four waves' sums in order.  Any summation order serves (k_tail_par has the argument); this one is fixed.
    __syncthreads();
#pragma unroll
    for (int u = 0; u < S; u++) shx[smp_slot8(threadIdx.x + 256u * (unsigned)u)] = dd[u];      // (beyond MS: 0)
    __syncthreads();
    const unsigned l0 = threadIdx.x * S;
    double v[S]; unsigned f[S];
#pragma unroll
    for (int q = 0; q < S; q++) { v[q] = shx[smp_slot8(l0 + q)]; f[q] = (b0 + l0 + q < MS) ? shr[smp_slot4(l0 + q)] >> 31 : 0u; }
    double wa = v[0]; unsigned wf = f[0];
#pragma unroll
    for (int q = 1; q < S; q++) { wa = f[q] ? v[q] : __dadd_rn(wa, v[q]); wf |= f[q]; }
    wave_seg_step<0x111, 0xf>(wa, wf); wave_seg_step<0x112, 0xf>(wa, wf); wave_seg_step<0x114, 0xf>(wa, wf); wave_seg_step<0x118, 0xf>(wa, wf);      // row_shr 1, 2, 4, 8
    wave_seg_step<0x142, 0xa>(wa, wf); wave_seg_step<0x143, 0xc>(wa, wf);                                                                              // row_bcast 15, 31
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 63) { swa[wv] = wa; swf[wv] = wf; }
    // (wa, wf) of the lane before: what precedes this thread's samples inside the wave
    double ea = __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(wa), 0x138 /* wave_shr:1 */, 0xf, 0xf, false),
                                 __builtin_amdgcn_update_dpp(0, __double2loint(wa), 0x138, 0xf, 0xf, false));
    const unsigned ef = (unsigned)__builtin_amdgcn_update_dpp(0, (int)wf, 0x138, 0xf, 0xf, false);
    __syncthreads();
    if (!ef) {                                             // no polyline starts in the wave before this thread: the waves before it count too
        double ca = 0.0;
        for (int k = 0; k < wv; k++) ca = swf[k] ? swa[k] : __dadd_rn(ca, swa[k]);
        ea = __dadd_rn(ca, ea);
    }
#pragma unroll
    for (int q = 0; q < S; q++) { ea = f[q] ? v[q] : __dadd_rn(ea, v[q]); v[q] = ea; }
    const unsigned gs = b0 + l0;
    if (gs + S <= MS) { double2* o = reinterpret_cast<double2*>(A.Sloc + gs); o[0] = make_double2(v[0], v[1]); o[1] = make_double2(v[2], v[3]); }
    else { for (int q = 0; q < S; q++) if (gs + q < MS) A.Sloc[gs + q] = v[q]; }
}

// ================================================================= A3: tail simulation (08:139-155)
// The tail length is a float64 running sum with data-dependent pops: strictly sequential per polyline.
// ---- the sequential simulation, replayed.  k_tail_par leaves for every sample the head the queue WOULD have if every comparison were
// decided by exact arithmetic; the reference decides them with a float64 running sum whose roundings depend on the whole history of pushes
// and pops.  Given the heads, that history is a fixed list of operations (+d[j], then -d[h] for every popped h), and its value after every
// operation is a prefix sum with SEQUENTIAL rounding -- which 64 lanes evaluate as 63 wave-shifted adds (lane i is final after step i).
// So a wavefront replays 64 operations at a time instead of deciding one comparison per
// ~400 cycles, then checks the predicted heads against the reference's loop conditions with the running values it now has (after the last
// pop: not > T; before it: > T).  Samples up to the first one that fails the check are final; that one is decided by the plain loop, and
// the replay goes on from there with heads that can only have moved forward (running maximum).  Whatever the prediction was, a sample
// is only ever committed when the reference's own conditions hold on the reference's own running value: the result is the sequential one.
__device__ __forceinline__ double dpp_shr1_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// inclusive scan of increment pairs over the wave (tw_compose is associative, the earlier lanes' pair goes first); lanes a DPP pattern leaves out receive (0, 0),
// the identity.  The same six steps as wave_incl_scan_u32.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void wave_tw_step(TwInc& f) {
    auto sh = [](long long x) -> long long {
        const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)x & 0xffffffffull), CTRL, ROWMASK, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)x >> 32), CTRL, ROWMASK, 0xf, false);
        return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    };
    TwInc p; p.ev = sh(f.ev); p.od = sh(f.od);
    f = tw_compose(p, f);
}
__device__ __forceinline__ void wave_incl_scan_tw(TwInc& f) {
    wave_tw_step<0x111, 0xf>(f); wave_tw_step<0x112, 0xf>(f); wave_tw_step<0x114, 0xf>(f); wave_tw_step<0x118, 0xf>(f);      // row_shr 1, 2, 4, 8
    wave_tw_step<0x142, 0xa>(f); wave_tw_step<0x143, 0xc>(f);                                                                    // row_bcast 15, 31
}
// `only` (k_tail_par's marks): a polyline is replayed from its first sample to its last unsure one and no further -- the samples behind it keep k_tail_par's
// heads, which are the reference's (the argument stands at k_tail_par).  Without it (ORIP_TAIL_SEQ) every polyline is replayed to its end.
// dbg (ORIP_TAIL_DBG only): {rounds, samples committed by rounds, samples decided by the plain loop, rounds in the integer form}, added to once per polyline.
__global__ __launch_bounds__(64) void k_tail_replay(const unsigned* __restrict__ sbase, int64_t n_rank, double T, SampleArrs A, unsigned* __restrict__ npop, const unsigned* __restrict__ only,
                                                    unsigned long long* __restrict__ dbg) {
    constexpr unsigned C = 1024u, RM = 2u * C - 1u;          // distances of the current chunk of C samples and of the one before it stay in LDS
    __shared__ double ops[64], rr[64];
    __shared__ double Dl[2 * C];
    __shared__ unsigned NPl[C];
    const int lane = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_rank; r += gridDim.x) {
        const unsigned stop = only ? only[r] : 0xffffffffu;      // 1 + the last unsure sample
        if (!stop) continue;
        const unsigned b = sbase[r], e = sbase[r + 1];
        if (e <= b) continue;
        const double* D = A.dprev + b; unsigned* NP = npop + b;
        const unsigned m = e - b, me = min(m, stop);          // samples me .. m - 1 are read (distances, predictions) and never written
        unsigned head = 0; double racc = 0.0;
        unsigned j0 = 0, cb = 0;
        unsigned n_rounds = 0, n_round_smp = 0, n_plain = 0, n_exact = 0;
        // one memory round trip per chunk: 32 independent loads per lane in flight, then the LDS writes (a load inside the rounds below
        // would cost the lone wave a round trip per 64 operations: most of the kernel's time)
        auto fill = [&](unsigned c0) {
            double td[16]; unsigned tn[16];
#pragma unroll
            for (int u = 0; u < 16; u++) { const unsigned idx = c0 + (unsigned)lane + 64u * u; td[u] = D[idx < m ? idx : m - 1u]; tn[u] = NP[idx < m ? idx : m - 1u]; }
#pragma unroll
            for (int u = 0; u < 16; u++) { const unsigned idx = c0 + (unsigned)lane + 64u * u; Dl[idx & RM] = td[u]; NPl[idx & (C - 1u)] = tn[u]; }
        };
        auto dist = [&](unsigned idx) -> double { return (idx + C >= cb && idx < cb + C) ? Dl[idx & RM] : D[idx]; };      // [cb - C, cb + C) is in LDS
        // the plain loop for one sample (08:139-155), every lane the same
        auto plain = [&](unsigned s) {
            if (s > head) racc = __dadd_rn(racc, dist(s));
            while (head <= s && racc > T) { head++; if (head <= s) racc = __dsub_rn(racc, dist(head)); else racc = 0.0; }
            if (lane == 0) NP[s] = head;
            n_plain++;
        };
        fill(0);
        __syncthreads();
        while (j0 < me) {
            if (j0 >= cb + C) { __syncthreads(); cb += C; fill(cb); __syncthreads(); }
            const unsigned s = j0 + (unsigned)lane; const bool valid = s < me && s < cb + C;
            unsigned hp = valid ? NPl[s & (C - 1u)] : 0u;
            hp = hp > head ? hp : head;
            hp = wave_incl_scan_max_u32(hp);                                               // heads never move back: running maximum (DPP steps: a ds_bpermute
                                                                                           // round trip per step was a quarter of the round)
            unsigned prevh = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hp, 0x138 /* wave_shr:1 */, 0xf, 0xf, true); if (lane == 0) prevh = head;
            const unsigned np = hp - prevh;
            const unsigned inc = valid ? 1u + np : 0u;
            unsigned off = wave_incl_scan_u32(inc);
            const unsigned long long fitm = __ballot(valid && off <= 64u);                 // (off is increasing over the valid lanes: a prefix)
            const int m_fit = __popcll(fitm);
            if (m_fit == 0) { plain(j0); j0++; continue; }                                 // a sample with more than 63 pops: the plain loop
            const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)off, m_fit - 1);
            off -= inc;                                                                    // exclusive
            if (lane < m_fit) {
                ops[off] = s > prevh ? dist(s) : 0.0;                                      // the push adds nothing to an empty queue
                for (unsigned t = 0; t < np; t++) ops[off + 1u + t] = -dist(prevh + 1u + t);
            }
            __syncthreads();
            const double v = (unsigned)lane < total ? ops[lane] : 0.0;
            // The running values after every operation.  First the integer form (tail_window.h): inside the binade of racc an operation is an increment of
            // racc / ulp that depends on nothing but the parity of the value it meets, so the window is one scan of increment pairs; it holds when every
            // partial sum stays strictly inside the binade.  Otherwise (the first windows of a polyline, a tail length at a power of two) the real additions:
            // 63 wave-shifted adds, lane i final after step i.
            double pre; bool exact = false;
            { int fe; long long fP;
              if (tw_frame(racc, fe, fP)) {
                  TwInc f; const bool fine = tw_inc(v, fe, f);
                  wave_incl_scan_tw(f);
                  const long long S = tw_apply(fP, f);
                  exact = !__ballot((unsigned)lane < total && !(fine && tw_inside(S)));
                  pre = tw_value(S, fe);                                                   // (lanes at and beyond `total` are never read)
              } }
            if (!exact) {
                const double d = lane == 0 ? __dadd_rn(racc, v) : v;
                pre = d;
#pragma unroll
                for (int q = 1; q < 64; q++) pre = __dadd_rn(dpp_shr1_f64(pre), d);
            } else n_exact++;
            rr[lane] = pre;
            __syncthreads();
            bool bad = false;
            if (lane < m_fit) {
                const double after = rr[off + np];
                bad = after > T || (np > 0u && !(rr[off + np - 1u] > T)) || hp > s;     // (a head beyond its own sample would be the emptied queue: plain loop)
            }
            const unsigned long long badm = __ballot(bad);
            const int ncommit = badm ? __ffsll((long long)badm) - 1 : m_fit;
            if (lane < ncommit) NP[s] = hp;
            if (ncommit > 0) {
                head = (unsigned)__builtin_amdgcn_readlane((int)hp, ncommit - 1);
                const unsigned last_op = (unsigned)__builtin_amdgcn_readlane((int)(off + np), ncommit - 1);
                racc = rr[last_op];
            }
            __syncthreads();
            j0 += (unsigned)ncommit; n_rounds++; n_round_smp += (unsigned)ncommit;
            if (badm) { plain(j0); j0++; }
        }
        if (dbg && lane == 0) { atomicAdd(&dbg[0], (unsigned long long)n_rounds); atomicAdd(&dbg[1], (unsigned long long)n_round_smp); atomicAdd(&dbg[2], (unsigned long long)n_plain); atomicAdd(&dbg[3], (unsigned long long)n_exact); }
        __syncthreads();
    }
}

// Parallel form of the same simulation.  After sample j is pushed the queue holds samples head..j and tail_len is the sum of the
// distances D[head+1..j]; the pops leave the smallest head with that sum <= tail_len_px (the sums shrink as head grows and a head
// never moves back because D >= 0), found by binary search.
// The sum comes from the block-local prefix sums k_samples leaves (Sloc: from the polyline's first sample or from the first sample of the 1024-sample block,
// whichever is later).  With j in block K and h on the same polyline:
//   h in block K too:   Sloc[j] - Sloc[h]                                      (both count from the same sample)
//   h in block K' < K:  Sloc[j] + (L[K-1] + L[K-2] + ... + L[K']) - Sloc[h]     L[k] = Sloc of block k's last sample: blocks K' .. K-1 lie inside the
//                                                                               polyline from h on, so L[k] is block k's whole sum (block K' counts from where h's
//                                                                               Sloc does).  The L are added in this order, from K-1 down.
// The window in LDS (the 256 sums before the tail block + its own) is brought into block K's frame once: an entry of block K-1 has L[K-1] taken off.
// The reference compares a float64 running sum with its own rounding history.  Here a distance reaches the compared value through fewer than 64 additions:
// at most 16 inside a Sloc (4 serial per thread, 6 levels of the wave scan, 2 wave sums, 1 to join them, and the 3 serial ones of the wave sums' own threads), 1 per
// block sum L, of which at most ORIP_TAIL_BLOCKS = 32 are taken, 2 for the difference -- and every partial sum is checked to stay below 2^22 px.  An addition
// errs by at most ulp(2^22) / 2 = 4.7e-10 px, so the value is within 3e-8 px of the real sum, as is the reference's (2 ulp(256) per push / pop over < 2^20 samples):
// a comparison that clears the threshold by more than ORIP_TAIL_EPS is the reference's decision, whatever the order of summation.
// Any sample that is closer marks its polyline, so does one whose search would go back over more than ORIP_TAIL_BLOCKS block sums, and marked polylines are
// redone by the sequential simulation (k_tail_replay) from the exact distances: the rounding of these sums decides which polylines are redone, never a result.
// The mark is redo[r] = 1 + the local index of the polyline's LAST unsure sample (0: none), and the replay stops behind that sample.  A sure sample j with
// head h here has sum(h+1..j) <= T - EPS and, for h > b, sum(h..j) > T + EPS in real numbers, up to 3e-8.  The reference enters j with the head h' it left at
// j - 1, and h' <= h: to have passed h it would have needed its running value over h+1..j-1 above T, but that sum is no larger than sum(h+1..j) <= T - EPS and
// the reference's value lies within 3e-8 of it WHATEVER pops and pushes came before (that bound is over the history's length, not its content).  At j it then
// pops while its value over head+1..j exceeds T: every head below h gives a sum >= sum(h..j) > T + EPS, so it pops; at h the sum is <= T - EPS, so it stops.
// The reference's head at a sure sample is h, also where an unsure sample before it left the reference's head one ahead of the parallel one (h' = h, no pop
// at j, against one pop here: the same head, and only heads are kept).  So behind the last unsure sample the npop written here are the reference's.
#define ORIP_TAIL_EPS 1e-6
#define ORIP_TAIL_BLOCKS 32u
__global__ __launch_bounds__(256) void k_tail_par(const unsigned* __restrict__ sbase, const unsigned* __restrict__ rank, const double* __restrict__ Sloc, unsigned MS, double T,
                                                   unsigned* __restrict__ npop, unsigned* __restrict__ redo, unsigned* __restrict__ dbg_first) {
    __shared__ double win[512];
    const unsigned g0 = blockIdx.x * 256, w0 = g0 >= 256 ? g0 - 256 : 0;      // window = samples w0 .. g0 + 255
    const unsigned KB = g0 / ORIP_SMP_BLOCK, B0 = KB * ORIP_SMP_BLOCK;         // the tail block lies inside block KB of k_samples, which starts at sample B0
    const double lastprev = w0 < B0 ? Sloc[B0 - 1] : 0.0;                     // (w0 < B0: the tail block is the first of block KB and the 256 before it the end of block KB - 1)
    for (unsigned t = threadIdx.x; t < 512; t += 256) {
        const unsigned idx = w0 + t;
        win[t] = (idx < MS && idx < g0 + 256) ? (idx < B0 ? Sloc[idx] - lastprev : Sloc[idx]) : 0.0;
    }
    __syncthreads();
    unsigned g = g0 + threadIdx.x;
    if (g >= MS) return;
    const unsigned r = rank[g], b = sbase[r];
    const double Sj = Sloc[g];
    bool unsure = !(Sj + (b < B0 ? lastprev : 0.0) < 4194304.0) || (g - b) >= (1u << 20);
    // tail(p) = sum of the distances of samples p + 1 .. g, for b <= p <= g.  Below the window: the block sums between p's block and KB, kept while the
    // search moves back (kc: the block reached, acc: L[KB-1] + ... + L[kc]).
    unsigned kc = KB; double acc = 0.0;
    auto tail = [&](unsigned p) -> double {
        if (p >= w0) return Sj - win[p - w0];
        const unsigned kb = p / ORIP_SMP_BLOCK;
        if (KB - kb > ORIP_TAIL_BLOCKS) { unsure = true; return __longlong_as_double(0x7ff0000000000000LL); }      // too far back for the error bound: "does not fit", the replay decides
        if (kb > kc) { kc = KB; acc = 0.0; }
        while (kc > kb) { kc--; acc += Sloc[kc * ORIP_SMP_BLOCK + (ORIP_SMP_BLOCK - 1u)]; }
        const double up = Sj + acc;
        if (!(up < 4194304.0)) unsure = true;
        return up - Sloc[p];
    };
    // smallest h in [b, g] with tail(h) <= T.  The tail covers a few dozen samples, so the answer almost always lies in the block's LDS
    // window; otherwise gallop back through global memory, then bisect.
    unsigned lo = b, hi = g;                 // answer in [lo, hi]; hi satisfies (tail(g) = 0 <= T)
    const unsigned wlo = max(b, w0);         // first index of my polyline inside the window
    if (wlo == b || !(tail(wlo) <= T)) {
        if (wlo > b) lo = wlo + 1;           // wlo fails: answer in (wlo, g]
        else if (tail(b) <= T) hi = b;       // the whole prefix fits
        while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (tail(mid) <= T) hi = mid; else lo = mid + 1; }
    } else {
        hi = wlo;                            // wlo still satisfies: continue below the window
        for (unsigned stepb = 1; hi > b; stepb <<= 1) {
            const unsigned p = (hi - b > stepb) ? hi - stepb : b;
            if (tail(p) <= T) { hi = p; if (p == b) break; } else { lo = p + 1; break; }
        }
        while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (tail(mid) <= T) hi = mid; else lo = mid + 1; }
    }
    const unsigned h = lo;
    if (!(tail(h) <= T - ORIP_TAIL_EPS)) unsure = true;
    if (h > b && !(tail(h - 1) > T + ORIP_TAIL_EPS)) unsure = true;
    npop[g] = h - b;
    if (unsure) {
        atomicMax(&redo[r], 1u + (g - b));                    // (k_rank_counts left 0)
        if (dbg_first) atomicMin(&dbg_first[r], g - b);       // ORIP_TAIL_DBG only
    }
}
// previous in-canvas sample of the same polyline (the far end of the capsule stamped when sample j is popped, 08:151-155); -1: none, -2: j is off-canvas
// lastin[g] = 1 + index of the last in-canvas sample at or before g inside its polyline (0: none): a max-scan by polyline
struct IncIndex {       // (the sentinel has every bit set, the first-sample flag included: an on-canvas word never equals it)
    const unsigned* pxy;
    __device__ unsigned operator()(unsigned g) const { return pxy[g] != ORIP_PXY_OUT ? g + 1u : 0u; }
};
__global__ __launch_bounds__(256) void k_capprev(const unsigned* __restrict__ sbase, unsigned MS, SampleArrs A, const unsigned* __restrict__ lastin, int* __restrict__ capprev) {
    unsigned g = blockIdx.x * 256 + threadIdx.x;
    if (g >= MS) return;
    if (A.pxy[g] == ORIP_PXY_OUT) { capprev[g] = -2; return; }
    const unsigned b = sbase[A.rank[g]];
    const unsigned l = g > b ? lastin[g - 1] : 0u;
    capprev[g] = l ? (int)(l - 1u - b) : -1;
}

// ================================================================= A4: capsule de-duplication + min-sequence stamping
__device__ __forceinline__ unsigned long long cap_key(int x0, int y0, int x1, int y1) {
    unsigned long long a = ((unsigned long long)(unsigned)x0 << 14) | (unsigned)y0, b = ((unsigned long long)(unsigned)x1 << 14) | (unsigned)y1;
    if (b < a) { unsigned long long t = a; a = b; b = t; }
    return ((a << 28) | b) + 1ULL;     // 0 is the empty marker
}
__device__ __forceinline__ unsigned long long hash64(unsigned long long x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33; return x; }
// one 16-byte slot per capsule: key and first sequence number arrive in one memory sector (the table is far larger than the caches and
// every probe is a random access: two arrays meant two sectors per probe)
struct __attribute__((aligned(16))) CapSlot { unsigned long long key; unsigned val; unsigned pad; };
// Also clears the four counters of A4 / A5 (LaneFlags has the argument for each).
__global__ __launch_bounds__(256) void k_caps_init(CapSlot* __restrict__ tab, unsigned long long tsize, LaneFlags* __restrict__ fl) {
    unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { fl->caps_overflow = 0; fl->caps_distinct = 0u; fl->accept_survivors = 0u; fl->accept_work = 0ull; }
    if (i < tsize) reinterpret_cast<uint4*>(tab)[i] = make_uint4(0u, 0u, 0xffffffffu, 0u);
}
// CP: capprev is given (some sample is off the canvas).  Without it every sample is on the canvas, the capsule of sample g runs from sample g - 1, and it has
// one unless g is the first sample of its polyline -- which its own pxy word says (ORIP_PXY_FIRST): two independent loads and the table, no rank or base.
//
// The set in LDS.  A probe whose key is in the table with a smaller sample index reads the slot and leaves, and on a retraced path that is nearly every
// probe; the repeats are close together in sample order (consecutive laps of one walk are contiguous).  So a workgroup owns a RANGE of `chunks` * 1024
// consecutive samples, goes through it in ascending chunks of 1024 and keeps in LDS the keys it has seen: `smask` + 1 slots of a 64-bit key (0: empty, as in
// the table) and the smallest sample index of that key in the range, open addressing over at most ORIP_CAPSSET_PROBES slots, the slot index from the top bits of
// hash64(key) (the table index takes the low ones).  Per chunk: (1) every live sample finds its key or claims an empty slot (atomicCAS) and takes the minimum
// of the slot's index with its own g (atomicMin); one that meets neither within the bound is "not in the set"; one barrier; (2) a sample goes to the
// table if it is not in the set or if the slot's index is its own -- the probe loop as it was.  Exact: the table has to end up with the minimum g per key.
// Indices ascend with the chunks, so the first occurrence of a key in the range fixes the slot's index for good, it alone of the range's occurrences can be
// the global minimum, and it reaches the table; so does every occurrence that did not fit.  Slots only ever fill up (nothing is evicted), so all occurrences
// of a key walk the same slots to the same end: one slot per key, or none.  Within a chunk the atomicMin and the barrier decide, not the winner of the CAS,
// who can be the later of two.  A later chunk's atomicMin cannot lower an index (its g are larger), so phase 2 of one chunk may run beside phase 1 of the
// next: one barrier per chunk.  Barrier rule (kmeans02.hip): the loop's bounds come from blockIdx.x, `chunks` and MS alone, samples beyond MS are dead lanes.
constexpr int ORIP_CAPSSET_PROBES = 4;
constexpr int ORIP_CAPSSET_SHIFT = 52;      // the top 12 bits of the hash: up to 4096 slots
template <bool CP>
__global__ __launch_bounds__(256) void k_caps_insert(SampleArrs A, const unsigned* __restrict__ sbase, const int* __restrict__ capprev, unsigned MS,
                                                      unsigned chunks, unsigned smask,
                                                      CapSlot* tab, unsigned long long tmask, int max_probe, int* __restrict__ overflow) {
    // Four samples per thread, a chunk's 1024 samples apart by 256: with one sample per thread the kernel waits for its chain of dependent loads one after the
    // other (1 TB/s of the card's 8 with every wave slot full); four independent chains per thread keep four times as many loads in flight.  With capprev the
    // chain is rank -> base -> pixels -> slot, without it pixels -> slot.
    constexpr int S = 4;
    extern __shared__ unsigned long long caps_set[];
    unsigned long long* skey = caps_set; unsigned* sval = reinterpret_cast<unsigned*>(caps_set + (smask + 1u));
    for (unsigned i = threadIdx.x; i <= smask; i += 256) { skey[i] = 0ULL; sval[i] = 0xffffffffu; }
    __syncthreads();
    const unsigned long long first = (unsigned long long)blockIdx.x * chunks * 1024ull;       // < MS: the grid is cdiv(MS, chunks * 1024)
    const unsigned long long left = (unsigned long long)MS - first;
    const unsigned nch = left < chunks * 1024ull ? (unsigned)((left + 1023ull) >> 10) : chunks;
    // the pixel words of a chunk; without capprev they are two independent loads, issued one chunk ahead (in front of the barrier of the chunk before)
    auto pixels = [&](unsigned ch, unsigned (&pa)[S], unsigned (&pb)[S], bool (&on)[S]) {
        unsigned g[S];
#pragma unroll
        for (int u = 0; u < S; u++) { g[u] = (unsigned)first + ch * 1024u + threadIdx.x + 256u * u; on[u] = ch < nch && g[u] < MS; pa[u] = 0; pb[u] = 0; }
        if constexpr (CP) {
            unsigned bb[S]; int cp[S];
#pragma unroll
            for (int u = 0; u < S; u++) bb[u] = on[u] ? A.rank[g[u]] : 0u;
#pragma unroll
            for (int u = 0; u < S; u++) if (on[u]) bb[u] = sbase[bb[u]];
#pragma unroll
            for (int u = 0; u < S; u++) { cp[u] = on[u] ? capprev[g[u]] : -1; on[u] = cp[u] >= 0; }
#pragma unroll
            for (int u = 0; u < S; u++) if (on[u]) pa[u] = A.pxy[bb[u] + cp[u]], pb[u] = A.pxy[g[u]];      // both on the canvas (cp >= 0): packed pixels
        } else {
#pragma unroll
            for (int u = 0; u < S; u++) if (on[u]) { pb[u] = A.pxy[g[u]]; pa[u] = g[u] ? A.pxy[g[u] - 1u] : 0u; }
        }
    };
    unsigned npa[S], npb[S]; bool non[S];
    pixels(0, npa, npb, non);
    for (unsigned ch = 0; ch < nch; ch++) {
        unsigned g[S]; bool on[S]; unsigned long long key[S], h[S]; int ss[S];
#pragma unroll
        for (int u = 0; u < S; u++) {
            g[u] = (unsigned)first + ch * 1024u + threadIdx.x + 256u * u; key[u] = 0; h[u] = 0; ss[u] = -1;
            on[u] = non[u]; if constexpr (!CP) on[u] = on[u] && !(npb[u] & ORIP_PXY_FIRST);
            if (on[u]) key[u] = cap_key(pxy_x(npa[u]), pxy_y(npa[u]), pxy_x(npb[u]), pxy_y(npb[u]));
        }
        pixels(ch + 1, npa, npb, non);          // (past the range: no load)
        // ---- 1: into the set
#pragma unroll
        for (int u = 0; u < S; u++) {
            if (!on[u]) continue;
            const unsigned long long hs = hash64(key[u]);
            h[u] = hs & tmask;
            unsigned i = (unsigned)(hs >> ORIP_CAPSSET_SHIFT) & smask;
            for (int p = 0; p < ORIP_CAPSSET_PROBES; p++, i = (i + 1u) & smask) {
                const unsigned long long old = atomicCAS(&skey[i], 0ULL, key[u]);
                if (old == 0ULL || old == key[u]) { atomicMin(&sval[i], g[u]); ss[u] = (int)i; break; }
            }
        }
        __syncthreads();
        // ---- 2: the first occurrence in the range, and whatever the set had no room for, to the table
#pragma unroll
        for (int u = 0; u < S; u++) on[u] = on[u] && (ss[u] < 0 || sval[ss[u]] == g[u]);
        uint4 sl[S];
#pragma unroll
        for (int u = 0; u < S; u++) sl[u] = on[u] ? *reinterpret_cast<const uint4*>(&tab[h[u]]) : make_uint4(0, 0, 0, 0);      // first probes of all four in flight together
#pragma unroll
        for (int u = 0; u < S; u++) {
            if (!on[u]) continue;
            uint4 s = sl[u]; unsigned long long hh = h[u];
            for (int probe = 0;; probe++) {
                if (probe >= max_probe) { *overflow = 1; break; }      // table too small for the number of distinct capsules: the host retries larger
                if (probe) s = *reinterpret_cast<const uint4*>(&tab[hh]);      // key and value in one 16-byte load (every probe reads another slot)
                unsigned long long cur = ((unsigned long long)s.y << 32) | s.x;
                if (cur == 0) { unsigned long long old = atomicCAS(&tab[hh].key, 0ULL, key[u]); if (old == 0 || old == key[u]) cur = key[u]; else cur = old; }
                if (cur == key[u]) { if (s.z > g[u]) atomicMin(&tab[hh].val, g[u]); break; }    // the minimum only decreases: a stale read can only cost a useless atomic
                hh = (hh + 1) & tmask;
            }
        }
    }
}

// The canvas is only ever READ at the pixels of samples (k_accept_pre: "was my pixel stamped before my own pops?"), and those are a thin
// set: the rounded sample positions, i.e. pixels on the paths.  k_samples sets one bit per sample pixel in a bit plane of the canvas
// (12.5 MB, cache-resident) and gives those pixels their "never stamped" value; a capsule then visits the words of the plane its box
// covers and tests / stamps only the set bits -- ~100 pixels instead of the ~1800 of its box, and no 400 MB clear of the canvas.
__global__ __launch_bounds__(256) void k_caps_stamp_bits(const CapSlot* __restrict__ tab, unsigned long long tsize, int rad, unsigned* __restrict__ firstseq, int W, int H,
                                                          const unsigned long long* __restrict__ pixbits, int Wq, unsigned* __restrict__ n_distinct) {
    const int lane = threadIdx.x & 63;
    const long long r2 = (long long)rad * rad;
    unsigned long long wave = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = ((unsigned long long)gridDim.x * 256) >> 6;
    unsigned mine = 0;
    for (unsigned long long s0 = wave * 64; s0 < tsize; s0 += nwaves * 64) {
        const uint4 sl = (s0 + lane < tsize) ? reinterpret_cast<const uint4*>(tab)[s0 + lane] : make_uint4(0u, 0u, 0u, 0u);
        unsigned long long k = ((unsigned long long)sl.y << 32) | sl.x;
        unsigned v = sl.z;
        unsigned long long occ = __ballot(k != 0);
        mine += (unsigned)__popcll(occ);
        while (occ) {
            int src = __ffsll((long long)occ) - 1; occ &= occ - 1;
            unsigned long long kk = __shfl(k, src, 64) - 1ULL; unsigned seq = __shfl(v, src, 64);
            unsigned long long a = kk >> 28, b = kk & ((1ULL << 28) - 1);
            int x0 = (int)(a >> 14), y0 = (int)(a & 16383), x1 = (int)(b >> 14), y1 = (int)(b & 16383);
            int bx0 = max(0, min(x0, x1) - rad), bx1 = min(W - 1, max(x0, x1) + rad), by0 = max(0, min(y0, y1) - rad), by1 = min(H - 1, max(y0, y1) + rad);
            const int w0 = bx0 >> 6, nw = (bx1 >> 6) - w0 + 1, bh = by1 - by0 + 1;
            for (int i = lane; i < nw * bh; i += 64) {
                const int y = by0 + i / nw, wq = w0 + i % nw;
                unsigned long long bits = pixbits[(size_t)y * Wq + wq];
                const int xb = wq << 6;
                if (xb < bx0) bits &= ~0ULL << (bx0 - xb);                         // the part of the word inside the box
                if (xb + 63 > bx1) bits &= ~0ULL >> (xb + 63 - bx1);
                while (bits) {
                    const int j = __ffsll((long long)bits) - 1; bits &= bits - 1;
                    const int x = xb + j;
                    if (vs::in_capsule(x, y, x0, y0, x1, y1, r2)) { unsigned* q = &firstseq[(size_t)y * W + x]; if (*q > seq) atomicMin(q, seq); }   // (minima only decrease: a stale read costs a useless atomic at worst)
                }
            }
        }
    }
    if (lane == 0 && mine) atomicAdd(n_distinct, mine);
}

// ================================================================= A5: _PointHash.near (08:85-93)
// The samples of a polyline are contiguous (rank-major), so the hash of a polyline is its own sample range sorted by cell: a
// segmented sort on the 32-bit cell key (column, row).  The sort is stable, so every bucket lists its samples in pop order.
__device__ __forceinline__ unsigned cell_key(long long cx, long long cy) {
    return ((unsigned)((cx + 32768) & 0xffff) << 16) | (unsigned)((cy + 32768) & 0xffff);
}
__global__ __launch_bounds__(256) void k_cell_keys(SampleArrs A, unsigned MS, double inv, unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
    unsigned g = blockIdx.x * 256 + threadIdx.x;
    if (g >= MS) return;
    long long cx = (long long)floor(__dmul_rn(A.sx[g], inv)), cy = (long long)floor(__dmul_rn(A.sy[g], inv));
    keys[g] = cell_key(cx, cy); vals[g] = g;
}
// Two passes: the cheap test (own sample on the canvas, first stamp of its pixel earlier than its own pops) streams over all samples
// and collects the survivors; the hash-bucket searches (dozens of dependent loads) then run over the dense survivor list, so a wave
// is not held up by one lane that has to search.
__global__ __launch_bounds__(256) void k_accept_pre(SampleArrs A, const unsigned* __restrict__ sbase, const unsigned* __restrict__ npop, unsigned MS,
                                                     const unsigned* __restrict__ firstseq, int W, uint8_t* __restrict__ sflag,
                                                     unsigned* __restrict__ surv, unsigned* __restrict__ n_surv, unsigned long long* __restrict__ work) {
    // four samples per thread, 256 apart (as k_caps_insert: the chains rank -> base and pixel -> canvas word are waited for, not the bandwidth)
    constexpr int S = 4;
    const unsigned g0 = blockIdx.x * (256 * S) + threadIdx.x;
    unsigned g[S], bb[S], np[S]; int xi[S], yi[S]; bool ok[S], on[S];
#pragma unroll
    for (int u = 0; u < S; u++) { g[u] = g0 + 256u * u; on[u] = g[u] < MS; bb[u] = on[u] ? A.rank[g[u]] : 0u; }
#pragma unroll
    for (int u = 0; u < S; u++) {
        np[u] = 0; xi[u] = 0; yi[u] = 0; ok[u] = false;
        if (on[u]) { bb[u] = sbase[bb[u]]; const unsigned p = A.pxy[g[u]]; ok[u] = p != ORIP_PXY_OUT; np[u] = npop[g[u]]; xi[u] = pxy_x(p); yi[u] = pxy_y(p); }
    }
    unsigned fs[S];
#pragma unroll
    for (int u = 0; u < S; u++) fs[u] = (on[u] && ok[u]) ? firstseq[(size_t)yi[u] * W + xi[u]] : 0xffffffffu;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < S; u++) {
        bool need = false; unsigned mynp = 0;
        if (on[u]) {
            const unsigned j = g[u] - bb[u];
            const unsigned limit = bb[u] + np[u];         // own samples with global index < limit have been popped (hashed + stamped)
            bool k = ok[u];
            if (k && fs[u] < limit) k = false;
            sflag[g[u]] = (k ? 1 : 0) | (j == 0 ? 2 : 0);
            need = k && np[u] > 0; mynp = need ? np[u] : 0u;
        }
        const unsigned long long m = __ballot(need);
        if (m) {
            unsigned long long wsum = mynp;                    // popped own samples the survivors of this wave have to be compared with
            for (int o = 32; o > 0; o >>= 1) wsum += __shfl_xor(wsum, o, 64);
            unsigned base = 0;
            if (lane == 0) { base = atomicAdd(n_surv, (unsigned)__popcll(m)); atomicAdd(work, wsum); }
            base = (unsigned)__shfl((int)base, 0, 64);
            if (need) surv[base + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = g[u];
        }
    }
}
// _PointHash.near without the hash: a survivor is compared with ALL popped samples of its own polyline, 64 at a time.  Equal to the
// hash answer whenever the cell is at least the radius (every point within R then lies in the 3 x 3 cells the reference looks at), and
// cheap whenever the survivors are few and early in their polylines -- the bench image: 56 k survivors of 7.4e7 samples, all within
// the first lap of their walk; the bucket sort of ALL samples this replaces was the largest kernel of stage 08-A.  The host picks
// this path from the work sum k_accept_pre leaves (sum of popped samples over the survivors) and keeps the sorted buckets otherwise.
__global__ __launch_bounds__(256) void k_accept_brute(SampleArrs A, const unsigned* __restrict__ sbase, const unsigned* __restrict__ npop, double R2,
                                                       const unsigned* __restrict__ surv, const unsigned* __restrict__ n_surv, uint8_t* __restrict__ sflag) {
    const unsigned ns = *n_surv;
    const int lane = threadIdx.x & 63;
    for (unsigned t = blockIdx.x * 4 + (threadIdx.x >> 6); t < ns; t += gridDim.x * 4) {
        const unsigned g = surv[t];
        const unsigned b = sbase[A.rank[g]], np = npop[g];
        const double x = A.sx[g], y = A.sy[g];
        bool rej = false;
        for (unsigned q0 = 0; q0 < np && !rej; q0 += 64) {
            const unsigned q = q0 + (unsigned)lane; bool hit = false;
            if (q < np) {
                double ddx = __dsub_rn(A.sx[b + q], x), ddy = __dsub_rn(A.sy[b + q], y);
                hit = __dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)) <= R2;
            }
            if (__ballot(hit)) rej = true;
        }
        if (rej && lane == 0) sflag[g] &= (uint8_t)~1u;
    }
}
// one wavefront per survivor: 65-ary lower-bound searches and 64-wide scans of the three buckets of a column (they are neighbours in
// key order).  A bucket lists the polyline's own samples in pop order, so "popped before me" is simply g2 < limit; the reference
// stops at the first later sample, here later samples are just not counted -- the answer (any earlier sample within R) is the same.
__global__ __launch_bounds__(256) void k_accept(SampleArrs A, const unsigned* __restrict__ sbase, const unsigned* __restrict__ npop, double inv, double R2,
                                                 const unsigned* __restrict__ skeys, const unsigned* __restrict__ svals,
                                                 const unsigned* __restrict__ surv, const unsigned* __restrict__ n_surv, uint8_t* __restrict__ sflag) {
    const unsigned ns = *n_surv;
    const int lane = threadIdx.x & 63;
    for (unsigned t = blockIdx.x * 4 + (threadIdx.x >> 6); t < ns; t += gridDim.x * 4) {
        const unsigned g = surv[t];
        const unsigned r = A.rank[g], b = sbase[r];
        const double x = A.sx[g], y = A.sy[g];
        const unsigned limit = b + npop[g];
        const long long cx = (long long)floor(__dmul_rn(x, inv)), cy = (long long)floor(__dmul_rn(y, inv));
        const long long seg_end = sbase[r + 1];
        bool rej = false;
        for (int dx = -1; dx <= 1 && !rej; dx++) {
            const unsigned key_lo = cell_key(cx + dx, cy - 1), key_hi = cell_key(cx + dx, cy + 1);
            long long lo = b, hi = seg_end;                       // first entry >= key_lo
            while (hi - lo > 0) {
                const long long w = (hi - lo + 64) / 65;          // 64 probes split [lo, hi) into 65 parts
                const long long pos = lo + (long long)(lane + 1) * w - 1;
                const bool below = pos < hi && skeys[pos] < key_lo;
                const int cnt = __popcll(__ballot(below));        // probes are increasing: the `below` lanes are a prefix
                const long long nlo = lo + (long long)cnt * w;
                const long long nhi = (cnt < 64) ? min(hi, lo + (long long)(cnt + 1) * w - 1) : hi;
                lo = min(nlo, hi); hi = nhi;
            }
            for (long long q = lo; q < seg_end; q += 64) {
                const long long idx = q + lane;
                bool in = false, hit = false;
                if (idx < seg_end) {
                    const unsigned k = skeys[idx];
                    in = k <= key_hi;
                    if (in) {
                        const unsigned g2 = svals[idx];
                        if (g2 < limit) {
                            double ddx = __dsub_rn(A.sx[g2], x), ddy = __dsub_rn(A.sy[g2], y);
                            hit = __dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)) <= R2;
                        }
                    }
                }
                if (__ballot(hit)) { rej = true; break; }
                if (__ballot(in) != ~0ull) break;
            }
        }
        if (rej && lane == 0) sflag[g] &= (uint8_t)~1u;
    }
}

// ================================================================= prefetch of the order-independent part of the front (under stage 07's greedy)
// Stage 07 only permutes and flips the scaled contours (07:55-95), and it does so with a serial chain of greedy steps that keeps one
// wavefront busy for milliseconds.  What stage 08 computes PER POLYLINE before anything depends on the order -- bounding box and numpy
// perimeter of the opened polyline (A0 / A1), its float32 cumulative lengths and sample count (A2) -- depends on the direction the
// polyline is read in, nothing else.  So both directions are computed on the lane's side stream while the chain runs, and stage 08
// picks per polyline by stage 07's flip flag.  (Closed contours are never flipped, 07:60-62: their reversed entries are unused.)
__global__ __launch_bounds__(256) void k_pf_views(const PolyFeat* __restrict__ feat07, const int64_t* __restrict__ off, int64_t n, VView* __restrict__ vf, VView* __restrict__ vr,
                                                   int64_t* __restrict__ lf, int64_t* __restrict__ lr) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == n) { lf[i] = 0; lr[i] = 0; }
    if (i >= n) return;
    const unsigned len = (unsigned)(off[i + 1] - off[i]);
    VView a; a.wid = (unsigned)i; a.first = 0u; a.len = (feat07[i].closed && len > 0u) ? len - 1u : len; a.rev = 0u;     // _ensure_open (08:48-51), as split_small leaves the kept polylines
    VView b; b.wid = (unsigned)i; b.first = 0u; b.len = len; b.rev = 1u;
    vf[i] = a; vr[i] = b; lf[i] = a.len; lr[i] = b.len;
}
__global__ __launch_bounds__(256) void k_pf_pick_feat(const VView* __restrict__ sview, int64_t n, const PolyFeat* __restrict__ pf, const float* __restrict__ per_rev, PolyFeat* __restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const VView v = sview[k];
    PolyFeat f = pf[v.wid];
    if (v.rev) { const int32_t ax = f.sx, ay = f.sy; f.sx = f.ex; f.sy = f.ey; f.ex = ax; f.ey = ay; f.per = per_rev[v.wid]; }      // the reversed polyline: same box, same points, ends swapped, its own pairwise sum
    out[k] = f;
}
__global__ __launch_bounds__(256) void k_pf_pick_info(const VView* __restrict__ kview, int64_t nk, const RsInfo* __restrict__ pinfo, int64_t npf, const int64_t* __restrict__ off_f,
                                                       const int64_t* __restrict__ off_r, int64_t tot_f, RsInfo* __restrict__ info, int64_t* __restrict__ cumoff) {
    int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nk) return;
    const VView v = kview[j];
    info[j] = pinfo[v.rev ? npf + (int64_t)v.wid : (int64_t)v.wid];
    cumoff[j] = v.rev ? tot_f + off_r[v.wid] : off_f[v.wid];       // (both readings of a polyline sit at its offset in the scaled list)
}
struct StreamSwap {       // everything issued while this lives goes to the lane's side stream
    LaneRes& l;
    explicit StreamSwap(LaneRes& lane) : l(lane) { std::swap(l.stream, l.stream2); }
    ~StreamSwap() { std::swap(l.stream, l.stream2); }
};
static std::atomic<uint64_t> g_pf_tag{1};
}  // namespace
int orip_prefetch08(orip_ctx* c, const orip_params08& P, DPolys& S, const PolyFeat* feat07) {
    LaneRes::Prefetch08& F = LN(c).pf08;
    F.valid = false;
    const int64_t n = S.n, total = S.total;
    if (n <= 0 || total <= 0 || total > 0x3fffffff) return 0;
    const double step = std::max(1.0, P.sample_step);
    HIPC(c, F.feat.ensure((size_t)n * (sizeof(PolyFeat) + 4) + 64));
    HIPC(c, F.info.ensure((size_t)2 * n * sizeof(RsInfo) + 64));
    HIPC(c, F.cum.ensure((size_t)2 * total * 4 + 64));
    HIPC(c, F.ord.ensure((size_t)n * 16 + 64));
    HIPC(c, F.seg.ensure((size_t)total * 4 + 64));
    {
        StreamSwap sw(LN(c));                       // LN(c).stream is the side stream from here to the end of the block
        HIPC(c, hipStreamWaitEvent(LN(c).stream, LN(c).ev2, 0));      // stage 07's features (feat07) and its use of the shared scratch end here (vreorder)
        PolyFeat* ff = F.feat.as<PolyFeat>(); float* per_rev = reinterpret_cast<float*>(ff + n); RsInfo* inf = F.info.as<RsInfo>(); float* cum = F.cum.as<float>();
        VSrc sS; ORIP_TRY(vsrc_of(c, S, sS));
        // per-polyline fields first (open view, end points; bounding box and perimeters of the short ones): one thread per polyline
        vfeatures_short(c, sS, n, VF_PER | VF_OPEN_VIEW | VF_PER_REV, ff, per_rev);
        // A2 (the long polylines): cumulative lengths of both readings, longest first.  k_seglen fetches the points (once each) and leaves every segment's
        // float32 length in F.seg and the open view's bounding box in ff; both readings and the perimeter sums (A0 / A1, forwards and backwards) then
        // read 4 bytes per segment instead of turning (polyline, index) into a point again.
        unsigned* kin = F.ord.as<unsigned>(); unsigned* kout = kin + n; unsigned* vin = kout + n; unsigned* ordl = vin + n;
        float* seg = F.seg.as<float>();
        ORIP_TRY(vlen_order(c, S.off.as<int64_t>(), n, kin, kout, vin, ordl));
        // (the sort borrows the lane's scan / sort scratch: the main stream, which sits in the greedy chain for milliseconds yet, takes it back behind this point)
        HIPC(c, hipEventRecord(LN(c).ev4, LN(c).stream));
        HIPC(c, hipStreamWaitEvent(LN(c).stream2 /* the main stream while the swap lives */, LN(c).ev4, 0));
        // What stage 08 asks for first (split_small: boxes and perimeters) goes first and gets an event of its own (ev4); the cumulative lengths, which A2 picks
        // up a dozen launches and a host read later, follow (ev3).
        if (total > ORIP_LONG_CUM) {
            { ProfScope ps(c, "k_seglen"); hipLaunchKernelGGL(k_seglen<VSrc>, dim3((unsigned)cdiv(total, 4 * 63 * 64)), dim3(256), 0, LN(c).stream, sS, n, total, seg, ff); }
            if (total > ORIP_LONG_POLY) ORIP_TRY(vfeatures_long_seg(c, sS, n, total, ff, ordl, per_rev, seg));
        }
        HIPC(c, hipEventRecord(LN(c).ev4, LN(c).stream));
        { ProfScope ps(c, "k_cumlen"); hipLaunchKernelGGL(k_cumlen2<VSrc>, dim3(cdiv(2 * n, 128)), dim3(128), 0, LN(c).stream, sS, feat07, n, step, cum, total, inf); }
        if (total > ORIP_LONG_CUM) { ProfScope ps(c, "k_cumlen_long"); const dim3 grid((unsigned)std::min<int64_t>(n, 8192), 2);       // both readings side by side
            hipLaunchKernelGGL(k_cumlen_long2<VSrc>, grid, dim3(64), 0, LN(c).stream, sS, n, step, cum, total, inf, ordl, 0, (const float*)seg); }
        HIPC(c, hipGetLastError());
        HIPC(c, hipEventRecord(LN(c).ev3, LN(c).stream));
    }
    F.pending = true;             // nobody has waited yet: split_small (ev4), A2 (ev3), or the next call on the lane (orip_pf08_drain)
    F.valid = true; F.tag = g_pf_tag.fetch_add(1); F.n = n; F.tot_f = total; F.step = step; F.src_off = S.off.as<int64_t>();
    return 0;
}
namespace {

// split_small_and_taps on a DPolys -> kept (opened) + taps appended to tapbuf at tap_base
// kept_feat (optional, room for src.n entries): features of the kept polylines' open views (bbox + numpy perimeter), so the caller
// does not have to read the points again
int split_small(orip_ctx* c, DPolys& src, const orip_params08& P, DPolys& kept, DBuf& tapbuf, int64_t tap_base, int64_t* n_taps_out, PolyFeat* kept_feat = nullptr) {
    *n_taps_out = 0;
    HIPC(c, kept.clear(LN(c).stream));
    int64_t n = src.n;
    if (n == 0) return 0;
    unsigned *is_tap, *is_keep, *tap_scan, *keep_scan; int2* tap_xy; GatherDesc *kd, *kd2;
    { Carve L; L.each(n + 1, is_tap, is_keep, tap_scan, keep_scan, tap_xy, kd, kd2); HIPC(c, L.commit(LN(c).vtmp[VTL_SPLIT], 256)); }
    HIPC(c, LN(c).vtmp[VTL_SPLIT_FEAT].ensure((size_t)n * sizeof(PolyFeat) + 64));
    PolyFeat* sfeat = LN(c).vtmp[VTL_SPLIT_FEAT].as<PolyFeat>();
    if (is_coded(src) && P.tap_max_v > 64) ORIP_TRY(orip_polys_materialize(c, src));      // the walk-coded tap test copies <= 64 vertices (default tap_max_vertices: 50)
    LaneRes::Prefetch08& F = LN(c).pf08;
    if (kept_feat && is_coded(src) && src.pf_tag && F.valid && F.tag == src.pf_tag && !src.vident) {      // computed under stage 07's greedy, per walk and direction
        if (F.pending) HIPC(c, hipStreamWaitEvent(LN(c).stream, LN(c).ev4, 0));
        hipLaunchKernelGGL(k_pf_pick_feat, dim3(cdiv(n, 256)), dim3(256), 0, LN(c).stream, src.vview.as<VView>(), n, F.feat.as<PolyFeat>(), reinterpret_cast<const float*>(F.feat.as<PolyFeat>() + F.n), sfeat);
    } else { HIPC(c, orip_pf08_drain(c)); ORIP_TRY(vfeatures(c, src, kept_feat ? (VF_PER | VF_OPEN_VIEW) : 0, sfeat)); }      // (the prefetch shares vfeatures' scratch)
    { ProfScope ps(c, "k_split_small08"); ORIP_WITH_SRC(c, src, sv, { hipLaunchKernelGGL(k_split_small08<decltype(sv)>, dim3(cdiv(n + 1, 128)), dim3(128), 0, LN(c).stream, sv, n, P, sfeat, is_tap, is_keep, tap_xy, kd); }); }
    ORIP_TRY(vscan_excl<unsigned>(c, is_tap, tap_scan, (size_t)n + 1));
    ORIP_TRY(vscan_excl<unsigned>(c, is_keep, keep_scan, (size_t)n + 1));
    unsigned nt = 0, nk = 0;
    HIPC(c, hipMemcpyAsync(&nt, tap_scan + n, 4, hipMemcpyDeviceToHost, LN(c).stream));      // both counts, one wait
    ORIP_TRY(vread(c, &nk, keep_scan + n));
    if (nt) {
        HIPC(c, tapbuf.ensure((size_t)(tap_base + nt) * 8 + 64, LN(c).stream, true));
        hipLaunchKernelGGL(k_compact<int2>, dim3(cdiv(n, 256)), dim3(256), 0, LN(c).stream, is_tap, tap_scan, n, tap_xy, tapbuf.as<int2>() + tap_base);
    }
    *n_taps_out = nt;
    if (nk) {
        hipLaunchKernelGGL(k_compact<GatherDesc>, dim3(cdiv(n, 256)), dim3(256), 0, LN(c).stream, is_keep, keep_scan, n, kd, kd2);
        ORIP_TRY(vgather_list(c, kd2, nk, src, kept));
        if (kept_feat) hipLaunchKernelGGL(k_compact<PolyFeat>, dim3(cdiv(n, 256)), dim3(256), 0, LN(c).stream, is_keep, keep_scan, n, sfeat, kept_feat);
    }
    HIPC(c, hipGetLastError());
    return 0;
}

// Also clears the any-out word that k_rank_counts sets (A08::sbase has the argument).
__global__ __launch_bounds__(256) void k_fill_per(const PolyFeat* __restrict__ f, int64_t n, float* __restrict__ k, unsigned* __restrict__ v, unsigned* __restrict__ any_out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *any_out = 0u;
    if (i < n) { k[i] = f[i].per; v[i] = (unsigned)i; }
}

// ================================================================= the phases of stage 08-A
// What flows from one phase of a dedup08_a call to the next: device pointers into the lane's scratch (the slot behind each group; orip_ctx.h has the
// lifetimes) and the counts the host has read back.
struct A08 {
    int64_t nk;                                                     // kept polylines
    PolyFeat* feat;                                                 // VTL_FEAT: their open-view features (A0 -> k_rank_counts)
    unsigned *ord, *mr, *sbase; RsInfo* info;                       // VTL_RANKS: order by perimeter, samples per rank, sample bases (nk + 1, then the any-out word), lengths
    // The any-out word, sbase[nk + 1], is cleared by k_fill_per (first kernel of A1, right behind the carve) and set by k_rank_counts (A2); in between run the
    // perimeter sort (its own four arrays and tmpF) and the cumulative lengths (VTL_CUM, info, or the prefetch's buffers): nothing touches the word, and the side
    // stream has no work of this call yet.  The read-back behind the scan of mr is its only reader.
    unsigned* redo;                                                 // VTL_RANKS too: nk + 1 words, 1 + the last sample the sequential simulation redoes (0: none).  Cleared by k_rank_counts (A2); set
    // by k_tail_par (A3), read by k_tail_replay on the side stream until ev3, which A5 awaits; between clearing and setting run the scan of mr, k_sample_hints and
    // k_samples, which take mr, sbase, info, ord of this slot and never redo, and nothing of this call on the side stream.  VTL_RANKS stays until A6.
    double step; int64_t* cumoff; float* cum;                       // VTL_CUM, or the prefetch's cum: cumulative lengths and where each polyline's start
    unsigned MS; bool any_out;                                      // samples of the layer; some polyline leaves the canvas
    SampleArrs A; unsigned* npop; int* capprev; uint8_t* sflag;     // VTL_SAMPLES: one entry per sample (capprev == nullptr: every sample is on the canvas); A.Sloc: VTL_TAIL_RUNS
    unsigned *ckin, *ckout, *cvin, *cvout; int2* hints;             // VTL_CELLS: cell keys / values of the bucket sort, hints of k_samples
    double cell, inv;                                               // side of a _PointHash cell and its inverse
    int Wq; unsigned* firstseq; unsigned long long* pixbits;        // canvas: first stamp per sample pixel; pixbits: the sample pixels, Wq words per row
};

// ---- A1: order by perimeter, descending, stable
static int a1_order(orip_ctx* c, A08& a) {
    const int64_t nk = a.nk; float *kin, *kout; unsigned* vin;
    { Carve L; L.each(nk, kin, kout, vin, a.ord); L.take(a.mr, nk + 1);
      L.take(a.sbase, nk + 2); L.take(a.info, nk); L.take(a.redo, nk + 1); HIPC(c, L.commit(LN(c).vtmp[VTL_RANKS], 256)); }      // sbase: nk + 1 sample bases, then the any-out word (one read-back fetches both)
    hipLaunchKernelGGL(k_fill_per, dim3(cdiv(nk, 256)), dim3(256), 0, LN(c).stream, a.feat, nk, kin, vin, a.sbase + nk + 1);
    ORIP_TRY((vsort_pairs<float, unsigned>(c, kin, kout, vin, a.ord, (size_t)nk, 0, 32, true)));
    return 0;
}
// ---- A2: resample.  Cumulative lengths, the sample count (a.MS; nothing more is done when it is 0), then every sample's record
static int a2_resample(orip_ctx* c, const orip_params08& P, DPolys& kept0, A08& a, PhaseTimer& T) {
    const int W = P.W, H = P.H; const int64_t nk = a.nk;
    a.step = std::max(1.0, P.sample_step);
    const LaneRes::Prefetch08& F = LN(c).pf08;
    const bool picked = is_coded(kept0) && kept0.pf_tag && F.valid && F.tag == kept0.pf_tag && F.step == a.step && !kept0.vident;
    HIPC(c, orip_pf08_drain(c));          // the cumulative lengths of the prefetch (ev3), if nobody has waited for them yet
    { Carve L; L.take(a.cumoff, nk + 1); L.take(a.cum, picked ? 0 : kept0.total); HIPC(c, L.commit(LN(c).vtmp[VTL_CUM], 128)); }
    if (picked) {       // cumulative lengths and sample counts were taken under stage 07's greedy, per walk and direction: pick this list's
        a.cum = F.cum.as<float>();
        hipLaunchKernelGGL(k_pf_pick_info, dim3(cdiv(nk, 256)), dim3(256), 0, LN(c).stream, kept0.vview.as<VView>(), nk, F.info.as<RsInfo>(), F.n, F.src_off, F.src_off, F.tot_f, a.info, a.cumoff);
    } else {
        HIPC(c, hipMemcpyAsync(a.cumoff, kept0.off.p, (size_t)(nk + 1) * 8, hipMemcpyDeviceToDevice, LN(c).stream));
        { ProfScope ps(c, "k_cumlen"); ORIP_WITH_SRC(c, kept0, sv, { hipLaunchKernelGGL(k_cumlen<decltype(sv)>, dim3(cdiv(nk, 128)), dim3(128), 0, LN(c).stream, sv, nk, a.step, a.cum, a.info); }); }
        if (kept0.total > ORIP_LONG_CUM) { ProfScope ps(c, "k_cumlen_long"); ORIP_WITH_SRC(c, kept0, sv, {
                hipLaunchKernelGGL(k_cumlen_long2<decltype(sv)>, dim3((unsigned)std::min<int64_t>(nk, 8192), 1), dim3(64), 0, LN(c).stream, sv, nk, a.step, a.cum, (int64_t)0, a.info, a.ord, 0, (const float*)nullptr); }); }
    }
    T.tick("cumlen");
    hipLaunchKernelGGL(k_rank_counts, dim3(cdiv(nk + 1, 256)), dim3(256), 0, LN(c).stream, a.info, a.ord, nk, a.mr, a.feat, W, H, a.sbase + nk + 1, a.redo);
    ORIP_TRY(vscan_excl<unsigned>(c, a.mr, a.sbase, (size_t)nk + 1));
    unsigned ms_out[2] = {0, 0};
    ORIP_TRY(vread(c, ms_out, a.sbase + nk, 2));                // the sample count and, with it, whether any polyline leaves the canvas
    const unsigned MS = a.MS = ms_out[0]; a.any_out = ms_out[1] != 0 || getenv("ORIP_CAPPREV_SCAN");
    if (MS == 0) return 0;
    if (MS > 0x7ffffff0u) ORIP_FAIL(c, "too many samples");
    if (T.on) { char b[48]; snprintf(b, sizeof b, " [MS %u]", MS); T.log += b; }
    { Carve L; L.each(MS, a.A.sx, a.A.sy, a.A.dprev, a.A.pxy, a.A.rank, a.npop, a.capprev, a.sflag); HIPC(c, L.commit(LN(c).vtmp[VTL_SAMPLES], 1024)); }
    { Carve L; L.take(a.A.Sloc, MS); HIPC(c, L.commit(LN(c).vtmp[VTL_TAIL_RUNS], 64)); }      // block-local tail sums: k_samples -> k_tail_par
    const unsigned nb = (unsigned)cdiv(MS, 256);
    { Carve L; L.each(MS, a.ckin, a.ckout, a.cvin, a.cvout); L.take(a.hints, nb + 1, 64);
      HIPC(c, L.commit(LN(c).vtmp[VTL_CELLS], 64 + (size_t)MS * 8)); }      // (8 MS: what two retired arrays took; no request shrinks with the layouts' restatement)
    a.cell = P.grid_stride > 0 ? P.grid_stride : std::max(4.0, P.col_rad); a.inv = 1.0 / a.cell;
    // canvas of first stamps: read at sample pixels only, so k_samples initialises exactly those and marks them in a bit plane
    a.Wq = (W + 63) >> 6;
    HIPC(c, LN(c).canvas.ensure((size_t)W * H * 4 + 64));
    a.firstseq = LN(c).canvas.as<unsigned>();
    HIPC(c, LN(c).pixbits.ensure((size_t)a.Wq * H * 8 + 64));
    a.pixbits = LN(c).pixbits.as<unsigned long long>();
    HIPC(c, hipMemsetAsync(a.pixbits, 0, (size_t)a.Wq * H * 8, LN(c).stream));
    hipLaunchKernelGGL(k_sample_hints, dim3(cdiv(nb, 256)), dim3(256), 0, LN(c).stream, a.cumoff, a.cum, a.info, a.ord, a.sbase, nk, MS, a.step, nb, a.hints);
    { ProfScope ps(c, "k_samples"); ORIP_WITH_SRC(c, kept0, sv, { hipLaunchKernelGGL(k_samples<decltype(sv)>, dim3(cdiv(nb, 4)), dim3(256), 0, LN(c).stream, sv, a.cumoff, a.cum, a.info, a.ord, a.sbase, nk, MS, a.step, W, H, a.A, a.hints, (unsigned)nb, a.pixbits, a.Wq, a.firstseq); }); }
    T.tick("samples");
    return 0;
}
// ORIP_TAIL_DBG (debug): how much of the layer the sequential tail simulation redoes.  Waits for the lane's stream.
// redo[q] is 1 + the last unsure sample of polyline q (0: not redone); first[q] the first unsure one (k_tail_par's dbg_first).
static void tail_dbg_dump(orip_ctx* c, int layer, const A08& a, const unsigned* first) {
    const int64_t nk = a.nk;
    std::vector<unsigned> h(nk), sb(nk + 1), f(nk);
    hipStreamSynchronize(LN(c).stream);
    hipMemcpy(h.data(), a.redo, nk * 4, hipMemcpyDeviceToHost);
    hipMemcpy(sb.data(), a.sbase, (nk + 1) * 4, hipMemcpyDeviceToHost);
    hipMemcpy(f.data(), first, nk * 4, hipMemcpyDeviceToHost);
    unsigned long long nf = 0, sf = 0, mx = 0, upto = 0;
    std::vector<int64_t> red;
    for (int64_t q = 0; q < nk; q++) if (h[q]) { nf++; sf += sb[q + 1] - sb[q]; upto += h[q]; mx = std::max<unsigned long long>(mx, sb[q + 1] - sb[q]); red.push_back(q); }
    fprintf(stderr, "[tail dbg] layer %d: %llu of %lld polylines redone, %llu of %u samples (%llu up to the last unsure one), longest redone %llu\n", layer, nf, (long long)nk, sf, a.MS, upto, mx);
    std::stable_sort(red.begin(), red.end(), [&](int64_t x, int64_t y) { return sb[x + 1] - sb[x] > sb[y + 1] - sb[y]; });
    for (size_t i = 0; i < red.size() && i < 5; i++) { const int64_t q = red[i];
        fprintf(stderr, "[tail dbg]   rank %lld: %u samples, first unsure %u, last unsure %u\n", (long long)q, sb[q + 1] - sb[q], f[q], h[q] - 1u); }
}
// the replay's counters (LaneFlags::tail_dbg).  Waits for the lane's side stream.
static void tail_dbg_replay(orip_ctx* c, int layer, const unsigned long long* dbg) {
    unsigned long long v[4] = {0, 0, 0, 0};
    hipStreamSynchronize(LN(c).stream2);
    hipMemcpy(v, dbg, sizeof v, hipMemcpyDeviceToHost);
    fprintf(stderr, "[tail dbg] layer %d: replay %llu rounds, %llu samples committed by rounds, %llu by the plain loop, %llu rounds in the integer form\n", layer, v[0], v[1], v[2], v[3]);
}
// ---- A3: pops per sample (tail simulation), then the previous in-canvas sample of every sample
static int a3_tails(orip_ctx* c, int layer, const orip_params08& P, A08& a) {
    const int64_t nk = a.nk; const unsigned MS = a.MS;
    {
        ProfScope ps(c, "k_tail_sim");
        const bool dbg = getenv("ORIP_TAIL_DBG") != nullptr;
        unsigned* dbg_first = nullptr; unsigned long long* dbg_cnt = nullptr;      // (debug: a buffer of its own, released below)
        if (dbg) {
            HIPC(c, hipMalloc(&dbg_first, (size_t)(nk + 1) * 4));
            const hipError_t me = hipMemsetAsync(dbg_first, 0xff, (size_t)(nk + 1) * 4, LN(c).stream);
            if (me != hipSuccess) { hipFree(dbg_first); HIPC(c, me); }      // (nothing between here and the hipFree below returns)
            dbg_cnt = LN(c).flags.as<LaneFlags>()->tail_dbg;
        }
        hipLaunchKernelGGL(k_tail_par, dim3(cdiv(MS, 256)), dim3(256), 0, LN(c).stream, a.sbase, a.A.rank, a.A.Sloc, MS, P.tail_len_px, a.npop, a.redo, dbg_first);
        if (dbg) { tail_dbg_dump(c, layer, a, dbg_first); hipFree(dbg_first); HIPC(c, hipMemsetAsync(dbg_cnt, 0, sizeof(LaneFlags::tail_dbg), LN(c).stream)); }
        const unsigned* only = getenv("ORIP_TAIL_SEQ") ? nullptr : a.redo;          // test hook: force the sequential simulation everywhere
        // the sequential redo only feeds the acceptance test (A6): it runs on the lane's side stream under the capsule / hash work
        HIPC(c, hipEventRecord(LN(c).ev2, LN(c).stream));
        HIPC(c, hipStreamWaitEvent(LN(c).stream2, LN(c).ev2, 0));
        hipLaunchKernelGGL(k_tail_replay, dim3((unsigned)std::min<int64_t>(nk, 65535)), dim3(64), 0, LN(c).stream2, a.sbase, nk, P.tail_len_px, a.A, a.npop, only, dbg_cnt);
        HIPC(c, hipEventRecord(LN(c).ev3, LN(c).stream2));
        if (dbg) tail_dbg_replay(c, layer, dbg_cnt);
    }
    if (a.any_out) {
        unsigned* lastin = LN(c).vtmp[VTL_TAIL_RUNS].as<unsigned>();            // MS words over Sloc: k_tail_par has consumed the tail sums
        auto vin = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0u), IncIndex{a.A.pxy});
        HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::inclusive_scan_by_key(tmp, bytes, a.A.rank, vin, lastin, (size_t)MS, rocprim::maximum<unsigned>(), rocprim::equal_to<unsigned>(), LN(c).stream); }));
        hipLaunchKernelGGL(k_capprev, dim3(cdiv(MS, 256)), dim3(256), 0, LN(c).stream, a.sbase, MS, a.A, lastin, a.capprev);
    }
    else a.capprev = nullptr;       // every sample is on the canvas: "the previous in-canvas sample" is simply the previous one (k_caps_insert)
    return 0;
}
// ---- A4: de-duplicated capsules -> min-sequence canvas.  Leaves the number of distinct capsules in flags.caps_distinct.
static int a4_capsules(orip_ctx* c, const orip_params08& P, A08& a) {
    const unsigned MS = a.MS; LaneFlags* fl = LN(c).flags.as<LaneFlags>();
    // The table only has to hold the DISTINCT capsules (retraced paths repeat theirs many times).  Their number is not known in advance:
    // start from what this lane saw last time (a resident chain repeats itself; 3 slots per capsule), else from a quarter of the sample
    // count, with bounded probing, and grow on overflow; 2 * MS slots always suffice.  A small table is a cache-resident one.
    unsigned long long tfull = 1024; while (tfull < 2ull * MS) tfull <<= 1;
    unsigned long long tsize = 1024;
    if (LN(c).caps_hint) { while (tsize < 3ull * LN(c).caps_hint) tsize <<= 1; } else { while (tsize < MS / 4ull) tsize <<= 1; }
    tsize = std::min(tsize, tfull);
    if (getenv("ORIP_CAPS_TINY")) tsize = 1024;            // test hook: exercise the growth path
    // The range of samples a workgroup owns and the slots of its set in LDS (k_caps_insert).  A longer range filters more and leaves fewer workgroups, each
    // going through its chunks one after the other: the card holds 256 x 6 workgroups of 24 KB of LDS at a time, so the largest range that still leaves
    // 2048 of them, down to one chunk, where the set only filters inside the chunk.  (Candidates and their times, longer ranges included: DESIGN 8.3.)
    static const unsigned cand[] = {8192u, 4096u, 2048u, 1024u};
    unsigned R = 1024u, TS = 2048u;
    for (unsigned r : cand) if (cdiv(MS, r) >= 2048 || r == 1024u) { R = r; break; }
    if (const char* e = getenv("ORIP_CAPS_RANGE")) {       // test hook: "R" or "R:T", a range of R samples (and a set of T slots) whatever the layer's size
        char* end = nullptr; const unsigned long r = strtoul(e, &end, 10); unsigned long t = TS;
        if (end && *end == ':') t = strtoul(end + 1, nullptr, 10);
        if (r < 1024 || r > 65536 || (r & 1023)) ORIP_FAIL(c, "ORIP_CAPS_RANGE: a multiple of 1024 up to 65536");
        if (t < 32 || t > 4096 || (t & (t - 1))) ORIP_FAIL(c, "ORIP_CAPS_RANGE: a power of two from 32 to 4096 slots");
        R = (unsigned)r; TS = (unsigned)t;
    }
    if (getenv("ORIP_CAPSSET_TINY")) TS = 32u;             // test hook: most samples find no room in the set
    const unsigned lds = TS * 12u;                         // 64-bit keys, then 32-bit sample indices: 24 KB
    CapSlot* tab = nullptr;
    int* d_ovf = &fl->caps_overflow; unsigned* d_dist = &fl->caps_distinct;
    for (;; tsize = std::min(tfull, tsize * 4)) {
        HIPC(c, LN(c).vtmp[VTL_CAPS].ensure((size_t)tsize * 16 + 64));
        tab = LN(c).vtmp[VTL_CAPS].as<CapSlot>();
        hipLaunchKernelGGL(k_caps_init, dim3((unsigned)cdiv(tsize, 256)), dim3(256), 0, LN(c).stream, tab, tsize, fl);      // (and the counters of A4 / A5)
        const int max_probe = tsize >= tfull ? 0x7fffffff : 96;
        { ProfScope ps(c, "k_caps_insert");
          if (a.capprev) hipLaunchKernelGGL(k_caps_insert<true>, dim3(cdiv(MS, R)), dim3(256), lds, LN(c).stream, a.A, a.sbase, a.capprev, MS, R / 1024u, TS - 1u, tab, tsize - 1, max_probe, d_ovf);
          else hipLaunchKernelGGL(k_caps_insert<false>, dim3(cdiv(MS, R)), dim3(256), lds, LN(c).stream, a.A, a.sbase, a.capprev, MS, R / 1024u, TS - 1u, tab, tsize - 1, max_probe, d_ovf); }
        int ovf = 0; ORIP_TRY(vread(c, &ovf, d_ovf));
        if (!ovf) break;
    }
    {
        ProfScope ps(c, "k_caps_stamp");
        const dim3 sg((unsigned)std::min<unsigned long long>(tsize / 64 / 4 + 1, 16384));
        hipLaunchKernelGGL(k_caps_stamp_bits, sg, dim3(256), 0, LN(c).stream, tab, tsize, P.brush_forbid / 2, a.firstseq, P.W, P.H, a.pixbits, a.Wq, d_dist);
    }
    return 0;
}
// ---- A5 / A6: cheap test of every sample, then _PointHash.near for the survivors
static int a56_accept(orip_ctx* c, const orip_params08& P, A08& a, PhaseTimer& T) {
    const int64_t nk = a.nk; const unsigned MS = a.MS; LaneFlags* fl = LN(c).flags.as<LaneFlags>();
    HIPC(c, hipStreamWaitEvent(LN(c).stream, LN(c).ev3, 0));       // pop counts of the redone polylines
    unsigned* surv = LN(c).vtmp[VTL_TAIL_RUNS].as<unsigned>();      // MS words again (the scan results kept there have been consumed by k_capprev)
    unsigned* d_ns = &fl->accept_survivors; unsigned long long* d_work = &fl->accept_work;
    { ProfScope ps(c, "k_accept"); hipLaunchKernelGGL(k_accept_pre, dim3(cdiv(MS, 1024)), dim3(256), 0, LN(c).stream, a.A, a.sbase, a.npop, MS, a.firstseq, P.W, a.sflag, surv, d_ns, d_work); }
    unsigned long long h_work = 0; ORIP_TRY(vread(c, &h_work, d_work));
    const double R2 = P.col_rad * P.col_rad;
    // without the hash when it gives the hash's answer (cell >= radius) and costs less than sorting every sample into buckets
    const bool brute = a.cell >= P.col_rad && h_work <= 64ull * (unsigned long long)MS && !getenv("ORIP_HASH_SORT");
    if (T.on) { char b2[64]; snprintf(b2, sizeof b2, " [near work %llu %s]", h_work, brute ? "direct" : "buckets"); T.log += b2; }
    if (brute) {
        ProfScope ps(c, "k_accept");
        hipLaunchKernelGGL(k_accept_brute, dim3((unsigned)std::min<unsigned>(cdiv(MS, 256), 16384u)), dim3(256), 0, LN(c).stream, a.A, a.sbase, a.npop, R2, surv, d_ns, a.sflag);
    } else {
        // (polyline, cell) buckets in pop order: the samples of a polyline are contiguous, so its hash is its own range sorted by cell key
        hipLaunchKernelGGL(k_cell_keys, dim3(cdiv(MS, 256)), dim3(256), 0, LN(c).stream, a.A, MS, a.inv, a.ckin, a.cvin);
        { ProfScope ps(c, "sort_cells"); HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::segmented_radix_sort_pairs(tmp, bytes, a.ckin, a.ckout, a.cvin, a.cvout, (unsigned)MS, (unsigned)nk, a.sbase, a.sbase + 1, 0u, 32u, LN(c).stream); })); }
        ProfScope ps(c, "k_accept");
        hipLaunchKernelGGL(k_accept, dim3((unsigned)std::min<unsigned>(cdiv(MS, 256), 16384u)), dim3(256), 0, LN(c).stream, a.A, a.sbase, a.npop, a.inv, R2, a.ckout, a.cvout, surv, d_ns, a.sflag);
    }
    HIPC(c, hipGetLastError());
    return 0;
}
}  // namespace

int dedup08_a(orip_ctx* c, int layer, const orip_params08& P, DPolys& S, DTaps& TOUT, PhaseTimer& T, bool& caps_counted) {
    DPolys& kept0 = LN(c).tp[0]; DPolys& cleaned = LN(c).tp[1]; DPolys& lines2 = LN(c).tp[2];
    int64_t nt0 = 0, nt2 = 0;
    A08 a{};
    // ---- A0: tiny polylines -> taps / dropped; the rest opened, with their features
    HIPC(c, LN(c).vtmp[VTL_FEAT].ensure((size_t)S.n * sizeof(PolyFeat) + 64));
    a.feat = LN(c).vtmp[VTL_FEAT].as<PolyFeat>();       // open-view features of the kept polylines (perimeter: A1)
    ORIP_TRY(split_small(c, S, P, kept0, TOUT.xy, 0, &nt0, a.feat));
    a.nk = kept0.n;
    T.tick("split");
    if (a.nk > 0) {
        if (kept0.total > 0x7fffffff) ORIP_FAIL(c, "layer too large");
        T.tick("feat");
        ORIP_TRY(a1_order(c, a));                          T.tick("A0-1");
        ORIP_TRY(a2_resample(c, P, kept0, a, T));          // (laps "cumlen" and, with samples, "samples")
        if (a.MS > 0) {
            ORIP_TRY(a3_tails(c, layer, P, a));            T.tick("tail");
            ORIP_TRY(a4_capsules(c, P, a));                caps_counted = true; T.tick("caps");
            ORIP_TRY(a56_accept(c, P, a, T));              T.tick("accept");
            ORIP_TRY(orip_runs_to_polys(c, SlotPtsF64{a.A.sx, a.A.sy}, a.sflag, a.MS, cleaned));
            T.tick("runs");
        }
        // ---- A7: the same split on the cleaned lines
        ORIP_TRY(split_small(c, cleaned, P, lines2, TOUT.xy, nt0, &nt2));
    }
    TOUT.n = nt0 + nt2;
    return 0;
}
