// csrc/gcode_simplify.hip -- --simplify-mm of gcode2stream.py / svg2stream.py: Ramer-Douglas-Peucker on the step grid, per stroke, exact in integers
// (orip_gcode_simplify; the rule is stated in include/orip.h and has one answer for every input).  Ours: the reference's simplify settings are dead.
//
// The unit of work is a SPAN (a, b): two kept points, as indices into the point list, whose interior a + 1 .. b - 1 is still undecided.  A span's point is
// the interior point with the largest 128-bit key K, the lowest index among equals; it is kept or the whole interior is dropped, and a kept point leaves
// two spans.  Which span is worked on when changes nothing: a span's answer depends on its two ends only, and the keep flags are a set.
//
// 1. Seed.  One thread per stroke flags its two ends and writes its span to list 0 (a stroke of two points writes a span without interior, which the
//    next kernel skips: no atomic, no compaction).
// 2. Levels.  Two kernels per level, fixed grids that stride over the current list; the count is read from device memory.
//      k_sp_level, one WAVE per span: a span of at most ORIP_SIMPLIFY_LOCAL points is FINISHED by its wave.  The points are staged in the wave's slice of
//      LDS, an explicit stack in LDS pushes the larger child and goes on with the smaller, so its depth stays under log2 of the span; per sub-span the
//      lanes take the interior 64 points at a time and the (K, index) maximum is reduced across the 64 lanes by a butterfly of shuffles, which leaves it
//      in every lane.
//      k_sp_long, one BLOCK per span (launched only when the input has more points than a wave finishes): a longer span gets ONE arg-max pass over
//      global memory, four loads per thread in flight, the four waves' winners combined in LDS; thread 0 sets the flag and appends the children that
//      have an interior to the next list with one atomicAdd.  One wave per long span took 41 - 65 ms in the levels on the drawing of tools/time_simplify.py, whose
//      first levels are a single span of 10^6 points: DESIGN 6 "simplify" has both figures.
//    Lists are double-buffered; three count words rotate (level r reads cnt[r % 3], k_sp_long adds to cnt[(r + 1) % 3] and k_sp_level clears
//    cnt[(r + 2) % 3]), so no word is read and written by one launch.  The host enqueues SP_BATCH levels, reads the SpState, and goes on while the next list is not empty: no round trip
//    per level, and launches behind the end find a count of 0 and do nothing.  No kernel waits for another workgroup.  rounds = levels behind level 0
//    that found a span.  Spans of one level are disjoint and a long one covers more than ORIP_SIMPLIFY_LOCAL - 1 segments, so a level appends at most
//    2 total / ORIP_SIMPLIFY_LOCAL children; the list capacity is max(n, that) and an append past it fails the call instead of writing.
// 3. Emit.  An exclusive scan over the keep flags gives every kept point its place; one thread per input point copies it and its index there, one thread
//    per stroke reads the new offset at its first point.
//
// Scratch, free between calls.  c->sp_tmp: keep u8[total + 1] (the last one stays 0, so the scan's last word is the output count); pos unsigned[total + 1];
// list int2[2][cap]; SpState.  Output: c->sp_off / c->sp_pts, made the resident list when the call succeeds (gc_publish; orip_ctx.h states the contract).
// Resident: kept int64[sp_points] in c->sp_res until the next call.
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <climits>

namespace {
constexpr int SP_S = ORIP_SIMPLIFY_LOCAL;           // points a wave finishes alone: SP_WAVES * SP_S * 8 bytes of LDS per block
constexpr int SP_WAVES = 4;
constexpr int SP_BLOCKS = 2048;                     // 8 per CU
constexpr int SP_LONG_BLOCKS = 1024;                // k_sp_long: one block per span longer than SP_S
constexpr int SP_STACK = 32;                        // the larger child is pushed: the depth stays under log2(SP_S) = 10
constexpr int SP_BATCH = 8;                         // levels between two looks at the counts
struct SpState { unsigned cnt[3], rounds, bad; };
typedef unsigned __int128 u128;
typedef unsigned long long u64;

struct SpChord { int2 A, B; long long dx, dy; u64 L; };
__device__ __forceinline__ SpChord sp_chord(const int2 A, const int2 B) {
    SpChord c; c.A = A; c.B = B; c.dx = (long long)B.x - A.x; c.dy = (long long)B.y - A.y; c.L = (u64)(c.dx * c.dx + c.dy * c.dy);
    return c;
}
// squared distance to the segment times L (L == 0: the squared distance to the point); differences are within 2^30, so every sum of two products is
// within 2^61 and only the last product needs 128 bits
__device__ __forceinline__ u128 sp_key(const SpChord& c, const int2 P) {
    const long long px = (long long)P.x - c.A.x, py = (long long)P.y - c.A.y;
    const u64 da = (u64)(px * px + py * py);
    if (c.L == 0) return (u128)da;
    const long long t = px * c.dx + py * c.dy;
    if (t <= 0) return (u128)da * c.L;
    if ((u64)t >= c.L) { const long long qx = (long long)P.x - c.B.x, qy = (long long)P.y - c.B.y; return (u128)(u64)(qx * qx + qy * qy) * c.L; }
    const long long cr = px * c.dy - py * c.dx;
    const u64 a = (u64)(cr < 0 ? -cr : cr);
    return (u128)a * a;
}
__device__ __forceinline__ bool sp_kept(const SpChord& c, const u128 K, const u64 tol4sq) { return c.L == 0 ? K > 0 : (K << 4) > (u128)tol4sq * c.L; }

// the largest K, the lowest index among equals, over the 64 lanes; every lane leaves with it
__device__ __forceinline__ void sp_wave_max(u128& K, int& idx) {
    u64 hi = (u64)(K >> 64), lo = (u64)K;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 oh = __shfl_xor(hi, m, 64), ol = __shfl_xor(lo, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        if (oh > hi || (oh == hi && (ol > lo || (ol == lo && oi < idx)))) { hi = oh; lo = ol; idx = oi; }
    }
    K = ((u128)hi << 64) | lo;
}
// LDS that one lane wrote and another lane of the same wave reads
__device__ __forceinline__ void sp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void k_sp_seed(const long long* __restrict__ off, int n, long long total, int2* __restrict__ list, uint8_t* __restrict__ keep, SpState* st) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    if (p == 0) st->cnt[0] = (unsigned)n;
    const long long a = off[p], b = off[p + 1] - 1;
    if (a < 0 || b < a || b >= total) { atomicOr(&st->bad, 1u); list[p] = make_int2(0, 0); return; }
    keep[a] = 1; keep[b] = 1;
    list[p] = make_int2((int)a, (int)b);
}

__global__ __launch_bounds__(256) void k_sp_level(const int2* __restrict__ pts, const int2* __restrict__ cur, unsigned cap, SpState* st, int ci, int zi, int counts, u64 tol4sq,
                                                  uint8_t* __restrict__ keep, int total) {
    __shared__ int2 lds_pts[SP_WAVES][SP_S];
    __shared__ int2 lds_stk[SP_WAVES][SP_STACK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned count = min(st->cnt[ci], cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->cnt[zi] = 0; if (counts && count) st->rounds++; }
    int2* const P = lds_pts[w]; int2* const S = lds_stk[w];
    for (unsigned k = blockIdx.x * SP_WAVES + w; k < count; k += gridDim.x * SP_WAVES) {
        const int2 sp = cur[k];
        const int a = __builtin_amdgcn_readfirstlane(sp.x), b = __builtin_amdgcn_readfirstlane(sp.y);
        if (a < 0 || b >= total || b - a < 2 || b - a >= SP_S) continue;     // no interior (a stroke of two points), or k_sp_long's
        const int np = b - a + 1;
        for (int i = lane; i < np; i += 64) P[i] = pts[a + i];
        sp_wave_sync();
        int lo = 0, hi = np - 1, top = 0;
        for (;;) {                                                        // (lo, hi) has an interior
            const SpChord c = sp_chord(P[lo], P[hi]);
            u128 K = 0; int m = INT_MAX;
            for (int i = lo + 1 + lane; i < hi; i += 64) { const u128 q = sp_key(c, P[i]); if (q > K) { K = q; m = i; } }
            sp_wave_max(K, m);
            m = __builtin_amdgcn_readfirstlane(m);
            if (sp_kept(c, K, tol4sq) && m > lo && m < hi) {
                if (lane == 0) keep[a + m] = 1;
                const bool left = m - lo >= 2, right = hi - m >= 2;
                if (left && right) {
                    const bool left_larger = m - lo > hi - m;
                    if (top < SP_STACK) { S[top] = left_larger ? make_int2(lo, m) : make_int2(m, hi); top++; } else if (lane == 0) atomicOr(&st->bad, 2u);
                    if (left_larger) lo = m; else hi = m;
                    continue;
                }
                if (left) { hi = m; continue; }
                if (right) { lo = m; continue; }
            }
            if (top == 0) break;
            top--;
            const int2 e = S[top];                                        // every lane wrote this entry itself
            lo = e.x; hi = e.y;
        }
        sp_wave_sync();                                                   // the next span overwrites P
    }
}

// the spans k_sp_level leaves alone, ONE BLOCK per span: one arg-max pass over global memory, four points per thread in flight, the waves' winners combined
// in LDS; thread 0 sets the flag and appends the children that have an interior to the next list with one atomicAdd
__global__ __launch_bounds__(256) void k_sp_long(const int2* __restrict__ pts, const int2* __restrict__ cur, int2* __restrict__ nxt, unsigned cap, SpState* st, int ci, int ni,
                                                 u64 tol4sq, uint8_t* __restrict__ keep, int total) {
    __shared__ u64 w_hi[SP_WAVES], w_lo[SP_WAVES];
    __shared__ int w_idx[SP_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned count = min(st->cnt[ci], cap);
    for (unsigned k = blockIdx.x; k < count; k += gridDim.x) {                // k, and with it the span, is the same in the whole block
        const int2 sp = cur[k];
        const int a = sp.x, b = sp.y;
        if (a < 0 || b >= total || b - a < SP_S) continue;
        const SpChord c = sp_chord(pts[a], pts[b]);
        u128 K = 0; int m = INT_MAX;
        int i = a + 1 + (int)threadIdx.x;                                     // a thread's points ascend, so its first maximum is its lowest index
        for (; i + 768 < b; i += 1024) {
            const int2 p0 = pts[i], p1 = pts[i + 256], p2 = pts[i + 512], p3 = pts[i + 768];
            u128 q = sp_key(c, p0); if (q > K) { K = q; m = i; }
            q = sp_key(c, p1); if (q > K) { K = q; m = i + 256; }
            q = sp_key(c, p2); if (q > K) { K = q; m = i + 512; }
            q = sp_key(c, p3); if (q > K) { K = q; m = i + 768; }
        }
        for (; i < b; i += 256) { const u128 q = sp_key(c, pts[i]); if (q > K) { K = q; m = i; } }
        sp_wave_max(K, m);
        if (lane == 0) { w_hi[w] = (u64)(K >> 64); w_lo[w] = (u64)K; w_idx[w] = m; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int v = 1; v < SP_WAVES; v++) {
                const u128 q = ((u128)w_hi[v] << 64) | w_lo[v];
                if (q > K || (q == K && w_idx[v] < m)) { K = q; m = w_idx[v]; }
            }
            if (sp_kept(c, K, tol4sq) && m > a && m < b) {
                keep[m] = 1;
                const bool left = m - a >= 2, right = b - m >= 2;
                const unsigned add = (unsigned)left + (unsigned)right;
                if (add) {
                    const unsigned at = atomicAdd(&st->cnt[ni], add);
                    if (at > cap || add > cap - at) atomicOr(&st->bad, 4u);
                    else { unsigned q = at; if (left) nxt[q++] = make_int2(a, m); if (right) nxt[q] = make_int2(m, b); }
                }
            }
        }
        __syncthreads();                                                      // the next span overwrites the winners
    }
}

struct SpFlag { __device__ unsigned operator()(uint8_t v) const { return v ? 1u : 0u; } };

__global__ __launch_bounds__(256) void k_sp_offs(const long long* __restrict__ off, int n, long long total, const unsigned* __restrict__ pos, long long* __restrict__ out_off, SpState* st) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    const long long a = off[p];
    if (a < 0 || a > total) { atomicOr(&st->bad, 8u); out_off[p] = 0; return; }
    out_off[p] = (long long)pos[a];
}
__global__ __launch_bounds__(256) void k_sp_emit(const int2* __restrict__ pts, long long total, const uint8_t* __restrict__ keep, const unsigned* __restrict__ pos, int2* __restrict__ out,
                                                 long long* __restrict__ kept) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total || !keep[i]) return;
    const unsigned q = pos[i];
    if ((long long)q < total) { out[q] = pts[i]; kept[q] = i; }
}
}  // namespace

// include/orip.h states the rule; the simplified polylines become the resident step polylines
extern "C" int orip_gcode_simplify(orip_ctx* c, const int64_t* off, const int32_t* pts, int64_t n, int32_t tol4, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats) ORIP_FAIL(c, "bad arguments");
    if (tol4 < 0 || tol4 > ORIP_SIMPLIFY_TOL4_MAX) ORIP_FAIL(c, "tolerance %d quarter steps: 0..2^17 - 1", tol4);
    int64_t total;
    ORIP_TRY(gc_steps_check(c, __func__, off, pts, n, true, total));
    hipStream_t s = LN(c).stream;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    const bool same_count = c->gc_ready && c->gc_n == n;                      // as many as the sources name: taken for the polylines a fetch gave out
    if (n == 0) {                                                             // nothing to launch; the explicit form leaves the empty list resident
        if (off) { ORIP_TRY(gc_publish_empty(c, __func__)); if (!same_count) c->gc_merged = true; }
        c->sp_points = 0;
        return 0;
    }
    const int N = (int)n;
    const size_t T = (size_t)total;
    const unsigned cap = (unsigned)std::max<int64_t>(n, 2 * (total / SP_S) + 2);
    uint8_t* keep; unsigned* pos; int2* list; SpState* st;
    { Carve L; L.take(keep, T + 1); L.take(pos, T + 1); L.take(list, 2 * (size_t)cap); L.take(st, 1); HIPC(c, L.commit(c->sp_tmp, 64)); }
    HIPC(c, c->sp_off.ensure(((size_t)N + 1) * 8 + 64)); HIPC(c, c->sp_pts.ensure(T * 8 + 64));                   // the output is never larger than the input
    HIPC(c, c->sp_res.ensure(T * 8 + 64));
    c->sp_points = -1;
    if (off) ORIP_TRY(gc_steps_upload(c, __func__, off, pts, n, total));      // checked above: from here on the input is the resident list
    if (off && !same_count) c->gc_merged = true;                              // the sources do not name these polylines
    HIPC(c, hipMemsetAsync(keep, 0, T + 1, s));
    HIPC(c, hipMemsetAsync(st, 0, sizeof(SpState), s));
    const long long* d_off = c->gc_off.as<long long>(); const int2* d_pts = c->gc_pts.as<int2>();
    const u64 tol4sq = (u64)tol4 * (u64)tol4;
    const dim3 b(256);
    hipLaunchKernelGGL(k_sp_seed, dim3(cdiv(N, 256)), b, 0, s, d_off, N, (long long)total, list, keep, st);
    SpState h = {{0, 0, 0}, 0, 0};
    int r = 0;                                                                // levels enqueued
    do {
        { ProfScope ps(c, "k_sp_level");
          for (int k = 0; k < SP_BATCH; k++, r++) {
              const int2 *cur = list + (size_t)(r & 1) * cap; int2* nxt = list + (size_t)((r + 1) & 1) * cap;
              hipLaunchKernelGGL(k_sp_level, dim3(SP_BLOCKS), b, 0, s, d_pts, cur, cap, st, r % 3, (r + 2) % 3, r > 0 ? 1 : 0, tol4sq, keep, (int)total);
              if (total > SP_S) hipLaunchKernelGGL(k_sp_long, dim3(SP_LONG_BLOCKS), b, 0, s, d_pts, cur, nxt, cap, st, r % 3, (r + 1) % 3, tol4sq, keep, (int)total);
          } }
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(&h, st, sizeof(SpState), hipMemcpyDeviceToHost, s));
        HIPC(c, hipStreamSynchronize(s));                                     // one look per batch
    } while (h.cnt[r % 3] != 0 && !h.bad);
    if (h.bad) { gc_drop(c); ORIP_FAIL(c, "the spans do not add up (internal error %u)", h.bad); }
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, rocprim::make_transform_iterator(keep, SpFlag()), pos, 0u, T + 1, rocprim::plus<unsigned>(), s); }));
    hipLaunchKernelGGL(k_sp_offs, dim3(cdiv((int64_t)N + 1, 256)), b, 0, s, d_off, N, (long long)total, pos, c->sp_off.as<long long>(), st);
    { ProfScope ps(c, "k_sp_emit");
      hipLaunchKernelGGL(k_sp_emit, dim3(cdiv(total, 256)), b, 0, s, d_pts, (long long)total, keep, pos, c->sp_pts.as<int2>(), c->sp_res.as<long long>()); }
    HIPC(c, hipGetLastError());
    unsigned points = 0;
    HIPC(c, hipMemcpyAsync(&points, pos + T, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h, st, sizeof(SpState), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (h.bad || (int64_t)points > total || (int64_t)points < 2 * n) { gc_drop(c); ORIP_FAIL(c, "the kept points do not add up (internal error %u)", h.bad); }
    gc_publish(c, c->sp_off, c->sp_pts, n, points);
    c->sp_points = points;
    stats[0] = n; stats[1] = total; stats[2] = points; stats[3] = h.rounds;
    return 0;
}

extern "C" int orip_gcode_simplify_fetch(orip_ctx* c, int64_t* kept) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (c->sp_points < 0) ORIP_FAIL(c, "no simplification: orip_gcode_simplify has not succeeded since the last failure");
    if (c->sp_points == 0) return 0;
    if (!kept) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(kept, c->sp_res.p, (size_t)c->sp_points * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
