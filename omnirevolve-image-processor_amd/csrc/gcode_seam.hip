// csrc/gcode_seam.hip -- --loop-start of gcode2stream.py / svg2stream.py: where every closed stroke of a drawing sequence is entered and left
// (orip_gcode_seam; the rule is stated in include/orip.h and has one answer for every input).  Ours: the reference has no such pass.
//
// Positions k = 0 .. n - 1 of the sequence; stroke order[k] is CLOSED when it has 4 points or more and ends where it starts, and then has the ring
// vertices 0 .. L - 2 of its stored points.  A RUN is a maximal stretch of closed positions.  The answer of a run does not depend on any other run: the
// open stroke (or the start, or nothing) on either side fixes the point the pen comes from and the point it goes to.
//
// Backward, per run, from its last position hi to its first lo: the cost-to-go f_k[v], int64, one value per ring vertex, all rings in one array (ring k at
// fo_k = the ring sizes before it, summed).  f_hi[v] = d(v, entry of hi + 1), or 0 when the sequence ends there; f_k[v] = min_u d(v, u) + f_{k+1}[u]: a
// LAYER, a min-plus product of R_k x R_{k+1} pairs.  Forward, per run: seam_k = the lowest v that attains min_v d(cursor, v) + f_k[v]; the cursor moves on
// to that vertex.  The lowest index at every step, in drawing order, is the lexicographically smallest of the assignments with the least travel.
//
// 32 bits in the inner loop.  f_k is 1-Lipschitz in d (a minimum of functions that are, by the triangle inequality; d(v, a) and 0 are too), so inside one
// ring f[u] - f[0] lies in [-2^30, 2^30].  A layer stages (x, y, F = f[u] - f[0] + 2^30) of the next ring in LDS, F in [0, 2^31], and a pair costs
// max(|dx|, |dy|) + F <= 3 * 2^30 in unsigned 32 bits: nine vector operations (|a - b| is a max, a min and a subtract), none of them 64-bit.  The
// int64 comes back when the vertex's minimum is stored.
//
// Kernels, all on the lane's stream, whose order is the only barrier between them:
//   k_sm_classify  thread per position: ring size (0 = open), where the stroke's points start, entry and exit (of a closed stroke: vertex 0, the seam
//                  it has), seam 0
//   k_sm_flags     thread per position: (ring size, run starts here, the layer k -> k + 1 is LARGE: R_k * R_{k+1} >= SM_HAND_OVER), scanned by rocPRIM
//   k_sm_runs      thread per position: first and last position of every run, by the run's number
//   k_sm_depth     thread per position: dep[k] = the large layers between k and the end of its run, k's own included; the large layers as a list
//                  (k, dep, R_k, R_{k+1})
//   k_sm_back      block per run and LEVEL d: the stretch of the run with dep == d, downwards.  Its top is the run's last ring (d = 0: f from the rule's
//                  end) or a large layer (d > 0: k_sm_layer has written it); every layer below the top is short, and the block walks them without a
//                  host round trip: a vertex or two per thread, the next ring through LDS 512 at a time, every lane reading the same entry (a broadcast).
//   k_sm_layer     one large layer over many blocks, 512 vertices each; blockIdx.y picks the layer among those of one level, which lie in different runs
//   k_sm_forward   wave per run: the lowest argmin per ring, 64 vertices at a time, (cost, vertex) reduced by shuffles; writes seam and the new entry / exit
//   k_sm_travel    the travel of the whole sequence from the start, before and after
// The host reads back once, behind k_sm_depth: the ring vertices of all runs (f's size), the number of runs, the large layers with their levels.  Then level
// 0, and per further level its large layers and k_sm_back again.  Without a large layer that is one launch backward and one forward, whatever n is.
//
// Scratch, free between calls: c->sm_state = the arrays below, all by position; c->sm_in = off / pts of an explicit input (the resident list is only
// read, and an explicit input does not become the resident one); c->sm_f = f.
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <vector>

namespace {
#ifndef SM_HAND_OVER_PAIRS
#define SM_HAND_OVER_PAIRS (1ll << 20)              // make EXTRA=-DSM_HAND_OVER_PAIRS=... builds another one for tools/time_seam.py --hand-over
#endif
constexpr long long SM_HAND_OVER = SM_HAND_OVER_PAIRS;      // pairs of one layer from which it gets blocks of its own (tests/seam_cases.py: HAND_OVER)
constexpr int SM_TILE = 512;                       // entries of the next ring staged at a time
constexpr int SM_CHUNK = 512;                      // vertices a block of 256 takes at a time: two per thread
constexpr unsigned SM_BIAS = 1u << 30;

struct SmScan { long long r; int h, l; };          // ring vertices, runs started, large layers: summed side by side
struct SmAdd { __device__ SmScan operator()(const SmScan& a, const SmScan& b) const { return SmScan{a.r + b.r, a.h + b.h, a.l + b.l}; } };
struct SmCounters { unsigned long long closed, moved, travel[2]; int bad, pad; };

__device__ __forceinline__ unsigned sm_d(int px, int py, int qx, int qy) { return max(__usad((unsigned)px, (unsigned)qx, 0u), __usad((unsigned)py, (unsigned)qy, 0u)); }

__global__ __launch_bounds__(256) void k_sm_classify(const long long* __restrict__ off, const int2* __restrict__ pts, long long total, const int* __restrict__ ord,
                                                     const uint8_t* __restrict__ rv, int n, long long* __restrict__ base, int* __restrict__ ring, int4* __restrict__ ab,
                                                     int* __restrict__ seam, SmCounters* __restrict__ cnt) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int p = ord ? ord[k] : k;
    long long a = 0, b = 0;
    if ((unsigned)p < (unsigned)n) { a = off[p]; b = off[p + 1]; }
    if (a < 0 || b - a < 2 || b > total || b - a >= (1ll << 30)) {           // checked on the host or kept by the writers of the resident list; the bound only states it
        cnt->bad = 1; base[k] = 0; ring[k] = 0; ab[k] = make_int4(0, 0, 0, 0); seam[k] = 0;
        return;
    }
    const int2 A = pts[a], B = pts[b - 1];
    const bool closed = b - a >= 4 && A.x == B.x && A.y == B.y;
    base[k] = a; ring[k] = closed ? (int)(b - a - 1) : 0; seam[k] = 0;
    ab[k] = (rv && rv[k]) ? make_int4(B.x, B.y, A.x, A.y) : make_int4(A.x, A.y, B.x, B.y);
}

__global__ __launch_bounds__(256) void k_sm_flags(const int* __restrict__ ring, int n, SmScan* __restrict__ in) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int r = ring[k], before = k > 0 ? ring[k - 1] : 0, after = k + 1 < n ? ring[k + 1] : 0;
    in[k] = SmScan{(long long)r, (r > 0 && before == 0) ? 1 : 0, ((long long)r * after >= SM_HAND_OVER) ? 1 : 0};
}

__global__ __launch_bounds__(256) void k_sm_runs(const int* __restrict__ ring, const SmScan* __restrict__ sc, int n, int* __restrict__ run_lo, int* __restrict__ run_hi) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n || ring[k] == 0) return;
    const int run = sc[k].h - 1;
    if (k == 0 || ring[k - 1] == 0) run_lo[run] = k;
    if (k == n - 1 || ring[k + 1] == 0) run_hi[run] = k;
}

__global__ __launch_bounds__(256) void k_sm_depth(const int* __restrict__ ring, const SmScan* __restrict__ in, const SmScan* __restrict__ sc, const int* __restrict__ run_hi, int n,
                                                  int* __restrict__ dep, int4* __restrict__ big) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    if (ring[k] == 0) { dep[k] = 0; return; }
    const int d = sc[run_hi[sc[k].h - 1]].l - sc[k].l + in[k].l;
    dep[k] = d;
    if (in[k].l) big[sc[k].l - 1] = make_int4(k, d, ring[k], ring[k + 1]);
}

// one chunk of the layer k -> next: f[fo + v] for v = v0 + threadIdx.x and, in a ring that reaches that far, v0 + 256 + threadIdx.x.  Every thread of the block calls it.
__device__ __forceinline__ void sm_chunk(const int2* __restrict__ pts, long long* f, long long bk, int R, long long fo, long long bn, int Rn, long long fon, int v0, int4* s_t) {
    int x[2], y[2]; unsigned best[2]; bool live[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int v = v0 + j * 256 + (int)threadIdx.x;
        live[j] = v < R; best[j] = ~0u; x[j] = 0; y[j] = 0;
        if (live[j]) { const int2 P = pts[bk + v]; x[j] = P.x; y[j] = P.y; }
    }
    const long long ref = f[fon];
    const bool two = v0 + 256 < R;                                            // the same in every thread
    for (int u0 = 0; u0 < Rn; u0 += SM_TILE) {
        const int cnt = min(SM_TILE, Rn - u0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) { const int2 P = pts[bn + u0 + t]; s_t[t] = make_int4(P.x, P.y, (int)(unsigned)(f[fon + u0 + t] - ref + (long long)SM_BIAS), 0); }
        __syncthreads();
        if (two) {
#pragma unroll 8
            for (int t = 0; t < cnt; t++) {
                const int4 G = s_t[t];
                best[0] = min(best[0], sm_d(x[0], y[0], G.x, G.y) + (unsigned)G.z);
                best[1] = min(best[1], sm_d(x[1], y[1], G.x, G.y) + (unsigned)G.z);
            }
        } else {
#pragma unroll 8
            for (int t = 0; t < cnt; t++) { const int4 G = s_t[t]; best[0] = min(best[0], sm_d(x[0], y[0], G.x, G.y) + (unsigned)G.z); }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++) if (live[j]) f[fo + v0 + j * 256 + (int)threadIdx.x] = (long long)best[j] - (long long)SM_BIAS + ref;
}

__global__ __launch_bounds__(256) void k_sm_back(const int2* __restrict__ pts, const long long* __restrict__ base, const int* __restrict__ ring, const SmScan* __restrict__ sc,
                                                 const int* __restrict__ run_lo, const int* __restrict__ run_hi, const int* __restrict__ dep, const int4* __restrict__ ab,
                                                 int n, int level, long long* f) {
    __shared__ int4 s_t[SM_TILE];
    const int lo = run_lo[blockIdx.x], hi = run_hi[blockIdx.x];
    if ((unsigned)lo >= (unsigned)n || (unsigned)hi >= (unsigned)n || lo > hi || dep[lo] < level) return;      // no stretch of this level; the rest only states the bound
    // dep does not increase along the run and falls by one at a time: the stretch is first .. top
    int a = lo, b = hi;
    while (a < b) { const int m = (a + b) >> 1; if (dep[m] <= level) b = m; else a = m + 1; }
    const int first = a;
    a = lo; b = hi;
    while (a < b) { const int m = (a + b + 1) >> 1; if (dep[m] >= level) a = m; else b = m - 1; }
    const int top = a;
    if (level == 0) {                                                         // top == hi: the end of the rule
        const int R = ring[top]; const long long bk = base[top], fo = sc[top].r - R;
        const bool more = top + 1 < n;
        int ax = 0, ay = 0;
        if (more) { const int4 e = ab[top + 1]; ax = e.x; ay = e.y; }
        for (int v = threadIdx.x; v < R; v += 256) { const int2 P = pts[bk + v]; f[fo + v] = more ? (long long)sm_d(P.x, P.y, ax, ay) : 0ll; }
        __syncthreads();
    }
    for (int k = top - 1; k >= first; k--) {
        const int R = ring[k], Rn = ring[k + 1];
        const long long bk = base[k], bn = base[k + 1], fo = sc[k].r - R, fon = sc[k + 1].r - Rn;
        for (int v0 = 0; v0 < R; v0 += SM_CHUNK) sm_chunk(pts, f, bk, R, fo, bn, Rn, fon, v0, s_t);
        __syncthreads();                                                      // f_k is read by every thread of the next layer
    }
}

__global__ __launch_bounds__(256) void k_sm_layer(const int2* __restrict__ pts, const long long* __restrict__ base, const int* __restrict__ ring, const SmScan* __restrict__ sc,
                                                  const int4* __restrict__ big, int first, int n, long long* f) {
    __shared__ int4 s_t[SM_TILE];
    const int k = big[first + blockIdx.y].x;
    if ((unsigned)k >= (unsigned)(n - 1)) return;                             // a list entry that names no layer: never, the bound only states it
    const int R = ring[k], Rn = ring[k + 1], v0 = blockIdx.x * SM_CHUNK;
    if (v0 >= R || Rn <= 0) return;
    sm_chunk(pts, f, base[k], R, sc[k].r - R, base[k + 1], Rn, sc[k + 1].r - Rn, v0, s_t);
}

__global__ __launch_bounds__(64) void k_sm_forward(const int2* __restrict__ pts, const long long* __restrict__ base, const int* __restrict__ ring, const SmScan* __restrict__ sc,
                                                   const int* __restrict__ run_lo, const int* __restrict__ run_hi, int n, int sx, int sy, const long long* __restrict__ f,
                                                   int4* __restrict__ ab, int* __restrict__ seam, SmCounters* __restrict__ cnt) {
    const int lo = run_lo[blockIdx.x], hi = run_hi[blockIdx.x];
    if ((unsigned)lo >= (unsigned)n || (unsigned)hi >= (unsigned)n || lo > hi) return;
    int cx = sx, cy = sy, moved = 0;
    if (lo > 0) { const int4 e = ab[lo - 1]; cx = e.z; cy = e.w; }
    for (int k = lo; k <= hi; k++) {
        const int R = ring[k]; const long long bk = base[k], fo = sc[k].r - R;
        long long bc = INT64_MAX; int bv = INT32_MAX;
        for (int v = threadIdx.x; v < R; v += 64) {                           // v ascends: a strict < keeps the lane's lowest
            const int2 P = pts[bk + v];
            const long long cost = (long long)sm_d(cx, cy, P.x, P.y) + f[fo + v];
            if (cost < bc) { bc = cost; bv = v; }
        }
        for (int o = 32; o; o >>= 1) {
            const long long c2 = __shfl_xor(bc, o); const int v2 = __shfl_xor(bv, o);
            if (c2 < bc || (c2 == bc && v2 < bv)) { bc = c2; bv = v2; }
        }
        if ((unsigned)bv >= (unsigned)R) bv = 0;                              // never: a ring has three vertices at least
        const int2 P = pts[bk + bv];
        if (threadIdx.x == 0) { seam[k] = bv; ab[k] = make_int4(P.x, P.y, P.x, P.y); }
        moved += bv != 0;
        cx = P.x; cy = P.y;
    }
    if (threadIdx.x == 0) { atomicAdd(&cnt->closed, (unsigned long long)(hi - lo + 1)); atomicAdd(&cnt->moved, (unsigned long long)moved); }
}

// the travel of the whole sequence from (sx, sy)
__global__ __launch_bounds__(256) void k_sm_travel(const int4* __restrict__ ab, int n, int sx, int sy, unsigned long long* out) {
    __shared__ unsigned long long part[4];
    const int k = blockIdx.x * 256 + threadIdx.x;
    unsigned long long v = 0;
    if (k < n) {
        const int4 e = ab[k];
        int bx = sx, by = sy;
        if (k > 0) { const int4 q = ab[k - 1]; bx = q.z; by = q.w; }
        v = sm_d(bx, by, e.x, e.y);
    }
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}
}  // namespace

// include/orip.h states the rule
extern "C" int orip_gcode_seam(orip_ctx* c, const int64_t* off, const int32_t* pts, int64_t n, const int32_t* order, const uint8_t* rev, const int32_t* start_xy,
                               int32_t* seam_out, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats || (n > 0 && !seam_out)) ORIP_FAIL(c, "bad arguments");
    if (n < 0 || n > (1 << 26)) ORIP_FAIL(c, "%lld paths: 0..2^26", (long long)n);
    int sx, sy;
    ORIP_TRY(gc_check_start(c, __func__, start_xy, sx, sy));
    if (n == 0) { for (int k = 0; k < 4; k++) stats[k] = 0; return 0; }
    int64_t total = 0;
    ORIP_TRY(gc_steps_check(c, __func__, off, pts, n, false, total));
    if (order) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int64_t k = 0; k < n; k++) {
            const int64_t p = order[k];
            if (p < 0 || p >= n || seen[(size_t)p]) ORIP_FAIL(c, "position %lld: the order is not a permutation (path %lld)", (long long)k, (long long)p);
            seen[(size_t)p] = 1;
        }
    }
    for (int64_t k = 0; rev && k < n; k++) if (rev[k] > 1) ORIP_FAIL(c, "position %lld: direction %d is neither 0 nor 1", (long long)k, (int)rev[k]);
    hipStream_t s = LN(c).stream;
    const int N = (int)n;
    long long* base; int *ring, *ord, *run_lo, *run_hi, *dep, *seam; int4 *ab, *big; SmScan *in, *sc; uint8_t* rv; SmCounters* cnt;
    { Carve L; L.take(base, (size_t)N); L.take(in, (size_t)N); L.take(sc, (size_t)N); L.take(ab, (size_t)N); L.take(big, (size_t)N); L.take(ring, (size_t)N); L.take(ord, (size_t)N);
      L.take(run_lo, (size_t)N); L.take(run_hi, (size_t)N); L.take(dep, (size_t)N); L.take(seam, (size_t)N); L.take(rv, (size_t)N); L.take(cnt, 1);
      HIPC(c, L.commit(c->sm_state, 64)); }
    const long long* d_off = c->gc_off.as<long long>(); const int2* d_pts = c->gc_pts.as<int2>();
    if (off) {                                                                // an explicit input goes to this pass's own buffer: the resident list stays what it was
        long long* o2; int2* p2;
        { Carve L; L.take(o2, (size_t)N + 1); L.take(p2, (size_t)total); HIPC(c, L.commit(c->sm_in, 64)); }
        HIPC(c, hipMemcpyAsync(o2, off, (size_t)(N + 1) * 8, hipMemcpyHostToDevice, s));
        HIPC(c, hipMemcpyAsync(p2, pts, (size_t)total * 8, hipMemcpyHostToDevice, s));
        d_off = o2; d_pts = p2;
    }
    if (order) HIPC(c, hipMemcpyAsync(ord, order, (size_t)N * 4, hipMemcpyHostToDevice, s));
    if (rev) HIPC(c, hipMemcpyAsync(rv, rev, (size_t)N, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(cnt, 0, sizeof(SmCounters), s));
    const dim3 b(256), gn(cdiv(N, 256));
    { ProfScope ps(c, "k_sm_prepare");
      hipLaunchKernelGGL(k_sm_classify, gn, b, 0, s, d_off, d_pts, (long long)total, order ? ord : (const int*)nullptr, rev ? rv : (const uint8_t*)nullptr, N, base, ring, ab, seam, cnt);
      hipLaunchKernelGGL(k_sm_travel, gn, b, 0, s, ab, N, sx, sy, &cnt->travel[0]);
      hipLaunchKernelGGL(k_sm_flags, gn, b, 0, s, ring, N, in);
      HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::inclusive_scan(tmp, bytes, in, sc, (size_t)N, SmAdd(), s); }));
      hipLaunchKernelGGL(k_sm_runs, gn, b, 0, s, ring, sc, N, run_lo, run_hi);
      hipLaunchKernelGGL(k_sm_depth, gn, b, 0, s, ring, in, sc, run_hi, N, dep, big); }
    HIPC(c, hipGetLastError());
    SmScan sum; SmCounters hc;
    HIPC(c, hipMemcpyAsync(&sum, sc + (N - 1), sizeof sum, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&hc, cnt, sizeof hc, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (hc.bad || sum.r < 0 || sum.r > total || sum.h < 0 || sum.h > (N + 1) / 2 || sum.l < 0 || sum.l >= N) ORIP_FAIL(c, "the runs do not add up (internal error)");
    const int n_runs = sum.h, n_big = sum.l;
    if (n_runs > 0) {
        HIPC(c, c->sm_f.ensure((size_t)sum.r * 8 + 64));
        long long* f = c->sm_f.as<long long>();
        std::vector<int4> hb((size_t)n_big);
        int levels = 0;
        if (n_big > 0) {                                                      // by level, so that one launch takes the large layers of a level; they lie in different runs
            HIPC(c, hipMemcpyAsync(hb.data(), big, (size_t)n_big * 16, hipMemcpyDeviceToHost, s));
            HIPC(c, hipStreamSynchronize(s));
            for (const int4& e : hb) {
                if (e.x < 0 || e.x >= N - 1 || e.y < 1 || e.y > n_big || e.z < 3 || e.z >= (1 << 30)) ORIP_FAIL(c, "the large layers do not add up (internal error)");
                levels = std::max(levels, e.y);
            }
            std::stable_sort(hb.begin(), hb.end(), [](const int4& p, const int4& q) { return p.y < q.y; });
            HIPC(c, hipMemcpyAsync(big, hb.data(), (size_t)n_big * 16, hipMemcpyHostToDevice, s));
        }
        { ProfScope ps(c, "k_sm_back");
          hipLaunchKernelGGL(k_sm_back, dim3(n_runs), b, 0, s, d_pts, base, ring, sc, run_lo, run_hi, dep, ab, N, 0, f);
          size_t at = 0;
          for (int level = 1; level <= levels; level++) {
              size_t end = at;
              while (end < hb.size() && hb[end].y == level) end++;
              for (size_t i = at; i < end; i += 32768) {                      // every layer of the launch gets the blocks of the widest ring among them
                  const int rows = (int)std::min<size_t>(32768, end - i);
                  int widest = 1;
                  for (int r = 0; r < rows; r++) widest = std::max(widest, cdiv(hb[i + r].z, SM_CHUNK));
                  hipLaunchKernelGGL(k_sm_layer, dim3(widest, rows), b, 0, s, d_pts, base, ring, sc, big, (int)i, N, f);
              }
              at = end;
              hipLaunchKernelGGL(k_sm_back, dim3(n_runs), b, 0, s, d_pts, base, ring, sc, run_lo, run_hi, dep, ab, N, level, f);
          } }
        { ProfScope ps(c, "k_sm_forward");
          hipLaunchKernelGGL(k_sm_forward, dim3(n_runs), dim3(64), 0, s, d_pts, base, ring, sc, run_lo, run_hi, N, sx, sy, f, ab, seam, cnt); }
    }
    hipLaunchKernelGGL(k_sm_travel, gn, b, 0, s, ab, N, sx, sy, &cnt->travel[1]);
    HIPC(c, hipGetLastError());
    std::vector<int32_t> hs((size_t)N);
    HIPC(c, hipMemcpyAsync(&hc, cnt, sizeof hc, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(hs.data(), seam, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (hc.travel[1] > hc.travel[0] || hc.moved > hc.closed || hc.closed > (unsigned long long)N) ORIP_FAIL(c, "the counts do not add up (internal error)");
    memcpy(seam_out, hs.data(), (size_t)N * 4);
    stats[0] = (int64_t)hc.closed; stats[1] = (int64_t)hc.moved; stats[2] = (int64_t)hc.travel[0]; stats[3] = (int64_t)hc.travel[1];
    return 0;
}
