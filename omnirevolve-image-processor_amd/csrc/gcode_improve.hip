// csrc/gcode_improve.hip -- --improve-order of gcode2stream.py / svg2stream.py: 2-opt and or-opt on a drawing sequence (orip_gcode_improve; the rule is stated
// in include/orip.h and has one answer for every input).  Ours: the reference stops at the greedy order.
//
// State: the whole sequence in position order, twice (buffers 0 and 1 of ImState): ab int4[n] = (a.x, a.y, b.x, b.y), the point where the stroke at a position
// is entered and the point where it is left, and id int[n] = stroke | reversed << 31.  A group owns the positions base .. base + m - 1.  link(k) is not kept:
// it is d(b_{k-1}, a_k) of two neighbouring rows and is worked out where a row is staged, which is cheaper than a third array every move would rewrite.
// Buffer 0 holds every group before its turn and after it (a group that ends in buffer 1 is copied back), so the cursor of a group is ab[0][base - 1].b.
//
// The GAP g = 0 .. m of a group lies in front of position g: (b_{g-1}, a_g, link(g), mask), with b_{-1} the cursor and, for g = m, no a_m: link 0 and
// mask 0, which blanks every distance to a_m.  Both kinds of move are a stroke i and a gap g:
//     R(i, j),  g = j + 1 > i:            P = link(i) + link(g)               N = d(b_{i-1}, b_{g-1}) + d(a_i, a_g)
//     M(i, L, p), g = p + 1, g - i not in 0 .. L, i + L <= m:
//                                          P = link(i) + link(i + L) + link(g) N = d(b_{i-1}, a_{i+L}) + d(b_{g-1}, a_i) + d(b_{i+L-1}, a_g)
// gain = P - N.  P and N are sums of at most three distances of at most 2^30 and fit unsigned 32 bits; their difference does not fit int32.  Only a positive
// gain is ever applied, so the kernel keeps max(P - N, 0) as unsigned: P - min(P, N).  0 = no move.
//
// One round = two launches on the lane's stream, and the stream's order is the only grid-wide barrier:
//   k_im_eval   block (x, y): thread x * 256 + t owns stroke i and keeps b_{i-1}, a_i, link(i) and for L = 1 .. 3 (b_{i+L-1}, P and N of the removal) in
//               registers; the gaps of chunk y go through LDS 256 at a time, every lane reads the same gap (a broadcast, no bank conflict).  6 distances and 4
//               candidates per (i, g), 4 and 3 without ORIP_ORDER_REVERSE.  g ascends, so per code a strict > keeps the lowest second index; the four codes, the wave and the block are reduced
//               by (gain desc, key asc), key = code << 34 | i << 17 | g: one ImRec per block.  Nothing is packed into one word with the gain.
//   k_im_apply  every block reduces the records again (the same answer in every block), then block 0 writes the next status and, when the gain is positive,
//               every thread writes one row of the other buffer: new[k] = old[f(k)], f the position map of the move; R also swaps a and b and flips the bit.
// Status: ImStatus[2], read at [round & 1] and written at [(round + 1) & 1], so no block reads a word another block of the same launch writes.  Launches
// behind `done` (converged, or the cap reached) change nothing but that copy.  The host enqueues IM_BATCH rounds, reads the 24 bytes, and goes on until done:
// no host sync per round, and the result does not depend on IM_BATCH.
//
// Scratch, free between calls: c->im_state = se int4[n] (the ends, uploaded or taken from the resident polylines), ord int[n], rv u8[n] (the given sequence),
// ab int4[2][n], id int[2][n]; c->im_rec = ImRec[IM_MAX_REC], ImStatus[2], travel u64[2].
#include "orip_ctx.h"
#include "gc_convert.h"

namespace {
constexpr int IM_BATCH = 32;                       // rounds between two looks at the status word
constexpr int IM_TILE = 256;                       // gaps staged at a time = threads of a block
constexpr int IM_BLOCKS = 2048;                    // blocks k_im_eval aims for: 8 per CU
constexpr int IM_MAX_REC = 4096;

struct ImRec { unsigned gain, pad; unsigned long long key; };
struct ImStatus { int done, converged, cur, pad; long long rounds; };
struct ImState { int4* ab[2]; int* id[2]; };

__device__ __forceinline__ unsigned im_d(int px, int py, int qx, int qy) { return (unsigned)max(abs(px - qx), abs(py - qy)); }
__device__ __forceinline__ bool im_better(unsigned g1, unsigned long long k1, unsigned g2, unsigned long long k2) { return g1 > g2 || (g1 == g2 && k1 < k2); }

// (gain, key) of the block's best in every thread; red: 2 * 4 words of LDS
__device__ __forceinline__ void im_block_best(unsigned& g, unsigned long long& k, unsigned* red_g, unsigned long long* red_k) {
    for (int o = 32; o; o >>= 1) {
        const unsigned g2 = __shfl_xor(g, o); const unsigned long long k2 = __shfl_xor(k, o);
        if (im_better(g2, k2, g, k)) { g = g2; k = k2; }
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();                                                          // red may still be read from the call before
    if ((threadIdx.x & 63) == 0) { red_g[w] = g; red_k[w] = k; }
    __syncthreads();
    g = red_g[0]; k = red_k[0];
    for (int i = 1; i < IM_TILE / 64; i++) if (im_better(red_g[i], red_k[i], g, k)) { g = red_g[i]; k = red_k[i]; }
}

// the sequence as given, in position order, into both buffers
__global__ __launch_bounds__(256) void k_im_init(const int4* __restrict__ se, const long long* __restrict__ off, const int2* __restrict__ pts, const int* __restrict__ ord,
                                                 const uint8_t* __restrict__ rv, int n, int4* __restrict__ ab0, int4* __restrict__ ab1, int* __restrict__ id0, int* __restrict__ id1) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int p = ord[k], r = rv[k] ? 1 : 0;
    if ((unsigned)p >= (unsigned)n) return;                                  // checked on the host; the bound only states it
    int4 e;
    if (se) e = se[p];
    else { const int2 a = pts[off[p]], b = pts[off[p + 1] - 1]; e = make_int4(a.x, a.y, b.x, b.y); }
    if (r) e = make_int4(e.z, e.w, e.x, e.y);
    const int id = p | (r << 31);
    ab0[k] = e; ab1[k] = e; id0[k] = id; id1[k] = id;
}

// the travel of the whole sequence from (sx, sy)
__global__ __launch_bounds__(256) void k_im_travel(const int4* __restrict__ ab, int n, int sx, int sy, unsigned long long* out) {
    __shared__ unsigned long long part[4];
    const int k = blockIdx.x * 256 + threadIdx.x;
    unsigned long long v = 0;
    if (k < n) {
        const int4 e = ab[k];
        int bx = sx, by = sy;
        if (k > 0) { const int4 q = ab[k - 1]; bx = q.z; by = q.w; }
        v = im_d(bx, by, e.x, e.y);
    }
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

// gap g of the group: (b_{g-1}, a_g) and (link(g), mask)
__device__ __forceinline__ void im_gap(const int4* __restrict__ ab, int m, int cx, int cy, int g, int4& pt, int2& lk) {
    int bx = cx, by = cy;
    if (g > 0) { const int4 q = ab[g - 1]; bx = q.z; by = q.w; }
    if (g < m) { const int4 e = ab[g]; pt = make_int4(bx, by, e.x, e.y); lk = make_int2((int)im_d(bx, by, e.x, e.y), -1); }
    else { pt = make_int4(bx, by, 0, 0); lk = make_int2(0, 0); }
}

__global__ __launch_bounds__(256) void k_im_eval(ImState S, int base, int m, int sx, int sy, int reverse, int chunk, long long cap,
                                                 const ImStatus* __restrict__ st, ImRec* __restrict__ rec) {
    __shared__ int4 s_pt[IM_TILE];
    __shared__ int2 s_lk[IM_TILE];
    __shared__ unsigned red_g[IM_TILE / 64];
    __shared__ unsigned long long red_k[IM_TILE / 64];
    const ImStatus now = *st;
    if (now.done || now.rounds >= cap) return;
    const int4* __restrict__ ab = S.ab[now.cur & 1] + base;
    int cx = sx, cy = sy;
    if (base > 0) { const int4 q = S.ab[0][base - 1]; cx = q.z; cy = q.w; }
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < m;
    // the stroke: gap i, and the three blocks that start at it
    int bix = 0, biy = 0, aix = 0, aiy = 0; unsigned li = 0;
    int bjx[3] = {0, 0, 0}, bjy[3] = {0, 0, 0}; unsigned remP[3] = {0, 0, 0}, remN[3] = {0, 0, 0}; bool okL[3] = {false, false, false};
    if (live) {
        int4 pt; int2 lk;
        im_gap(ab, m, cx, cy, i, pt, lk);
        bix = pt.x; biy = pt.y; aix = pt.z; aiy = pt.w; li = (unsigned)lk.x;
    }
#pragma unroll
    for (int L = 1; L <= 3; L++) {
        if (live && i + L <= m) {
            int4 pt; int2 lk;
            im_gap(ab, m, cx, cy, i + L, pt, lk);                             // (b_{i+L-1}, a_{i+L}, link(i+L), mask)
            okL[L - 1] = true; bjx[L - 1] = pt.x; bjy[L - 1] = pt.y;
            remP[L - 1] = li + (unsigned)lk.x; remN[L - 1] = im_d(bix, biy, pt.z, pt.w) & (unsigned)lk.y;
        }
    }
    unsigned bg[4] = {0, 0, 0, 0}; int bq[4] = {0, 0, 0, 0};
    const int g_lo = blockIdx.y * chunk, g_hi = min(g_lo + chunk, m + 1);     // this block's gaps
    for (int g0 = g_lo; g0 < g_hi; g0 += IM_TILE) {
        const int cnt = min(IM_TILE, g_hi - g0);
        __syncthreads();
        if ((int)threadIdx.x < cnt) { int4 pt; int2 lk; im_gap(ab, m, cx, cy, g0 + threadIdx.x, pt, lk); s_pt[threadIdx.x] = pt; s_lk[threadIdx.x] = lk; }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < cnt; t++) {
            const int4 G = s_pt[t]; const int2 K = s_lk[t];
            const int g = g0 + t, gi = g - i;
            const unsigned lg = (unsigned)K.x, mk = (unsigned)K.y;
            if (reverse) {   // R(i, g - 1); the flag is the same in every lane
                const unsigned P = li + lg, N = im_d(bix, biy, G.x, G.y) + (im_d(aix, aiy, G.z, G.w) & mk);
                const unsigned gn = (live && gi >= 1) ? P - min(P, N) : 0u;
                if (gn > bg[0]) { bg[0] = gn; bq[0] = g; }
            }
            const unsigned d3 = im_d(G.x, G.y, aix, aiy);
#pragma unroll
            for (int L = 1; L <= 3; L++) {   // M(i, L, g - 1)
                const unsigned P = remP[L - 1] + lg, N = remN[L - 1] + d3 + (im_d(bjx[L - 1], bjy[L - 1], G.z, G.w) & mk);
                const unsigned gn = (okL[L - 1] && (unsigned)gi > (unsigned)L) ? P - min(P, N) : 0u;
                if (gn > bg[L]) { bg[L] = gn; bq[L] = g; }
            }
        }
    }
    unsigned g = 0; unsigned long long k = ~0ull;
#pragma unroll
    for (int code = 0; code < 4; code++)
        if (bg[code] > g) { g = bg[code]; k = ((unsigned long long)code << 34) | ((unsigned long long)(unsigned)i << 17) | (unsigned)bq[code]; }
    im_block_best(g, k, red_g, red_k);
    if (threadIdx.x == 0) { ImRec r; r.gain = g; r.pad = 0; r.key = k; rec[blockIdx.y * gridDim.x + blockIdx.x] = r; }
}

__global__ __launch_bounds__(256) void k_im_apply(ImState S, int base, int m, long long cap, int n_rec, const ImRec* __restrict__ rec,
                                                  const ImStatus* __restrict__ st, ImStatus* __restrict__ st_next) {
    __shared__ unsigned red_g[IM_TILE / 64];
    __shared__ unsigned long long red_k[IM_TILE / 64];
    ImStatus now = *st;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (now.done || now.rounds >= cap) {                                      // nothing was evaluated: the records are stale
        now.done = 1;
        if (first) *st_next = now;
        return;
    }
    unsigned g = 0; unsigned long long key = ~0ull;
    for (int r = threadIdx.x; r < n_rec; r += 256) { const ImRec q = rec[r]; if (im_better(q.gain, q.key, g, key)) { g = q.gain; key = q.key; } }
    im_block_best(g, key, red_g, red_k);
    if (g == 0) {
        now.done = 1; now.converged = 1;
        if (first) *st_next = now;
        return;
    }
    const int code = (int)(key >> 34), i = (int)((key >> 17) & 0x1FFFF), gq = (int)(key & 0x1FFFF);
    const int cur = now.cur & 1;
    if (first) { now.cur = cur ^ 1; now.rounds++; *st_next = now; }
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    int f = k, flip = 0;
    if (code == 0) {
        const int j = gq - 1;
        if (k >= i && k <= j) { f = i + j - k; flip = 1; }
    } else {
        const int L = code, p = gq - 1, j = i + L - 1;
        if (p > j) {                                                          // the block goes towards the end: j + 1 .. p close up, then the block
            if (k >= i && k <= p - L) f = k + L;
            else if (k > p - L && k <= p) f = i + (k - (p - L + 1));
        } else {                                                              // towards the front (p <= i - 2): the block, then p + 1 .. i - 1 move up
            if (k > p && k <= p + L) f = i + (k - p - 1);
            else if (k > p + L && k <= j) f = k - L;
        }
    }
    if ((unsigned)f >= (unsigned)m) return;                                  // a decoded move that leaves the group: never, the bound only states it
    int4 e = S.ab[cur][base + f]; int id = S.id[cur][base + f];
    if (flip) { e = make_int4(e.z, e.w, e.x, e.y); id ^= (int)0x80000000u; }
    S.ab[cur ^ 1][base + k] = e; S.id[cur ^ 1][base + k] = id;
}
}  // namespace

// include/orip.h states the rule
extern "C" int orip_gcode_improve(orip_ctx* c, const int32_t* ends, const int32_t* group, int64_t n, int32_t n_groups, int32_t flags, const int32_t* start_xy, int64_t max_rounds,
                                  int32_t* order, uint8_t* rev, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats) ORIP_FAIL(c, "bad arguments");
    if (n < 0 || (n > 0 && (!group || !order || !rev)) || (flags & ~ORIP_ORDER_REVERSE)) ORIP_FAIL(c, "bad arguments");
    int sx, sy;
    ORIP_TRY(gc_check_groups(c, __func__, nullptr, 0, n_groups, nullptr));
    ORIP_TRY(gc_check_start(c, __func__, start_xy, sx, sy));
    if (max_rounds < 0) ORIP_FAIL(c, "%lld rounds: 0 or more, or ORIP_IMPROVE_ROUNDS_AUTO", (long long)max_rounds);
    for (int k = 0; k < 5; k++) stats[k] = 0;
    if (n == 0) return 0;
    if (!ends) ORIP_TRY(gc_check_resident(c, __func__, n));
    if (n > (1 << 26)) ORIP_FAIL(c, "%lld paths: at most 2^26", (long long)n);
    int64_t paths[ORIP_ORDER_MAX_GROUPS] = {0};
    ORIP_TRY(gc_check_groups(c, __func__, group, n, n_groups, paths));
    if (ends)
        for (int64_t i = 0; i < 4 * n; i++) if (ends[i] < 0 || ends[i] > GC_COORD_MAX) ORIP_FAIL(c, "path %lld: coordinate %d outside 0..2^30", (long long)(i / 4), ends[i]);
    const int reverse = flags & ORIP_ORDER_REVERSE ? 1 : 0;
    {   // the sequence: a permutation whose groups do not decrease, directions only with the flag
        std::vector<uint8_t> seen((size_t)n, 0);
        int last = 0;
        for (int64_t k = 0; k < n; k++) {
            const int64_t p = order[k];
            if (p < 0 || p >= n || seen[(size_t)p]) ORIP_FAIL(c, "position %lld: the order is not a permutation (path %lld)", (long long)k, (long long)p);
            seen[(size_t)p] = 1;
            if (group[p] < last) ORIP_FAIL(c, "position %lld: group %d behind group %d", (long long)k, group[p], last);
            last = group[p];
            if (rev[k] > 1 || (rev[k] && !reverse)) ORIP_FAIL(c, "position %lld: reversed without ORIP_ORDER_REVERSE", (long long)k);
        }
    }
    hipStream_t s = LN(c).stream;
    const int N = (int)n;
    int4 *se, *ab0, *ab1; int *ord, *id0, *id1; uint8_t* rv; ImRec* rec; ImStatus* st; unsigned long long* trav;
    { Carve L; L.take(se, (size_t)N); L.take(ab0, (size_t)N); L.take(ab1, (size_t)N); L.take(ord, (size_t)N); L.take(id0, (size_t)N); L.take(id1, (size_t)N); L.take(rv, (size_t)N);
      HIPC(c, L.commit(c->im_state, 64)); }
    { Carve L; L.take(rec, (size_t)IM_MAX_REC); L.take(st, 2); L.take(trav, 2); HIPC(c, L.commit(c->im_rec, 64)); }
    if (ends) HIPC(c, hipMemcpyAsync(se, ends, (size_t)N * 16, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(ord, order, (size_t)N * 4, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(rv, rev, (size_t)N, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemsetAsync(trav, 0, 16, s));
    const dim3 b(256), gn(cdiv(N, 256));
    hipLaunchKernelGGL(k_im_init, gn, b, 0, s, ends ? se : (const int4*)nullptr, c->gc_off.as<long long>(), c->gc_pts.as<int2>(), ord, rv, N, ab0, ab1, id0, id1);
    hipLaunchKernelGGL(k_im_travel, gn, b, 0, s, ab0, N, sx, sy, trav);
    ImState S; S.ab[0] = ab0; S.ab[1] = ab1; S.id[0] = id0; S.id[1] = id1;
    int64_t rounds = 0, converged = 0, skipped = 0, base = 0;
    for (int g = 0; g < n_groups; base += paths[g], g++) {
        const int64_t m64 = paths[g];
        if (m64 == 0) continue;
        if (m64 > ORIP_IMPROVE_MAX_PATHS) { skipped++; continue; }
        const int m = (int)m64, B = (int)base;
        const long long cap = max_rounds == ORIP_IMPROVE_ROUNDS_AUTO ? 2ll * m + 64 : (long long)max_rounds;
        // the gaps 0 .. m are split over grid.y when the strokes alone give too few blocks
        const int gx = cdiv(m, 256), tiles = cdiv((int64_t)m + 1, IM_TILE);
        const int gy = std::max(1, std::min(tiles, IM_BLOCKS / gx));
        const int chunk = cdiv(tiles, gy) * IM_TILE, gy_used = cdiv((int64_t)m + 1, chunk), n_rec = gx * gy_used;
        if (n_rec > IM_MAX_REC) ORIP_FAIL(c, "%d records (internal error)", n_rec);
        ImStatus h = {0, 0, 0, 0, 0};
        HIPC(c, hipMemcpyAsync(st, &h, sizeof h, hipMemcpyHostToDevice, s));
        HIPC(c, hipStreamSynchronize(s));                                     // h is on the stack and is written again below
        int round = 0;                                                        // launched rounds: chooses the status slot
        while (!h.done) {
            { ProfScope ps(c, "k_im_round");
              for (int r = 0; r < IM_BATCH; r++, round++) {
                  hipLaunchKernelGGL(k_im_eval, dim3(gx, gy_used), b, 0, s, S, B, m, sx, sy, reverse, chunk, cap, st + (round & 1), rec);
                  hipLaunchKernelGGL(k_im_apply, dim3(gx), b, 0, s, S, B, m, cap, n_rec, rec, st + (round & 1), st + ((round + 1) & 1));
              } }
            HIPC(c, hipGetLastError());
            HIPC(c, hipMemcpyAsync(&h, st + (round & 1), sizeof h, hipMemcpyDeviceToHost, s));
            HIPC(c, hipStreamSynchronize(s));
            if (h.rounds < 0 || h.rounds > cap || (unsigned)h.cur > 1u) ORIP_FAIL(c, "the status word is off (internal error)");
        }
        if (h.cur) {                                                          // buffer 0 is where the next group and the end look
            HIPC(c, hipMemcpyAsync(ab0 + B, ab1 + B, (size_t)m * 16, hipMemcpyDeviceToDevice, s));
            HIPC(c, hipMemcpyAsync(id0 + B, id1 + B, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
        }
        rounds += h.rounds; converged += h.converged ? 1 : 0;
    }
    hipLaunchKernelGGL(k_im_travel, gn, b, 0, s, ab0, N, sx, sy, trav + 1);
    HIPC(c, hipGetLastError());
    unsigned long long htrav[2] = {0, 0};
    HIPC(c, hipMemcpyAsync(htrav, trav, 16, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(order, id0, (size_t)N * 4, hipMemcpyDeviceToHost, s));    // stroke | reversed << 31, taken apart below
    HIPC(c, hipStreamSynchronize(s));
    for (int64_t k = 0; k < n; k++) { const uint32_t v = (uint32_t)order[k]; order[k] = (int32_t)(v & 0x7FFFFFFFu); rev[k] = (uint8_t)(v >> 31); }
    stats[0] = (int64_t)htrav[0]; stats[1] = (int64_t)htrav[1]; stats[2] = rounds; stats[3] = converged; stats[4] = skipped;
    return 0;
}
