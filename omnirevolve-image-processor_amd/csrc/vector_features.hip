// csrc/vector_features.hip -- the per-polyline features of the vector stages (vec_common.h: vfeatures*, vlen_order, vwalk_arcs): bounding box, end points,
// cv::arcLength and numpy's float32 pairwise perimeter, bit for bit; short polylines a lane each, long ones a block each.
#include "vec_common.h"

namespace {
// the reversed polyline as a point getter (pt(i) = point n - 1 - i)
template <class Cur> struct RevPt {
    Cur& c; int64_t n;
    __device__ __forceinline__ vs::IPt operator()(int64_t i) const { const int2 p = c.at(n - 1 - i); return vs::IPt{p.x, p.y}; }
};
// what: vec_common.h (VF_*)
__host__ __device__ __forceinline__ bool vf_want_rev(int what) { return (what & (VF_PER | VF_PER_REV)) == (VF_PER | VF_PER_REV); }
template <class Src>
__global__ __launch_bounds__(128) void k_poly_features(Src src, int64_t n_polys, int what, PolyFeat* __restrict__ out, float* __restrict__ per_rev) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_polys) return;
    auto cu = src.cur(i);
    int64_t n = src.len(i);
    PolyFeat f;
    const int2 pf = cu.at(0); int2 pl = n >= 1 ? cu.at(n - 1) : pf;
    f.closed = (n >= 2 && pf.x == pl.x && pf.y == pl.y) ? 1 : 0;
    if ((what & VF_OPEN_VIEW) && f.closed) { n -= 1; pl = cu.at(n - 1); }
    f.n = n;
    f.sx = pf.x; f.sy = pf.y; f.ex = pl.x; f.ey = pl.y;
    f.per = 0.f; f.arc = 0.0; f.x0 = f.x1 = pf.x; f.y0 = f.y1 = pf.y;
    if (n > ORIP_LONG_POLY) { out[i] = f; return; }      // bbox / sums of long polylines: k_poly_features_long (one block each)
    int32_t x0 = pf.x, x1 = pf.x, y0 = pf.y, y1 = pf.y;
    for (int64_t k = 1; k < n; k++) { const int2 q = cu.at(k); x0 = min(x0, q.x); x1 = max(x1, q.x); y0 = min(y0, q.y); y1 = max(y1, q.y); }
    f.x0 = x0; f.y0 = y0; f.x1 = x1; f.y1 = y1;
    const CurPt<decltype(cu)> pt{cu};
    if (what & VF_PER) f.per = vs::pairwise_seglen_sum_p<0>(pt, n);
    if (vf_want_rev(what)) { const RevPt<decltype(cu)> rp{cu, n}; per_rev[i] = vs::pairwise_seglen_sum_p<0>(rp, n); }
    if (what & VF_PER_HYPOT) f.per = vs::pairwise_seglen_sum_p<1>(pt, n);
    if (what & VF_ARC_CLOSED) f.arc = vs::arc_length_p(pt, n, true);
    if (what & VF_ARC_OPEN) f.arc = vs::arc_length_p(pt, n, false);
    out[i] = f;
}

// Long polylines (n > ORIP_LONG_POLY): one 256-thread block per polyline.  bbox and cv::arcLength are plain parallel
// reductions (the double sum of float edge lengths is exact at these magnitudes, so its order is free).  The numpy float32
// pairwise perimeter keeps numpy's exact tree: every leaf of the tree has 64..128 elements (n2 = n/2 - (n/2)%8 >= 64 for
// n > 128), so each multiple of 64 lies in exactly one leaf; the thread that holds the first multiple of 64 of a leaf sums
// that leaf in numpy's 8-accumulator order, and thread 0 then combines the leaf sums with the explicit-stack traversal.
// numpy's split of a node of n > 128 elements: the left child takes the first n2, the right child the rest
__device__ __forceinline__ int64_t pairwise_split(int64_t n) { int64_t n2 = n / 2; n2 -= n2 % 8; return n2; }
// the leaf of numpy's tree over ns elements that holds element pm: elements [s, s + len)
__device__ __forceinline__ void pairwise_leaf_of(int64_t ns, int64_t pm, int64_t& s, int64_t& len) {
    s = 0; len = ns;
    while (len > 128) { const int64_t n2 = pairwise_split(len); if (pm < s + n2) len = n2; else { s += n2; len -= n2; } }
}
// Evaluates numpy's pairwise tree below the node (s0, n0) from the leaf sums; `part`/`depth_left` let the root traversal stop at
// nodes that other threads have already reduced (code = path bits from the root).
__device__ float pairwise_subtree(const float* __restrict__ leafsum, int64_t s0, int64_t n0, const float* part, int depth_left) {
    int64_t fs[28], fn[28]; int fstate[28], fdep[28]; unsigned fcode[28]; float fleft[28];     // depth <= log2(2^31 / 64) + 2
    int sp = 1; fs[0] = s0; fn[0] = n0; fstate[0] = 0; fdep[0] = depth_left; fcode[0] = 0;
    float ret = 0.f;
    while (sp > 0) {
        int t = sp - 1;
        if (fn[t] <= 128) { ret = leafsum[(fs[t] + 63) >> 6]; sp--; continue; }
        if (part && fdep[t] == 0) { ret = part[fcode[t]]; sp--; continue; }
        const int64_t n2 = pairwise_split(fn[t]);
        if (fstate[t] == 0) { fstate[t] = 1; fs[sp] = fs[t]; fn[sp] = n2; fstate[sp] = 0; fdep[sp] = fdep[t] - 1; fcode[sp] = fcode[t] << 1; sp++; }
        else if (fstate[t] == 1) { fleft[t] = ret; fstate[t] = 2; fs[sp] = fs[t] + n2; fn[sp] = fn[t] - n2; fstate[sp] = 0; fdep[sp] = fdep[t] - 1; fcode[sp] = (fcode[t] << 1) | 1u; sp++; }
        else { ret = fleft[t] + ret; sp--; }
    }
    return ret;
}
// one numpy leaf (8 <= n <= 128 elements el(0) .. el(n - 1)) summed by 8 lanes: lane j owns accumulator r[j]; the xor tree reproduces
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) (float addition commutes), the n % 8 tail is added in order.  The getters in use: float32 length (or np.hypot length)
// of a segment from the points, or a STORED length (sl[k] = float32 length of segment k; prefetch08: k_seglen), each in forward order or over the REVERSED
// sequence (element i' of the reversed polyline's ns segment lengths is forward segment ns - 1 - i').
template <class El>
__device__ __forceinline__ float pairwise_leaf8(El el, int64_t n, int j) {
    const int64_t lim = n - (n % 8);
    float r = el(j);
    for (int64_t i = 8 + j; i < lim; i += 8) r += el(i);
    r += __shfl_xor(r, 1, 64); r += __shfl_xor(r, 2, 64); r += __shfl_xor(r, 4, 64);
    for (int64_t i = lim; i < n; i++) r += el(i);
    return r;
}
#define ORIP_PW_DEPTH 8
__global__ __launch_bounds__(256) void k_len_keys(const int64_t* __restrict__ off, int64_t n, unsigned* __restrict__ key, unsigned* __restrict__ val) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { int64_t m = off[i + 1] - off[i]; key[i] = (unsigned)(m > 0xffffffffLL ? 0xffffffffLL : m); val[i] = (unsigned)i; }
}
// All leaves of numpy's pairwise trees of all long polylines in ONE launch, from stored segment lengths (prefetch08): 8 lanes per slot of the leaf table
// (slot (off[i] >> 6) + 2 i + m belongs to the multiple 64 m of polyline i; the leaf that holds element 64 m owns it when 64 m is its first multiple of 64).
// The same leaf shape serves the forward sum and the sum over the reversed sequence (element i' of the reversed polyline = forward segment ns - 1 - i').
// k_poly_features_long then only combines the leaves (VF_LEAVES_DONE): with one block per polyline staging the lengths through LDS the launch was as long as
// ~7 rounds of 186 k-element polylines at five blocks per CU.
__device__ __forceinline__ void perim_leaves_seg_block(int64_t vblock, int64_t* i_first, const int64_t* __restrict__ off, int64_t n_polys, const PolyFeat* __restrict__ feat,
                                                       const float* __restrict__ seg, float* __restrict__ leafbuf, float* __restrict__ leafbuf_rev, int64_t nslots) {
    const int64_t q = (vblock * 256 + threadIdx.x) >> 3; const int j = threadIdx.x & 7;
    if (threadIdx.x == 0) {                               // polyline of the block's first slot: the last i with (off[i] >> 6) + 2 i <= q; the other 31 slots walk on from it
        int64_t lo = 0, hi = n_polys - 1;
        while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if ((off[mid] >> 6) + 2 * mid <= q) lo = mid; else hi = mid - 1; }
        *i_first = lo;
    }
    __syncthreads();
    if (q >= nslots) return;
    int64_t i = *i_first;
    while (i + 1 < n_polys && (off[i + 1] >> 6) + 2 * (i + 1) <= q) i++;
    const int64_t n = feat[i].n;
    if (n <= ORIP_LONG_POLY) return;
    const int64_t ns = n - 1, pm = (q - ((off[i] >> 6) + 2 * i)) << 6;
    if (pm >= ns) return;
    int64_t s, len; pairwise_leaf_of(ns, pm, s, len);
    if ((((s + 63) >> 6) << 6) != pm) return;
    const float* sl = seg + off[i];
    const float v = pairwise_leaf8([&](int64_t k) { return sl[s + k]; }, len, j);
    if (j == 0) leafbuf[q] = v;
    if (leafbuf_rev) { const float r = pairwise_leaf8([&](int64_t k) { return sl[ns - 1 - (s + k)]; }, len, j); if (j == 0) leafbuf_rev[q] = r; }
}
__global__ __launch_bounds__(256) void k_perim_leaves_seg(const int64_t* __restrict__ off, int64_t n_polys, const PolyFeat* __restrict__ feat, const float* __restrict__ seg,
                                                          float* __restrict__ leafbuf, float* __restrict__ leafbuf_rev, int64_t nslots) {
    __shared__ int64_t i_first;
    perim_leaves_seg_block((int64_t)blockIdx.x, &i_first, off, n_polys, feat, seg, leafbuf, leafbuf_rev, nslots);
}
#define ORIP_PF_MARGIN 132      // points staged on either side of a turn's 2048: a leaf has at most 128 elements and owns a multiple of 64 of the turn
template <class Src, bool FROM_SEG = false>
__global__ __launch_bounds__(256) void k_poly_features_long(Src src, int64_t n_polys, int what,
                                                             PolyFeat* __restrict__ out, float* __restrict__ leafbuf, const unsigned* __restrict__ order,
                                                             float* __restrict__ per_rev, float* __restrict__ leafbuf_rev, const float* __restrict__ seg = nullptr) {
    __shared__ int rx0[256], rx1[256], ry0[256], ry1[256];
    __shared__ double rarc[256];
    __shared__ float part[2 << ORIP_PW_DEPTH];
    __shared__ int2 stage[2048 + 2 * ORIP_PF_MARGIN + 8];
    const bool want_rev = vf_want_rev(what);
    for (int64_t rr = blockIdx.x; rr < n_polys; rr += gridDim.x) {
        const int64_t i = order[rr];               // longest first: a block that draws a long polyline late would be the tail of the launch
        PolyFeat f = out[i];
        const int64_t n = f.n;                     // already the open view when requested
        if (n <= ORIP_LONG_POLY) continue;         // uniform for the block
        auto cu = src.cur(i);
        auto P2 = [&](int64_t k) { return cu.at(k); };
        const int tid = threadIdx.x;
        int x0 = f.sx, x1 = f.sx, y0 = f.sy, y1 = f.sy; double arc = 0.0;
        const bool closed_arc = (what & VF_ARC_CLOSED) != 0, any_arc = (what & (VF_ARC_CLOSED | VF_ARC_OPEN)) != 0, any_per = (what & (VF_PER | VF_PER_HYPOT)) != 0;
        if (any_arc) {
            // arc length next to the bounding box: four loads in flight per thread; a thread adds its terms in the order of its k
            auto seg = [&](int64_t k, const int2 a, const int2 b) {       // b: predecessor of point k
                x0 = min(x0, a.x); x1 = max(x1, a.x); y0 = min(y0, a.y); y1 = max(y1, a.y);
                float dx = (float)a.x - (float)b.x, dy = (float)a.y - (float)b.y;
                arc += (double)sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
            };
            auto pred = [&](int64_t k) -> int64_t { return k == 0 ? (closed_arc ? n - 1 : 0) : k - 1; };
            // A wave takes four consecutive windows of 64 points per turn and fetches every point once (a cursor call is ~25 instructions):
            // the predecessor of point k sits in the lane below, that of a window's first point in the last lane of the window before,
            // and only the first point of a turn needs one extra fetch.
            const int lane = tid & 63;
            for (int64_t base = (int64_t)(tid >> 6) * 256; base < n; base += 1024) {
                int2 p[4];
#pragma unroll
                for (int w = 0; w < 4; w++) { const int64_t k = base + 64 * w + lane; p[w] = k < n ? P2(k) : make_int2(0, 0); }
                int2 first = P2(pred(base));
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    int2 b;
                    b.x = __builtin_amdgcn_update_dpp(0, p[w].x, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
                    b.y = __builtin_amdgcn_update_dpp(0, p[w].y, 0x138, 0xf, 0xf, true);
                    if (lane == 0) b = first;
                    const int64_t k = base + 64 * w + lane;
                    if (k < n) seg(k, p[w], b);
                    first = make_int2(__builtin_amdgcn_readlane(p[w].x, 63), __builtin_amdgcn_readlane(p[w].y, 63));
                }
            }
        } else if (!any_per) {
            // bounding box only: four independent 8-byte loads per turn keep the memory pipeline busy (the loop is latency-bound otherwise)
            int64_t k = tid;
            for (; k + 768 < n; k += 1024) {
                const int2 a = P2(k), b = P2(k + 256), cc = P2(k + 512), d = P2(k + 768);
                x0 = min(min(x0, a.x), min(min(b.x, cc.x), d.x)); x1 = max(max(x1, a.x), max(max(b.x, cc.x), d.x));
                y0 = min(min(y0, a.y), min(min(b.y, cc.y), d.y)); y1 = max(max(y1, a.y), max(max(b.y, cc.y), d.y));
            }
            for (; k < n; k += 256) { const int2 a = P2(k); x0 = min(x0, a.x); x1 = max(x1, a.x); y0 = min(y0, a.y); y1 = max(y1, a.y); }
        }
        float per = 0.f, perR = 0.f;
        if (any_per) {
            const int64_t ns = n - 1;               // number of segments
            float* ls = leafbuf + (src.off[i] >> 6) + 2 * i;
            float* lsR = want_rev ? leafbuf_rev + (src.off[i] >> 6) + 2 * i : nullptr;
            const int grp = tid >> 3, j = tid & 7;  // 32 groups of 8 lanes, one leaf per group, turn and direction
            // A turn covers the 32 multiples of 64 in [r0, r0 + 2048).  The leaves of numpy's tree that own them lie inside
            // [r0 - 63, r0 + 2047 + 128]; the leaves of the REVERSED sequence that own the multiples of 64 of the mirrored interval
            // [ns - r0 - 2048, ns - r0) map to forward segments inside [r0 - 129, r0 + 2048 + 128).  So one stretch of points, staged
            // in LDS by all threads (independent coalesced loads), serves both directions -- and the bounding box (a point is read once).
            // The points of the NEXT turn are requested before the leaves of this turn are summed and only land in LDS after them.
            constexpr int NX = (2048 + 2 * ORIP_PF_MARGIN + 255) / 256;
            int2 nxt[NX];
            // FROM_SEG: the stretch holds the stored LENGTHS of the segments [lo, hi - 1) instead of the points [lo, hi) (the bounding box is in place already)
            const float* sgp = FROM_SEG ? seg + src.off[i] : nullptr;
            float* stagef = reinterpret_cast<float*>(stage);
            auto request = [&](int64_t r0) {
                const int64_t lo = max((int64_t)0, r0 - ORIP_PF_MARGIN), hi = min(n, r0 + 2048 + ORIP_PF_MARGIN);
#pragma unroll
                for (int u = 0; u < NX; u++) {
                    const int64_t q = lo + tid + 256 * u;
                    if (FROM_SEG) nxt[u].x = q < hi - 1 ? __float_as_int(sgp[q]) : 0;
                    else nxt[u] = q < hi ? P2(q) : make_int2(0, 0);
                }
            };
            if (!(what & VF_LEAVES_DONE)) request(0);
            for (int64_t r0 = 0; r0 < n && !(what & VF_LEAVES_DONE); r0 += 32 * 64) {      // (the last turn may hold points only: the bounding box wants them all; VF_LEAVES_DONE: the leaf sums are in place, k_perim_leaves_seg)
                const int64_t lo = max((int64_t)0, r0 - ORIP_PF_MARGIN), hi = min(n, r0 + 2048 + ORIP_PF_MARGIN);       // points [lo, hi)
                __syncthreads();
#pragma unroll
                for (int u = 0; u < NX; u++) {
                    const int64_t q = lo + tid + 256 * u;
                    if (FROM_SEG) { if (q < hi - 1) stagef[tid + 256 * u] = __int_as_float(nxt[u].x); }
                    else if (q < hi) {
                        stage[tid + 256 * u] = nxt[u];
                        if (q >= r0 && q < r0 + 2048) { x0 = min(x0, nxt[u].x); x1 = max(x1, nxt[u].x); y0 = min(y0, nxt[u].y); y1 = max(y1, nxt[u].y); }
                    }
                }
                __syncthreads();
                if (r0 + 32 * 64 < n) request(r0 + 32 * 64);
                const int32_t* sp = reinterpret_cast<const int32_t*>(stage) - 2 * lo;        // sp[2 * k] = x of point k
                const float* sf = stagef - lo;                                               // sf[k] = length of segment k
                const int64_t pm = r0 + (int64_t)grp * 64;
                if (pm < ns) {
                    int64_t s, len; pairwise_leaf_of(ns, pm, s, len);
                    if (((s + 63) >> 6) << 6 == pm) {   // every multiple of 64 lies in exactly one leaf; its first one owns the leaf
                        float v = FROM_SEG ? pairwise_leaf8([&](int64_t k) { return sf[s + k]; }, len, j)
                                           : (what & VF_PER) ? pairwise_leaf8([&](int64_t k) { return vs::seg_len_f32(sp, s + k); }, len, j)
                                                             : pairwise_leaf8([&](int64_t k) { return vs::seg_hypot_f32(sp, s + k); }, len, j);
                        if (j == 0) ls[pm >> 6] = v;
                    }
                }
                if (want_rev) {
                    // multiples of 64 of the reversed index space inside the mirrored interval [max(0, ns - r0 - 2048), ns - r0)
                    const int64_t ilo = max((int64_t)0, ns - r0 - 2048), ihi = ns - r0;
                    const int64_t pmr = (((ilo + 63) >> 6) << 6) + (int64_t)grp * 64;
                    if (pmr < ihi) {
                        int64_t s, len; pairwise_leaf_of(ns, pmr, s, len);
                        if (((s + 63) >> 6) << 6 == pmr) {
                            float v = FROM_SEG ? pairwise_leaf8([&](int64_t k) { return sf[ns - 1 - (s + k)]; }, len, j)
                                               : pairwise_leaf8([&](int64_t k) { return vs::seg_len_f32(sp, ns - 1 - (s + k)); }, len, j);
                            if (j == 0) lsR[pmr >> 6] = v;
                        }
                    }
                }
            }
            __threadfence_block();
            __syncthreads();
            // numpy's tree, level by level.  Node `code` (heap numbering, root 1) at depth d is reached by the d path bits of code - 2^d
            // (0 = left half of n2 = n/2 - (n/2)%8 elements).  Depth ORIP_PW_DEPTH: thread t reduces the subtree below its node from
            // the leaf sums; the levels above combine left + right in LDS, a node that is itself a leaf takes its leaf sum.
            auto node_of = [&](int d, int t, int64_t& s, int64_t& len) -> bool {      // false: an ancestor is already a leaf
                s = 0; len = ns;
                for (int lvl = d - 1; lvl >= 0; lvl--) {
                    if (len <= 128) return false;
                    const int64_t n2 = pairwise_split(len);
                    if ((t >> lvl) & 1) { s += n2; len -= n2; } else len = n2;
                }
                return true;
            };
            for (int dir = 0; dir < (want_rev ? 2 : 1); dir++) {
                const float* lsd = dir ? lsR : ls;
                {
                    int64_t s, len;
                    if (node_of(ORIP_PW_DEPTH, tid, s, len)) part[(1 << ORIP_PW_DEPTH) + tid] = pairwise_subtree(lsd, s, len, nullptr, 0);
                }
                for (int d = ORIP_PW_DEPTH - 1; d >= 0; d--) {
                    __syncthreads();
                    if (tid < (1 << d)) {
                        int64_t s, len; const int code = (1 << d) + tid;
                        if (node_of(d, tid, s, len)) part[code] = (len <= 128) ? lsd[(s + 63) >> 6] : part[2 * code] + part[2 * code + 1];
                    }
                }
                __syncthreads();
                if (tid == 0) { if (dir) perR = part[1]; else per = part[1]; }
                __syncthreads();
            }
        }
        rx0[tid] = x0; rx1[tid] = x1; ry0[tid] = y0; ry1[tid] = y1; rarc[tid] = arc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) { rx0[tid] = min(rx0[tid], rx0[tid + s]); rx1[tid] = max(rx1[tid], rx1[tid + s]); ry0[tid] = min(ry0[tid], ry0[tid + s]); ry1[tid] = max(ry1[tid], ry1[tid + s]); rarc[tid] += rarc[tid + s]; }
            __syncthreads();
        }
        if (tid == 0) {
            if (!FROM_SEG) { f.x0 = rx0[0]; f.x1 = rx1[0]; f.y0 = ry0[0]; f.y1 = ry1[0]; }       // FROM_SEG: the box came with f (k_cumlen_long2 wrote it)
            f.arc = rarc[0]; f.per = per; out[i] = f; if (want_rev) per_rev[i] = perR;
        }
        __syncthreads();
    }
}
// cv::arcLength(contour, closed = true) (07:50) of the long contours of a walk-coded list whose polylines are whole walks, WITHOUT visiting their points:
// a walk is its own points plus tail pieces that run through consecutive log entries, the last ones lap after lap around one cycle (walker.h: VWalk /
// VPiece), so its perimeter is the own segments + per piece the segments of one lap (x laps) and of the partial lap + the junctions.  The reference adds the
// float32 segment lengths into a double; every length is a multiple of 2^-23 and the total stays below 2^22, so every partial sum is exact and the order (and
// the multiplication by the lap count) cannot change the result -- the same argument k_poly_features_long's parallel sum rests on.  One wave per walk; the pass
// over 2.8e8 points it replaces sat on the chain in front of stage 07's greedy order with 1 - 4 ms.
__global__ __launch_bounds__(64) void k_walk_arcs(VSrc src, int64_t n_polys, PolyFeat* __restrict__ feat) {
    const int lane = threadIdx.x;
    auto len2 = [](const int2 a, const int2 b) -> double {
        const float dx = (float)a.x - (float)b.x, dy = (float)a.y - (float)b.y;
        return (double)sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
    };
    auto wave_sum = [](double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; };
    for (int64_t i = blockIdx.x; i < n_polys; i += gridDim.x) {
        if (feat[i].n <= ORIP_LONG_POLY) continue;           // the short ones have their sum from k_poly_features
        const VWalk w = src.walk[i];
        const int2* own = src.g.own + w.own_off;
        double acc = 0.0;
        for (unsigned t = 1u + (unsigned)lane; t <= w.n_own; t += 64u) acc += len2(own[t], own[t - 1u]);
        const unsigned closing = w.flags & 1u;
        const unsigned T = w.len - closing - (w.n_own + 1u);      // tail points
        int2 last = own[w.n_own];
        for (unsigned j = 0; j < w.n_piece && T > 0u; j++) {
            const VPiece q = src.g.piece[w.piece_off + j];
            const unsigned cnt = (j + 1u < w.n_piece ? src.g.piece[w.piece_off + j + 1u].u0 : T) - q.u0;
            if (cnt == 0u) continue;
            const int2* L = src.g.lxy + q.ent;
            if (lane == 0) acc += len2(L[0], last);               // the junction into the piece
            if (q.lam == 0u) {
                for (unsigned e = (unsigned)lane; e + 1u < cnt; e += 64u) acc += len2(L[e + 1u], L[e]);
                last = L[cnt - 1u];
            } else {
                // points m = 0 .. cnt - 1 sit at entry m mod lam: step m wraps iff m mod lam == 0, every lap is the lam - 1 inner steps + the wrap
                const unsigned laps = (cnt - 1u) / q.lam, r = (cnt - 1u) % q.lam;
                double full = 0.0, part = 0.0;
                for (unsigned e = (unsigned)lane; e + 1u < q.lam; e += 64u) { const double d = len2(L[e + 1u], L[e]); full += d; if (e < r) part += d; }
                full = wave_sum(full);
                if (lane == 0) acc += (double)laps * (full + len2(L[0], L[q.lam - 1u]));
                acc += part;
                last = L[r];
            }
        }
        if (lane == 0) acc += len2(own[0], last);                 // to the closing point when there is one (then the wrap is 0), else the closed contour's wrap
        acc = wave_sum(acc);
        if (lane == 0) feat[i].arc = acc;
    }
}
}  // namespace
// ---- the host side of the features (vec_common.h)
void vfeatures_short(orip_ctx* c, const VSrc& src, int64_t n, int what, PolyFeat* feat, float* per_rev) {
    hipLaunchKernelGGL(k_poly_features<VSrc>, dim3(cdiv(n, 128)), dim3(128), 0, LN(c).stream, src, n, what, feat, per_rev);
}
void vwalk_arcs(orip_ctx* c, const VSrc& src, int64_t n, PolyFeat* feat) {
    hipLaunchKernelGGL(k_walk_arcs, dim3((unsigned)std::min<int64_t>(n, 16384)), dim3(64), 0, LN(c).stream, src, n, feat);
}
int vlen_order(orip_ctx* c, const int64_t* off, int64_t n, unsigned* kin, unsigned* kout, unsigned* vin, unsigned* order) {
    hipLaunchKernelGGL(k_len_keys, dim3(cdiv(n, 256)), dim3(256), 0, LN(c).stream, off, n, kin, vin);
    return vsort_pairs<unsigned, unsigned>(c, kin, kout, vin, order, (size_t)n, 0, 32, true);
}
// the long polylines' part of vfeatures_src
template <class Src>
static int vfeatures_long(orip_ctx* c, const Src& src, int64_t n, int64_t total, int what, PolyFeat* feat, float* per_rev) {
    if (n == 0 || total <= ORIP_LONG_POLY) return 0;
    const size_t nleaf = (size_t)(total >> 6) + 2 * (size_t)n + 8;
    float* leafbuf; unsigned *kin, *kout, *vin, *vout;
    { Carve L; L.take(leafbuf, nleaf * ((what & VF_PER_REV) ? 2 : 1)); L.each(n, kin, kout, vin, vout); HIPC(c, L.commit(LN(c).vtmp[VT_LEAVES], 64)); }      // (leafbuf: forward leaves, then the reversed reading's)
    float* leafbuf_rev = (what & VF_PER_REV) ? leafbuf + nleaf : nullptr;
    ORIP_TRY(vlen_order(c, src.off, n, kin, kout, vin, vout));
    ProfScope ps(c, "k_poly_features_long");
    hipLaunchKernelGGL((k_poly_features_long<Src, false>), dim3((unsigned)std::min<int64_t>(n, 4096)), dim3(256), 0, LN(c).stream, src, n, what, feat, leafbuf, vout, per_rev, leafbuf_rev, (const float*)nullptr);
    HIPC(c, hipGetLastError());
    return 0;
}
int vfeatures_long_seg(orip_ctx* c, const VSrc& src, int64_t n, int64_t total, PolyFeat* feat, const unsigned* order, float* per_rev, const float* seg) {
    ProfScope ps(c, "k_poly_features_long");
    const size_t nleaf = (size_t)(total >> 6) + 2 * (size_t)n + 8;
    HIPC(c, LN(c).vtmp[VT_LEAVES].ensure(nleaf * sizeof(float) * 2 + 64));
    float* leafbuf = LN(c).vtmp[VT_LEAVES].as<float>(); float* leafbuf_rev = leafbuf + nleaf;      // (one array: forward leaves, then the reversed reading's)
    hipLaunchKernelGGL(k_perim_leaves_seg, dim3((unsigned)cdiv((int64_t)nleaf * 8, 256)), dim3(256), 0, LN(c).stream, src.off, n, feat, seg, leafbuf, leafbuf_rev, (int64_t)nleaf);
    hipLaunchKernelGGL((k_poly_features_long<VSrc, true>), dim3((unsigned)std::min<int64_t>(n, 4096)), dim3(256), 0, LN(c).stream, src, n, VF_PER | VF_OPEN_VIEW | VF_PER_REV | VF_LEAVES_DONE, feat, leafbuf, order, per_rev, leafbuf_rev, seg);
    return 0;
}
template <class Src>
static int vfeatures_src(orip_ctx* c, const Src& src, int64_t n, int64_t total, int what, PolyFeat* feat, float* per_rev = nullptr) {
    if (n == 0) return 0;
    if (!per_rev) what &= ~VF_PER_REV;
    hipLaunchKernelGGL(k_poly_features<Src>, dim3(cdiv(n, 128)), dim3(128), 0, LN(c).stream, src, n, what, feat, per_rev);
    ORIP_TRY(vfeatures_long(c, src, n, total, what, feat, per_rev));
    HIPC(c, hipGetLastError());
    return 0;
}
int vfeatures(orip_ctx* c, const DPolys& P, int what, PolyFeat* feat) {
    ORIP_WITH_SRC(c, P, src, { ORIP_TRY(vfeatures_src(c, src, P.n, P.total, what, feat)); });
    return 0;
}
