// csrc/vector08b.hip -- stage 08-B (08_dedup_layer_basic.py _post_skeleton_merge, 08:376-469) on gfx950.
//
// Stage B runs all clusters at once on one padded canvas: clusters are more than 4 post_brush + 12 px apart in one axis (76 at the default brush) and a
// band reaches post_brush / 2 <= PAD8 beyond its lines, so per-ROI rasterise / thin / label equals whole-canvas rasterise / thin / label (DESIGN.md
// "stage 08-B"; dedup08_b refuses a brush whose band the pad would clip).
// Layout: the kernels (groups, raster, Zhang-Suen thinning, components, paths), then the host side: one function per phase (b_groups, b_raster_thin,
// b_components, b_paths) and dedup08_b, which calls them in order.  Scans and sorts go through vscan_excl / vsort_pairs (vec_common.h); the bit-plane
// kernels (thinning word, CCL, compaction, heads) are the shared blocks of bitplane.h, with the linear pixel id y * Wp + x.  Nothing passes over the canvas
// pixel by pixel: the stamps set the bit plane themselves and everything behind them works on its words or on the skeleton's pixel list.
#include "vec08.h"
#include "bitplane.h"
#include <cstdio>
#define PAD8 64

namespace {

// ================================================================= B: _post_skeleton_merge
__global__ __launch_bounds__(256) void k_iota(int* a, int n) { int i = blockIdx.x * 256 + threadIdx.x; if (i < n) a[i] = i; }
__global__ __launch_bounds__(256) void k_bbox_pairs(const PolyFeat* __restrict__ f, int n, int exp, int* __restrict__ par) {
    // bboxes expanded by exp on each side overlap  <=>  not separated (08:41-42)
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        int ax0 = f[i].x0 - exp, ay0 = f[i].y0 - exp, ax1 = f[i].x1 + exp, ay1 = f[i].y1 + exp;
        for (int j = i + 1 + threadIdx.x; j < n; j += 256) {
            int bx0 = f[j].x0 - exp, by0 = f[j].y0 - exp, bx1 = f[j].x1 + exp, by1 = f[j].y1 + exp;
            if (!(ax1 < bx0 || bx1 < ax0 || ay1 < by0 || by1 < ay0)) uf_unite(par, i, j);
        }
    }
}
struct GroupInfo { int x0, y0, x1, y1; unsigned long long longest; unsigned long long near0, near1; int rank; int a0x, a0y, a1x, a1y; };
__global__ __launch_bounds__(256) void k_group_init(GroupInfo* g, int n) {
    int i = blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
    GroupInfo q; q.x0 = q.y0 = 0x7fffffff; q.x1 = q.y1 = -0x7fffffff; q.longest = ~0ULL; q.near0 = q.near1 = ~0ULL; q.rank = -1; q.a0x = q.a0y = q.a1x = q.a1y = 0;
    g[i] = q;
}
__global__ __launch_bounds__(256) void k_group_accum(const PolyFeat* __restrict__ f, int n, int exp, int* __restrict__ par, GroupInfo* __restrict__ g, unsigned* __restrict__ is_root) {
    int i = blockIdx.x * 256 + threadIdx.x; if (i > n) return;
    if (i == n) { is_root[i] = 0; return; }
    int r = uf_find(par, i); par[i] = r;
    is_root[i] = (r == i) ? 1u : 0u;
    atomicMin(&g[r].x0, f[i].x0 - exp); atomicMin(&g[r].y0, f[i].y0 - exp); atomicMax(&g[r].x1, f[i].x1 + exp); atomicMax(&g[r].y1, f[i].y1 + exp);
    unsigned long long key = ((unsigned long long)(~__float_as_uint(f[i].per)) << 32) | (unsigned)i;     // longest, first index on ties (08:391)
    atomicMin(&g[r].longest, key);
}
__global__ __launch_bounds__(256) void k_group_finish(const PolyFeat* __restrict__ f, int n, const unsigned* __restrict__ is_root, const unsigned* __restrict__ root_scan, GroupInfo* __restrict__ g) {
    int i = blockIdx.x * 256 + threadIdx.x; if (i >= n || !is_root[i]) return;
    g[i].rank = (int)root_scan[i];
    int l = (int)(g[i].longest & 0xffffffffu);
    g[i].a0x = f[l].sx; g[i].a0y = f[l].sy; g[i].a1x = f[l].ex; g[i].a1y = f[l].ey;
}
// raster: gid[pixel] = group root + 1 for every pixel within r of a segment of a line of the group, and the pixel's bit in the plane `bits` (Wwp words per
// row, cleared by the caller; gid is NOT: it is defined at the pixels stamped here and read at those only).  One wave per segment.  The box index q is
// linear, so the lanes of one trip that share a row and a 64-pixel word are neighbours and lane s + t holds the pixel t to the right of lane s: the first
// lane of such a stretch shifts the stretch's part of the ballot into place and issues ONE 64-bit atomicOr for it.  No shuffle, no LDS.
__global__ __launch_bounds__(256) void k_stamp_groups(const int64_t* __restrict__ off, const int32_t* __restrict__ pts, int64_t n_polys, int64_t n_pts, const int* __restrict__ par,
                                                       int rad, unsigned* __restrict__ gid, unsigned long long* __restrict__ bits, int Wp, int Hp, int Wwp) {
    const int lane = threadIdx.x & 63; const long long r2 = (long long)rad * rad;
    long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((long long)gridDim.x * 256) >> 6;
    for (long long i = wave; i + 1 < n_pts; i += nw) {
        // polyline of point i: last off <= i
        long long lo = 0, hi = n_polys;
        while (lo < hi) { long long mid = (lo + hi) >> 1; if (off[mid + 1] <= i) lo = mid + 1; else hi = mid; }
        if (i + 1 >= off[lo + 1]) continue;                 // i is the last point of its polyline
        unsigned val = (unsigned)par[lo] + 1u;
        int x0 = pts[2 * i] + PAD8, y0 = pts[2 * i + 1] + PAD8, x1 = pts[2 * i + 2] + PAD8, y1 = pts[2 * i + 3] + PAD8;
        int bx0 = max(0, min(x0, x1) - rad), bx1 = min(Wp - 1, max(x0, x1) + rad), by0 = max(0, min(y0, y1) - rad), by1 = min(Hp - 1, max(y0, y1) + rad);
        int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
        if (bw <= 0 || bh <= 0) continue;
        for (int q0 = 0; q0 < bw * bh; q0 += 64) {          // (wave-uniform trip count: every lane takes part in the ballots)
            const int q = q0 + lane;
            const int x = bx0 + q % bw, y = by0 + q / bw;
            const bool in = q < bw * bh && vs::in_capsule(x, y, x0, y0, x1, y1, r2);
            if (in) gid[(size_t)y * Wp + x] = val;
            const unsigned long long m = __ballot(in);
            const unsigned long long heads = __ballot(lane == 0 || (x & 63) == 0 || x == bx0);      // first lane of a (row, word) stretch
            if (!m) continue;
            const unsigned long long rest = (heads >> lane) >> 1;                                    // the heads after this lane
            const int len = rest ? __ffsll((long long)rest) : 64 - lane;                              // lanes of this stretch (1 .. 64)
            const unsigned long long seg = (m >> lane) & (len == 64 ? ~0ULL : (1ULL << len) - 1ULL);
            if (((heads >> lane) & 1ULL) && seg) atomicOr(&bits[(size_t)y * Wwp + (x >> 6)], seg << (x & 63));      // (seg != 0: some lane of it is inside the box, so this row is)
        }
    }
}
// ---- standard-orientation Zhang-Suen thinning (08:349-366) on the bit plane of the padded canvas (12.8 MB, i.e. cache-resident): zs_delete<ZS_STANDARD>
// of bitplane.h evaluates a sub-iteration for the 64 pixels of a word.  Out-of-image pixels are background.
// `iters` whole iterations (two sub-iterations each) in ONE launch: a block keeps a tile of 64 rows x 2 words plus a halo of ZS_HALO rows / one word on
// every side in LDS and runs the sub-iterations there.  A sub-iteration reads the 3x3 neighbourhood, so after t of them the tile is exact everywhere at
// least t pixels inside the staged region: with iters <= ZS_HALO / 2 the core is exact after all of them, whatever the neighbouring tiles do meanwhile
// (they read the same source plane s; the result goes to d).  changed[b] is set when iteration b deletes a pixel of some core.  Twelve iterations were
// 24 dispatches of ~30 us on the layer's chain; most tiles of a canvas of thin lines are empty and leave after the staging.
#define ZS_HALO 24
#define ZS_TR 64
#define ZS_ROWS (ZS_TR + 2 * ZS_HALO)
__global__ __launch_bounds__(256) void k_zs_tile(const unsigned long long* __restrict__ s, unsigned long long* __restrict__ d, int H, int Ww, int iters, int* __restrict__ changed) {
    __shared__ unsigned long long T[2][ZS_ROWS][4];
    __shared__ int any_s;
    const int tid = threadIdx.x;
    const int y0 = blockIdx.y * ZS_TR - ZS_HALO, x0 = blockIdx.x * 2 - 1;          // first staged row / word
    if (tid == 0) any_s = 0;
    __syncthreads();
    int any = 0;
    for (int i = tid; i < ZS_ROWS * 4; i += 256) {
        const int r = i >> 2, wx = i & 3, y = y0 + r, xw = x0 + wx;
        const unsigned long long v = (y < 0 || y >= H || xw < 0 || xw >= Ww) ? 0ULL : s[(size_t)y * Ww + xw];
        T[0][r][wx] = v; any |= v != 0;
    }
    if (any) any_s = 1;
    __syncthreads();
    const bool empty = !any_s;
    int cur = 0;
    if (!empty) {
        for (int t = 0; t < 2 * iters; t++) {
            int del_core = 0;
            for (int i = tid; i < ZS_ROWS * 4; i += 256) {
                const int r = i >> 2, wx = i & 3;
                const unsigned long long M = T[cur][r][wx];
                unsigned long long out = 0;
                if (M) {
                    auto G = [&](int rr, int ww) -> unsigned long long { return (rr < 0 || rr >= ZS_ROWS || ww < 0 || ww > 3) ? 0ULL : T[cur][rr][ww]; };
                    const unsigned long long del = zs_delete<ZS_STANDARD>(M, nb8_of(M, G(r - 1, wx), G(r - 1, wx - 1), G(r - 1, wx + 1), G(r, wx - 1), G(r, wx + 1), G(r + 1, wx), G(r + 1, wx - 1), G(r + 1, wx + 1)), t & 1);
                    out = M & ~del;
                    if (del && r >= ZS_HALO && r < ZS_HALO + ZS_TR && (wx == 1 || wx == 2)) del_core = 1;
                }
                T[cur ^ 1][r][wx] = out;
            }
            if (del_core) changed[t >> 1] = 1;
            cur ^= 1;
            __syncthreads();
        }
    }
    for (int i = tid; i < ZS_TR * 2; i += 256) {
        const int r = ZS_HALO + (i >> 1), wx = 1 + (i & 1), y = y0 + r, xw = x0 + wx;
        if (y < H && xw < Ww) d[(size_t)y * Ww + xw] = empty ? 0ULL : T[cur][r][wx];
    }
}
// anchors: nearest skeleton pixel of the group to a0 / a1 (first in raster order on ties, 08:428-432)
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) { unsigned long long t = __shfl_xor(v, o, 64); if (t < v) v = t; }
    return v;
}
__global__ __launch_bounds__(256) void k_nearest_anchor(const unsigned* __restrict__ lin, int64_t m, const unsigned* __restrict__ gid, int Wp, GroupInfo* __restrict__ g,
                                                        unsigned long long* __restrict__ ckey, unsigned nc) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < m;
    if (i < nc) ckey[i] = ~0ULL;                               // (nc <= m) the components' keys, for the minima of k_comp_keys behind this kernel
    unsigned grp = 0; unsigned long long k0 = ~0ULL, k1 = ~0ULL;
    if (valid) {
        unsigned p = lin[i]; int x = (int)(p % Wp) - PAD8, y = (int)(p / Wp) - PAD8;
        grp = gid[p] - 1;
        const GroupInfo* G = g + grp;
        long long d0 = (long long)(y - G->a0y) * (y - G->a0y) + (long long)(x - G->a0x) * (x - G->a0x);
        long long d1 = (long long)(y - G->a1y) * (y - G->a1y) + (long long)(x - G->a1x) * (x - G->a1x);
        k0 = ((unsigned long long)d0 << 27) | p; k1 = ((unsigned long long)d1 << 27) | p;
    }
    // pixels next to each other in raster order mostly share their group: one atomic per (wave, group) instead of one per pixel
    unsigned long long rem = __ballot(valid);
    const int lane = threadIdx.x & 63;
    while (rem) {
        int L = __ffsll((long long)rem) - 1;
        unsigned gL = (unsigned)__shfl((int)grp, L, 64);
        bool same = valid && grp == gL;
        unsigned long long m0 = wave_min_u64(same ? k0 : ~0ULL), m1 = wave_min_u64(same ? k1 : ~0ULL);
        if (lane == L) {       // the minima only ever decrease: a stale read can only let a useless atomic through, never drop a winner
            GroupInfo* G = g + gL;
            if (m0 < *(volatile unsigned long long*)&G->near0) atomicMin(&G->near0, m0);
            if (m1 < *(volatile unsigned long long*)&G->near1) atomicMin(&G->near1, m1);
        }
        rem &= ~__ballot(same);
    }
}
// per component: sort key (group rank, ROI-relative block-raster key of its first block)
// One thread per pixel of the component-sorted list (a component of 20 000 pixels was one thread's loop, and the launch as long as that loop): pixel q belongs
// to component head_scan[q] + head[q] - 1 (the heads and their exclusive scan, still in place behind k_comp_starts).  Every pixel forms the whole key with the
// group of its component's FIRST pixel, as the loop did, so the keys of one component differ in the block index alone and their minimum is the old key.  A
// component's pixels are neighbours in the list: a segmented running minimum over the wave, then one atomicMin per (wave, component) on the word that
// k_nearest_anchor has set to all ones.
__global__ __launch_bounds__(256) void k_comp_keys(const unsigned* __restrict__ cs, const unsigned* __restrict__ head, const unsigned* __restrict__ head_scan, unsigned m,
                                                    const unsigned* __restrict__ lin, const unsigned* __restrict__ gid, int Wp,
                                                    const GroupInfo* __restrict__ g, unsigned long long* __restrict__ ckey, unsigned* __restrict__ cidx) {
    const unsigned q = blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < m;
    unsigned c = 0xffffffffu; unsigned long long key = ~0ULL;
    if (valid) {
        const unsigned hd = head[q];
        c = head_scan[q] + hd - 1u;
        const GroupInfo* G = g + (gid[lin[cs[c]]] - 1);
        int w = max(1, G->x1 - G->x0); int wb = (w + 1) >> 1;
        unsigned p = lin[q]; int x = (int)(p % Wp) - PAD8 - G->x0, y = (int)(p / Wp) - PAD8 - G->y0;
        unsigned k = (unsigned)((y >> 1) * wb + (x >> 1));
        key = ((unsigned long long)(unsigned)G->rank << 32) | k;
        if (hd) cidx[c] = c;
    }
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {                         // the lanes of a component are contiguous: equal c at distance o means equal c in between
        const unsigned long long t = __shfl_up(key, o, 64); const unsigned ct = (unsigned)__shfl_up((int)c, o, 64);
        if (lane >= o && ct == c && t < key) key = t;
    }
    const unsigned cn = (unsigned)__shfl_down((int)c, 1, 64);
    if (valid && (lane == 63 || cn != c)) {                    // the last lane of the component in this wave (an invalid lane has no component)
        if (key < *(volatile unsigned long long*)&ckey[c]) atomicMin(&ckey[c], key);      // (a stale read only lets a useless atomic through: k_nearest_anchor)
    }
}

__device__ const int OFY[8] = {-1, -1, -1, 0, 1, 1, 1, 0};     // _OFFS (dy,dx), 08:252
__device__ const int OFX[8] = {-1, 0, 1, 1, 1, 0, -1, -1};

// ---- _component_best_path (08:295-317) + resample + RDP (08:444-463), one wavefront per skeleton component ----
// Components are contiguous ranges [cs[c], cs[c+1]) of the raster-ordered pixel list `lin`; a pixel's position in that list is its
// compact id (cid canvas), its index inside the range its local id.  nbr[q*8+k] = compact id of the k-th _OFFS neighbour (or ~0).
// The BFS keeps the reference's FIFO order exactly: the queue is consumed eight nodes (64 (node, direction) pairs) at a time, a pixel
// reached by several pairs of one chunk goes to the lowest pair, and winners are appended in pair order.
__global__ __launch_bounds__(256) void k_cid_fill(const unsigned* __restrict__ lin, unsigned m, unsigned* __restrict__ cid) {
    unsigned q = blockIdx.x * 256 + threadIdx.x; if (q < m) cid[lin[q]] = q;
}
// (sk: the thinned bit plane, Wwp words per row; cid is defined at its set pixels only)
__global__ __launch_bounds__(256) void k_nbr_build(const unsigned* __restrict__ lin, unsigned m, const unsigned long long* __restrict__ sk, const unsigned* __restrict__ cid, int Wp, int Hp, int Wwp,
                                                   unsigned* __restrict__ nbr) {
    size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; if (t >= (size_t)m * 8) return;
    unsigned q = (unsigned)(t >> 3); int k = (int)(t & 7);
    unsigned p = lin[q]; int y = (int)(p / Wp) + OFY[k], x = (int)(p % Wp) + OFX[k];
    unsigned v = ~0u;
    if (y >= 0 && y < Hp && x >= 0 && x < Wp && ((sk[(size_t)y * Wwp + (x >> 6)] >> (x & 63)) & 1ULL)) v = cid[(size_t)y * Wp + x];
    nbr[t] = v;
}
// class lists: 0 = fits the small LDS layout, 1 = the large one, 2 = global scratch
__global__ __launch_bounds__(256) void k_comp_classes(const unsigned* __restrict__ corder, unsigned nc, const unsigned* __restrict__ cs, unsigned cap0, unsigned cap1, int need,
                                                      unsigned* __restrict__ counts, unsigned* __restrict__ l0, unsigned* __restrict__ l1, unsigned* __restrict__ l2, unsigned* __restrict__ outcnt) {
    unsigned oi = blockIdx.x * 256 + threadIdx.x; if (oi >= nc) return;
    unsigned c = corder[oi]; unsigned s = cs[c + 1] - cs[c];
    outcnt[oi] = 0;
    if ((int)s < need) return;                              // a path cannot be longer than its component
    if (s <= cap0) l0[atomicAdd(&counts[0], 1u)] = oi;
    else if (s <= cap1) l1[atomicAdd(&counts[1], 1u)] = oi;
    else l2[atomicAdd(&counts[2], 1u)] = oi;
}

template <bool LDSV> struct CompWork;
template <> struct CompWork<true> {
    typedef uint16_t Id; typedef ushort2 Stk;
    static constexpr unsigned NONE = 0xffffu;
    Id* nb; Id* prev; Id* que; float* cum; u8* seen; float2* P; Stk* stk; u8* keep;
    __device__ __forceinline__ unsigned nbr_of(unsigned u, int k) const { return nb[u * 8 + k]; }
};
template <> struct CompWork<false> {
    typedef uint32_t Id; typedef int2 Stk;
    static constexpr unsigned NONE = 0xffffffffu;
    const unsigned* nbr; unsigned b;
    Id* prev; Id* que; float* cum; u8* seen; float2* P; Stk* stk; u8* keep;
    __device__ __forceinline__ unsigned nbr_of(unsigned u, int k) const { unsigned v = nbr[(size_t)(b + u) * 8 + k]; return v == ~0u ? NONE : v - b; }
};
// FIFO BFS from src over local ids; stops when goal is dequeued (goal == NONE: full sweep).  Returns the last dequeued node.
template <class WK> __device__ unsigned bfs_wave(WK& w, unsigned src, unsigned goal, u8 stamp, int lane) {
    if (lane == 0) { w.que[0] = (typename WK::Id)src; w.seen[src] = stamp; w.prev[src] = (typename WK::Id)WK::NONE; }
    __syncthreads();
    unsigned head = 0, tail = 1;
    const int slot = lane >> 3, dir = lane & 7;
    const unsigned long long lt = (1ull << lane) - 1ull;
    while (head < tail) {
        unsigned nn = min(8u, tail - head);
        unsigned u = (unsigned)slot < nn ? (unsigned)w.que[head + slot] : WK::NONE;
        bool hit = false;
        if (goal != WK::NONE) {
            unsigned long long gm = __ballot((unsigned)slot < nn && u == goal);
            if (gm) { nn = (unsigned)((__ffsll((long long)gm) - 1) >> 3); hit = true; }
        }
        bool act = (unsigned)slot < nn;
        unsigned v = act ? w.nbr_of(u, dir) : WK::NONE;
        bool nw = act && v != WK::NONE && w.seen[v] != stamp;
        unsigned long long cand = __ballot(nw), win = 0;
        while (cand) {
            int L = __ffsll((long long)cand) - 1;
            unsigned vL = (unsigned)__shfl((int)v, L, 64);
            unsigned long long dup = __ballot(nw && v == vL);
            win |= 1ull << L; cand &= ~dup;
        }
        if ((win >> lane) & 1ull) {
            unsigned pos = tail + (unsigned)__popcll(win & lt);
            w.que[pos] = (typename WK::Id)v; w.seen[v] = stamp; w.prev[v] = (typename WK::Id)u;
        }
        tail += (unsigned)__popcll(win);
        head += nn;
        __syncthreads();
        if (hit) return goal;
    }
    return (unsigned)w.que[tail - 1];
}

template <bool LDSV>
__device__ void comp_path_wave(CompWork<LDSV>& w, unsigned oi, unsigned b, unsigned S, unsigned a0c, unsigned a1c, const unsigned* __restrict__ lin, int Wp,
                               int min_len, double step, float eps, unsigned pcap, unsigned omul, int2* __restrict__ outpts, unsigned* __restrict__ outcnt, int lane) {
    typedef CompWork<LDSV> WK;
    const unsigned NONE = WK::NONE;
    const unsigned e = b + S;
    const bool ha = a0c >= b && a0c < e, hb = a1c >= b && a1c < e;       // "comp[a0]" (08:300): the anchor pixel lies in this component
    const unsigned a0 = a0c - b, a1 = a1c - b;
    const int need = max(2, min_len);
    int plen = 0; unsigned pv = NONE;
    if (ha && hb) {
        if (a0 == a1) plen = 1;
        else {
            bfs_wave(w, a0, a1, 1, lane);
            if (w.seen[a1] == 1) pv = a1;
        }
    }
    // length of the prev-chain ending in pv, written backwards into the tail of the queue buffer (which the path then occupies)
    auto backtrack = [&](unsigned endn) -> int {
        int cnt = 0;
        if (lane == 0) { unsigned p = endn; unsigned pos = S; while (p != NONE) { w.que[--pos] = (typename WK::Id)p; p = (unsigned)w.prev[p]; cnt++; } }
        cnt = __shfl(cnt, 0, 64);
        __syncthreads();
        return cnt;
    };
    if (pv != NONE) { plen = backtrack(pv); }
    if (plen < need) plen = 0;
    if (plen == 0) {
        unsigned u = bfs_wave(w, 0u, NONE, 2, lane);                     // seed = first pixel in raster order (08:306)
        unsigned v = bfs_wave(w, u, NONE, 3, lane);
        plen = (u == v) ? 1 : backtrack(v);                              // the sweep from u is _bfs_path's own search, cut at v
        if (plen < need) plen = 0;
    }
    if (plen < 2) return;
    const typename WK::Id* path = w.que + (S - plen);
    auto PX = [&](int k) -> float { return (float)((int)(lin[b + path[k]] % (unsigned)Wp) - PAD8); };
    auto PY = [&](int k) -> float { return (float)((int)(lin[b + path[k]] / (unsigned)Wp) - PAD8); };
    // float32 segment lengths in parallel, then the sequential float32 cumsum (08:444-446)
    for (int k = 1 + lane; k < plen; k += 64) { float dx = PX(k) - PX(k - 1), dy = PY(k) - PY(k - 1); w.cum[k] = sqrtf(dx * dx + dy * dy); }
    __syncthreads();
    if (lane == 0) { float acc = w.cum[1]; w.cum[0] = 0.f; for (int k = 2; k < plen; k++) { acc = acc + w.cum[k]; w.cum[k] = acc; } }
    __syncthreads();
    const float total = w.cum[plen - 1];
    int m;
    if ((double)total <= step) {
        m = plen;
        if ((unsigned)m > pcap) return;      // cannot happen: plen - 1 <= total <= step, and pcap >= min(step, cap) + 2 (LDS) or S (global)
        for (int k = lane; k < plen; k += 64) w.P[k] = make_float2(PX(k), PY(k));
    } else {
        m = (int)ceil((double)total / step);
        if ((unsigned)m > pcap) return;      // cannot happen: total <= sqrt(2) (plen - 1), and pcap >= sqrt(2) cap / step + 2 (LDS) or omul S (global), b_paths
        const float t0 = 0.0f, t1 = (float)(0.0 + step), delta = t1 - t0;
        for (int i = lane; i < m; i += 64) {
            float tf = i == 0 ? t0 : (i == 1 ? t1 : t0 + (float)i * delta);
            double t = (double)tf;
            int lo = 0, hi = plen - 2;                                   // k = #{ j in [1, plen-2] : s[j] <= t }  (searchsorted right - 1, clipped)
            while (lo < hi) { int mid = (lo + hi + 1) >> 1; if ((double)w.cum[mid] <= t) lo = mid; else hi = mid - 1; }
            int k = lo;
            double sk = (double)w.cum[k], sk1 = (double)w.cum[k + 1];
            float ax = PX(k), ay = PY(k), bx = PX(k + 1), by = PY(k + 1);
            double u = (t - sk) / fmax(1e-6, sk1 - sk);
            double a = 1.0 - u;
            w.P[i] = make_float2((float)((double)ax * a + (double)bx * u), (float)((double)ay * a + (double)by * u));
        }
    }
    if (m < 2) return;
    // RDP, explicit LIFO stack (08:453-462); the farthest point of a span is found 64 points at a time
    for (int i = lane; i < m; i += 64) w.keep[i] = (i == 0 || i == m - 1) ? 1 : 0;
    int sp = 0;
    if (lane == 0) { w.stk[0].x = 0; w.stk[0].y = (decltype(w.stk[0].y))(m - 1); }
    sp = 1;
    __syncthreads();
    while (sp > 0) {
        --sp;
        const int s = (int)w.stk[sp].x, en = (int)w.stk[sp].y;
        __syncthreads();
        if (en <= s + 1) continue;
        float ax = w.P[s].x, ay = w.P[s].y, bx = w.P[en].x, by = w.P[en].y;
        float segx = bx - ax, segy = by - ay, nx = -segy, ny = segx;
        float q = segx * segx + segy * segy;
        double seg_len = (double)sqrtf(q) + 1e-12; float seg_len_f = (float)seg_len;
        float bestd = -1.f; int bi = 0x7fffffff;
        for (int i = s + 1 + lane; i < en; i += 64) {
            float dx = w.P[i].x - ax, dy = w.P[i].y - ay;
            float t0 = dx * nx, t1 = dy * ny;
            float d = fabsf(t0 + t1) / seg_len_f;
            if (d > bestd) { bestd = d; bi = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            float od = __shfl_xor(bestd, o, 64); int oi2 = __shfl_xor(bi, o, 64);
            if (od > bestd || (od == bestd && oi2 < bi)) { bestd = od; bi = oi2; }
        }
        if (bestd > eps) {
            if (lane == 0) {
                w.keep[bi] = 1;
                w.stk[sp].x = (decltype(w.stk[0].x))s; w.stk[sp].y = (decltype(w.stk[0].y))bi;
                w.stk[sp + 1].x = (decltype(w.stk[0].x))bi; w.stk[sp + 1].y = (decltype(w.stk[0].y))en;
            }
            sp += 2;
        }
        __syncthreads();
    }
    int2* o = outpts + (size_t)b * omul; unsigned cnt = 0;      // the component's region: omul S points >= m >= the kept ones
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int i0 = 0; i0 < m; i0 += 64) {
        int i = i0 + lane; bool kp = i < m && w.keep[i];
        unsigned long long bm = __ballot(kp);
        if (kp) { float2 p = w.P[i]; o[cnt + (unsigned)__popcll(bm & lt)] = make_int2((int)p.x, (int)p.y); }
        cnt += (unsigned)__popcll(bm);
    }
    if (lane == 0) outcnt[oi] = cnt;
}

struct CompArgs {
    const unsigned* corder; const unsigned* cs; const unsigned* lin; const unsigned* gid; const GroupInfo* g; const unsigned* cid; const unsigned* nbr;
    int Wp; int min_len; double step; float eps; unsigned omul; int2* outpts; unsigned* outcnt;      // omul: resample / output points per component pixel (1 or 2)
};
__device__ __forceinline__ void comp_anchors(const CompArgs& A, unsigned b, unsigned& a0c, unsigned& a1c) {
    const GroupInfo* G = A.g + (A.gid[A.lin[b]] - 1);
    a0c = (G->near0 == ~0ULL) ? ~0u : A.cid[(unsigned)(G->near0 & ((1ULL << 27) - 1))];
    a1c = (G->near1 == ~0ULL) ? ~0u : A.cid[(unsigned)(G->near1 & ((1ULL << 27) - 1))];
}
// LDS-resident components (cap nodes, pcap resample points per block)
__global__ __launch_bounds__(64) void k_comp_paths_lds(CompArgs A, const unsigned* __restrict__ list, const unsigned* __restrict__ count, unsigned cap, unsigned pcap) {
    extern __shared__ __align__(16) unsigned char smem[];
    CompWork<true> w;
    w.cum = reinterpret_cast<float*>(smem);
    w.P = reinterpret_cast<float2*>(w.cum + cap);
    w.stk = reinterpret_cast<ushort2*>(w.P + pcap);
    w.nb = reinterpret_cast<uint16_t*>(w.stk + pcap);
    w.prev = w.nb + (size_t)cap * 8; w.que = w.prev + cap;
    w.seen = reinterpret_cast<u8*>(w.que + cap); w.keep = w.seen + cap;
    const int lane = threadIdx.x;
    const unsigned n = *count;
    for (unsigned li = blockIdx.x; li < n; li += gridDim.x) {
        unsigned oi = list[li]; unsigned c = A.corder[oi]; unsigned b = A.cs[c], S = A.cs[c + 1] - b;
        for (unsigned t = lane; t < S * 8; t += 64) { unsigned v = A.nbr[(size_t)b * 8 + t]; w.nb[t] = v == ~0u ? (uint16_t)0xffffu : (uint16_t)(v - b); }
        for (unsigned t = lane; t < S; t += 64) w.seen[t] = 0;
        __syncthreads();
        unsigned a0c, a1c; comp_anchors(A, b, a0c, a1c);
        comp_path_wave<true>(w, oi, b, S, a0c, a1c, A.lin, A.Wp, A.min_len, A.step, A.eps, pcap, A.omul, A.outpts, A.outcnt, lane);
        __syncthreads();
    }
}
// components too large for LDS: same code over per-pixel scratch in global memory
struct CompScratch { unsigned* prev; unsigned* que; float* cum; u8* seen; float2* P; int2* stk; u8* keep; };
__global__ __launch_bounds__(64) void k_comp_paths_glb(CompArgs A, const unsigned* __restrict__ list, const unsigned* __restrict__ count, CompScratch X) {
    const int lane = threadIdx.x;
    const unsigned n = *count;
    for (unsigned li = blockIdx.x; li < n; li += gridDim.x) {
        unsigned oi = list[li]; unsigned c = A.corder[oi]; unsigned b = A.cs[c], S = A.cs[c + 1] - b;
        CompWork<false> w; w.nbr = A.nbr; w.b = b;
        const size_t bp = (size_t)b * A.omul;                  // P, stk and keep hold omul entries per pixel (resample points), the others one
        w.prev = X.prev + b; w.que = X.que + b; w.cum = X.cum + b; w.seen = X.seen + b; w.P = X.P + bp; w.stk = X.stk + bp; w.keep = X.keep + bp;
        for (unsigned t = lane; t < S; t += 64) w.seen[t] = 0;
        __syncthreads();
        unsigned a0c, a1c; comp_anchors(A, b, a0c, a1c);
        comp_path_wave<false>(w, oi, b, S, a0c, a1c, A.lin, A.Wp, A.min_len, A.step, A.eps, S * A.omul, A.omul, A.outpts, A.outcnt, lane);
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_path_desc(const unsigned* __restrict__ corder, const unsigned* __restrict__ cs, const unsigned* __restrict__ outcnt, const unsigned* __restrict__ flag,
                                                    const unsigned* __restrict__ scan, unsigned nc, unsigned omul, GatherDesc* __restrict__ d) {
    unsigned oi = blockIdx.x * 256 + threadIdx.x; if (oi >= nc || !flag[oi]) return;
    GatherDesc g; g.begin = (int64_t)cs[corder[oi]] * omul; g.len = outcnt[oi]; g.rev = 0; g.src = 0;
    d[scan[oi]] = g;
}
__global__ __launch_bounds__(256) void k_flag_nonzero(const unsigned* __restrict__ v, unsigned n, unsigned* __restrict__ f) {
    unsigned i = blockIdx.x * 256 + threadIdx.x; if (i < n) f[i] = v[i] >= 2 ? 1u : 0u; if (i == n) f[i] = 0;
}
__global__ __launch_bounds__(256) void k_concat_taps(const int2* a, int64_t na, const int2* b, int64_t nb, int2* out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < na) out[i] = a[i]; else if (i < na + nb) out[i] = b[i - na];
}

// ================================================================= the phases of stage 08-B
// What flows from one phase of a dedup08_b call to the next: the padded raster's shape, device pointers into the lane's scratch (the slot behind each
// group; orip_ctx.h has the lifetimes) and the counts the host has read back.
struct B08 {
    int64_t n2; int Wp, Hp; size_t Np;                              // lines; the padded raster and its pixel count
    PolyFeat* f2; int* par; unsigned *is_root, *root_scan; GroupInfo* grp;      // VTL_FEAT: features, union-find parents and groups of the lines (groups -> paths)
    unsigned* gid;                                                  // canvas: group root + 1 (raster -> paths), DEFINED AT THE PIXELS THIS CALL STAMPED ONLY: it is never
                                                                    // cleared, anything else is stale (an earlier call or 08-A's first stamps on this lane's canvas).  Every
                                                                    // reader reads it at skeleton pixels -- thinning only deletes, so those were stamped by this call
    int Wwp; size_t nwords; unsigned long long *bA, *bB;            // VTL_STEPLOG: the two thinning bit planes (bA: the current one, the skeleton after the thinning), Wwp words per row
    unsigned M; unsigned *keys, *lin;                               // VTL_CUM: skeleton pixels sorted by component label (lin: their pixel index)
    unsigned NC; unsigned *cs, *corder, *outcnt, *oflag, *oscan; GatherDesc* pd;      // VTL_CAPS: components: first pixel in lin (NC + 1), processing order, path tables
};

// ---- groups: lines whose expanded boxes overlap, their box, longest line and its end points (08:376-400)
static int b_groups(orip_ctx* c, const orip_params08& P, DPolys& lines2, B08& b) {
    const int64_t n2 = b.n2; const int exp = P.post_brush * 2 + 6;
    { Carve L; L.take(b.f2, n2); L.each(n2 + 1, b.par, b.is_root, b.root_scan); L.take(b.grp, n2); HIPC(c, L.commit(LN(c).vtmp[VTL_FEAT], 256)); }
    ORIP_TRY(vfeatures(c, lines2, VF_PER, b.f2));
    hipLaunchKernelGGL(k_iota, dim3(cdiv(n2, 256)), dim3(256), 0, LN(c).stream, b.par, (int)n2);
    { ProfScope ps(c, "k_bbox_pairs"); hipLaunchKernelGGL(k_bbox_pairs, dim3((unsigned)std::min<int64_t>(n2, 8192)), dim3(256), 0, LN(c).stream, b.f2, (int)n2, exp, b.par); }
    hipLaunchKernelGGL(k_group_init, dim3(cdiv(n2, 256)), dim3(256), 0, LN(c).stream, b.grp, (int)n2);
    hipLaunchKernelGGL(k_group_accum, dim3(cdiv(n2 + 1, 256)), dim3(256), 0, LN(c).stream, b.f2, (int)n2, exp, b.par, b.grp, b.is_root);
    ORIP_TRY(vscan_excl<unsigned>(c, b.is_root, b.root_scan, (size_t)n2 + 1));
    hipLaunchKernelGGL(k_group_finish, dim3(cdiv(n2, 256)), dim3(256), 0, LN(c).stream, b.f2, (int)n2, b.is_root, b.root_scan, b.grp);
    return 0;
}
// ---- raster and thin: every group's lines stamped on the padded raster, then Zhang-Suen to the skeleton (bit plane b.bA)
static int b_raster_thin(orip_ctx* c, const orip_params08& P, DPolys& lines2, B08& b, PhaseTimer& T) {
    const int Wp = b.Wp, Hp = b.Hp; const size_t Np = b.Np; const int rad = std::max(1, P.post_brush) / 2;
    HIPC(c, LN(c).canvas.ensure(Np * 4 + 64));
    b.gid = LN(c).canvas.as<unsigned>();
    dim3 blk(256);
    const size_t ntile_max = (size_t)cdiv(Wp, 64) * cdiv(Hp, 4);
    const int Wwp = b.Wwp = (Wp + 63) >> 6; const size_t nwords = b.nwords = (size_t)Hp * Wwp;
    { Carve L; L.each(nwords, b.bA, b.bB);
      HIPC(c, L.commit(LN(c).vtmp[VTL_STEPLOG], 256 + 2 * Np + ntile_max * 4)); }      // (2 Np + 4 ntile_max: what two byte planes and a tile list took; no request shrinks here)
    // nothing passes over the canvas: the bit plane (12.8 MB at the default sheet) is cleared, the stamps set gid and their bits, every later reader goes
    // through the bits (B08::gid)
    HIPC(c, hipMemsetAsync(b.bA, 0, nwords * 8, LN(c).stream));
    { ProfScope ps(c, "k_stamp_groups"); hipLaunchKernelGGL(k_stamp_groups, dim3(8192), dim3(256), 0, LN(c).stream, lines2.off.as<int64_t>(), lines2.pts.as<int32_t>(), b.n2, lines2.total, b.par, rad, b.gid, b.bA, Wp, Hp, Wwp); }
    T.tick("raster");
    // Twelve iterations before the first round trip to the host (16-px lines thin in 9 .. 12), four per round trip after that, each iteration with
    // its own flag: an iteration after the first unchanged one changes nothing either, so running to the end of a batch leaves the image the
    // reference's loop stops with (48 iterations at most: the same cap).  A batch is one launch, tile by tile in LDS.
    int* d_chg = LN(c).flags.as<LaneFlags>()->zs_changed;
    for (int it = 0; it < 48; ) {
        const int nb = it == 0 ? 12 : 4;
        HIPC(c, hipMemsetAsync(d_chg, 0, sizeof(LaneFlags::zs_changed), LN(c).stream));
        { ProfScope ps(c, "k_zs_sub"); hipLaunchKernelGGL(k_zs_tile, dim3((unsigned)cdiv(Wwp, 2), (unsigned)cdiv(Hp, ZS_TR)), blk, 0, LN(c).stream, b.bA, b.bB, Hp, Wwp, nb, d_chg); }
        std::swap(b.bA, b.bB);
        int ch[12] = {0}; ORIP_TRY(vread(c, ch, d_chg, 12));
        bool all = true; for (int q = 0; q < nb; q++) all = all && ch[q] != 0;
        if (!all) break;
        it += nb;
    }
    return 0;
}
// ---- components of the thinned bit plane: their pixels in raster order (b.M of them; nothing more is done when it is 0), each group's anchors, the
// components' processing order
static int b_components(orip_ctx* c, B08& b, PhaseTimer& T) {
    const int Wp = b.Wp, Hp = b.Hp, Wwp = b.Wwp; const size_t nwords = b.nwords;
    dim3 blk(256); const dim3 gwd((unsigned)cdiv((int64_t)nwords, 256));
    HIPC(c, LN(c).vtmp[VTL_SPLIT_FEAT].ensure(b.Np * 4 + 64));
    int* L2 = LN(c).vtmp[VTL_SPLIT_FEAT].as<int>();      // union-find label per pixel of the padded raster (linear id: k_ccl_bits<IdsLinear>, init / merge / flatten)
    hipLaunchKernelGGL(k_ccl_bits<IdsLinear>, gwd, blk, 0, LN(c).stream, b.bA, L2, Hp, Wp, Wwp, 0);
    { ProfScope ps(c, "k_ccl2_merge"); hipLaunchKernelGGL(k_ccl_bits<IdsLinear>, gwd, blk, 0, LN(c).stream, b.bA, L2, Hp, Wp, Wwp, 1); }
    hipLaunchKernelGGL(k_ccl_bits<IdsLinear>, gwd, blk, 0, LN(c).stream, b.bA, L2, Hp, Wp, Wwp, 2);
    T.tick("c:ccl");
    const int nblk = (int)cdiv((int64_t)nwords, 256);
    unsigned *bc, *bo; { Carve L; L.each(nblk + 1, bc, bo); HIPC(c, L.commit(LN(c).vtmp[VTL_RANKS], 64)); }
    HIPC(c, hipMemsetAsync(bc + nblk, 0, 4, LN(c).stream));
    bp_compact_count(LN(c).stream, (unsigned)nblk, b.bA, nwords, bc);
    ORIP_TRY(vscan_excl<unsigned>(c, bc, bo, (size_t)nblk + 1));
    b.M = 0; ORIP_TRY(vread(c, &b.M, bo + nblk));
    const unsigned M = b.M;
    if (M == 0) return 0;
    unsigned *kin, *lin_in;
    { Carve L; L.each(M, kin, lin_in, b.keys, b.lin); HIPC(c, L.commit(LN(c).vtmp[VTL_CUM], 64)); }
    hipLaunchKernelGGL(k_compact_write_bits<Emit08>, dim3(nblk), blk, 0, LN(c).stream, b.bA, nwords, bo, Emit08{L2, Wp, Wwp}, kin, lin_in);
    ORIP_TRY((vsort_pairs<unsigned, unsigned>(c, kin, b.keys, lin_in, b.lin, (size_t)M, 0, 27)));
    unsigned *head, *hs; { Carve L; L.each((size_t)M + 1, head, hs); HIPC(c, L.commit(LN(c).vtmp[VTL_SAMPLES], 64)); }
    bp_heads(LN(c).stream, b.keys, (int64_t)M, (int64_t)M + 1, head);
    ORIP_TRY(vscan_excl<unsigned>(c, head, hs, (size_t)M + 1));
    b.NC = 0; ORIP_TRY(vread(c, &b.NC, hs + M));
    const unsigned NC = b.NC; const size_t nc1 = (size_t)NC + 1;
    unsigned long long *ckin, *ckout; unsigned* cidx;
    { Carve L; L.each(nc1, ckin, ckout); L.take(b.cs, nc1 + 1);
      L.each(nc1, cidx, b.corder, b.outcnt, b.oflag, b.oscan); L.take(b.pd, NC); HIPC(c, L.commit(LN(c).vtmp[VTL_CAPS], 256)); }
    bp_comp_starts(LN(c).stream, head, hs, (int64_t)M, b.cs, NC);
    T.tick("c:sort");
    hipLaunchKernelGGL(k_nearest_anchor, dim3(cdiv(M, 256)), blk, 0, LN(c).stream, b.lin, (int64_t)M, b.gid, Wp, b.grp, ckin, NC);      // (also sets the NC <= M keys to "none yet")
    T.tick("c:anchor");
    hipLaunchKernelGGL(k_comp_keys, dim3(cdiv(M, 256)), blk, 0, LN(c).stream, b.cs, head, hs, M, b.lin, b.gid, Wp, b.grp, ckin, cidx);      // head, hs: VTL_SAMPLES, untouched since the carve above
    if (getenv("ORIP_COMP_DBG")) {      // debug / test hook: the keys as k_comp_keys left them, one line per component in list order.  Waits for the lane's stream.
        std::vector<unsigned long long> hk(NC);
        hipStreamSynchronize(LN(c).stream);
        hipMemcpy(hk.data(), ckin, (size_t)NC * 8, hipMemcpyDeviceToHost);
        for (unsigned q = 0; q < NC; q++) fprintf(stderr, "[comp dbg] rank %u block %u\n", (unsigned)(hk[q] >> 32), (unsigned)hk[q]);
    }
    ORIP_TRY((vsort_pairs<unsigned long long, unsigned>(c, ckin, ckout, cidx, b.corder, (size_t)NC, 0, 64)));
    T.tick("comps");
    return 0;
}
// ---- paths: per component best path, resample, RDP (08:295-317, 444-463); the paths with at least two points -> merged
static int b_paths(orip_ctx* c, const orip_params08& P, B08& b, DPolys& merged, PhaseTimer& T) {
    const int Wp = b.Wp, Hp = b.Hp; const size_t Np = b.Np; const unsigned M = b.M, NC = b.NC; const size_t nc1 = (size_t)NC + 1;
    dim3 blk(256);
    const double stp = P.post_step;                             // >= 1 (dedup08_b), +inf included
    // A path of plen <= S pixels is sqrt(2) (plen - 1) long at most, and its float32 running sum of 1 and fl(sqrt 2) stays within 1.41422 / 1.41421356 of
    // that while the sum is below 2^17 (from there on the ulp is 1/64 and every fl(sqrt 2) term rounds up to 1.421875, 0.5 % high): for paths of up to
    // ~93 000 diagonal pixels, i.e. every LDS component and global ones up to that length.  Longer than the step, a path resamples to
    // m = ceil(total / step) <= ratio S + 1 points; otherwise it passes through with its m = plen <= min(S, step + 1) pixels.  RDP keeps at most m points
    // and holds at most m spans, so m bounds P, stk, keep and the output.  For a step >= 1.41422 that is m <= S: one entry per pixel (omul = 1).  Below
    // it (1 <= step < 1.41422) m <= 1.41422 (S - 1) + 1 <= 2 S, with 40 % to spare for the rounding of any sum: two.  Past the 2^17 limit, at a step in
    // [1.41422, 1.422), m can exceed S in the global class; the m > pcap guard of comp_path_wave then drops that component's line and writes nothing.
    const double ratio = 1.41422 / stp;                         // resample points per component pixel
    const unsigned omul = ratio > 1.0 ? 2u : 1u;
    const double pass = std::min(stp, 65536.0);                 // pixels of a passed-through path, as far as the step bounds them
    auto pcap_of = [&](unsigned cap) { return (unsigned)(cap * ratio) + std::min((unsigned)pass, cap) + 4u; };
    auto cap_of = [&](size_t budget) {                             // bytes: 25/node + 13/resample point; the pass-through room in full, or bounded by cap
        const double a = ((double)budget - 13.0 * (pass + 4.0) - 64.0) / (25.0 + 13.0 * ratio), b2 = ((double)budget - 13.0 * 4.0 - 64.0) / (25.0 + 13.0 * (ratio + 1.0));
        const double cap = std::max(a, b2);                     // (signed: a is negative for a step above budget / 13; b2 >= 576, so no class is ever empty by its sizing)
        return (unsigned)std::min(cap, 65000.0) & ~7u;
    };
    const size_t lds0 = 32 * 1024, lds1 = 160 * 1024;
    unsigned cap0 = cap_of(lds0), cap1 = cap_of(lds1);
    if (const char* ov = getenv("ORIP_COMP_CAPS")) {          // test hook: force components into the larger classes
        unsigned a = 0, b2 = 0; if (sscanf(ov, "%u,%u", &a, &b2) == 2 && a >= 8 && a <= b2) { cap0 = std::min(cap0, a & ~7u); cap1 = std::min(cap1, b2 & ~7u); }
    }
    auto lds_bytes = [&](unsigned cap) { return (size_t)cap * 25 + (size_t)pcap_of(cap) * 13 + 16; };
    // scratch: cid canvas (reuses the BFS canvas), nbr, class lists, global-class work arrays
    unsigned *cid, *nbr, *l0, *l1, *l2; int2* outpts; CompScratch X;
    { Carve L; L.take(cid, Np); L.take(nbr, (size_t)M * 8); L.each(M, X.prev, X.que, X.cum); L.each((size_t)M * omul, X.P, X.stk);
      L.take(outpts, (size_t)M * omul); L.each(nc1, l0, l1, l2); L.take(X.seen, M); L.take(X.keep, (size_t)M * omul); HIPC(c, L.commit(LN(c).vtmp[VTL_CELLS], 1024)); }
    unsigned* counts = LN(c).flags.as<LaneFlags>()->comp_counts;
    HIPC(c, hipMemsetAsync(counts, 0, sizeof(LaneFlags::comp_counts), LN(c).stream));
    hipLaunchKernelGGL(k_cid_fill, dim3(cdiv(M, 256)), blk, 0, LN(c).stream, b.lin, M, cid);
    hipLaunchKernelGGL(k_nbr_build, dim3((unsigned)cdiv((int64_t)M * 8, 256)), blk, 0, LN(c).stream, b.lin, M, b.bA, cid, Wp, Hp, b.Wwp, nbr);
    hipLaunchKernelGGL(k_comp_classes, dim3(cdiv(NC, 256)), blk, 0, LN(c).stream, b.corder, NC, b.cs, cap0, cap1, std::max(2, P.post_minlen), counts, l0, l1, l2, b.outcnt);
    CompArgs A; A.corder = b.corder; A.cs = b.cs; A.lin = b.lin; A.gid = b.gid; A.g = b.grp; A.cid = cid; A.nbr = nbr; A.Wp = Wp; A.min_len = P.post_minlen; A.step = stp;
    A.eps = (float)P.post_eps; A.omul = omul; A.outpts = outpts; A.outcnt = b.outcnt;
    static std::once_flag attr_once;            // several layer threads may arrive here together
    static std::atomic<int> attr_err{0};
    std::call_once(attr_once, [&] { orip_max_lds(k_comp_paths_lds, (int)lds1, attr_err); });
    if (attr_err.load()) ORIP_FAIL(c, "hipFuncSetAttribute(k_comp_paths_lds) failed: %s", hipGetErrorString((hipError_t)attr_err.load()));
    ProfScope ps(c, "k_comp_paths");
    // the few large components are long serial chains: they start on the side stream while the many small ones run here
    HIPC(c, hipEventRecord(LN(c).ev2, LN(c).stream));
    HIPC(c, hipStreamWaitEvent(LN(c).stream2, LN(c).ev2, 0));
    hipLaunchKernelGGL(k_comp_paths_lds, dim3(std::min(NC, 1024u)), dim3(64), lds_bytes(cap1), LN(c).stream2, A, l1, counts + 1, cap1, pcap_of(cap1));
    hipLaunchKernelGGL(k_comp_paths_glb, dim3(std::min(NC, 1024u)), dim3(64), 0, LN(c).stream2, A, l2, counts + 2, X);
    HIPC(c, hipEventRecord(LN(c).ev3, LN(c).stream2));
    hipLaunchKernelGGL(k_comp_paths_lds, dim3(std::min(NC, 8192u)), dim3(64), lds_bytes(cap0), LN(c).stream, A, l0, counts + 0, cap0, pcap_of(cap0));
    HIPC(c, hipStreamWaitEvent(LN(c).stream, LN(c).ev3, 0));
    T.tick("paths");
    hipLaunchKernelGGL(k_flag_nonzero, dim3(cdiv(NC + 1, 256)), blk, 0, LN(c).stream, b.outcnt, NC, b.oflag);
    ORIP_TRY(vscan_excl<unsigned>(c, b.oflag, b.oscan, (size_t)NC + 1));
    unsigned NP = 0; ORIP_TRY(vread(c, &NP, b.oscan + NC));
    HIPC(c, merged.clear(LN(c).stream));
    if (NP) {
        hipLaunchKernelGGL(k_path_desc, dim3(cdiv(NC, 256)), blk, 0, LN(c).stream, b.corder, b.cs, b.outcnt, b.oflag, b.oscan, NC, omul, b.pd);
        ORIP_TRY(vgather(c, b.pd, NP, reinterpret_cast<const int32_t*>(outpts), merged));
    }
    return 0;
}
}  // namespace

int dedup08_b(orip_ctx* c, const orip_params08& P, PhaseTimer& T) {
    DPolys& lines2 = LN(c).tp[2]; DPolys& merged = LN(c).tp[3];
    B08 b{};
    b.n2 = lines2.n;
    if (b.n2 > 0x3fffffff) ORIP_FAIL(c, "too many lines");
    b.Wp = P.W + 2 * PAD8; b.Hp = P.H + 2 * PAD8; b.Np = (size_t)b.Wp * b.Hp;
    if (b.Np >= (1ull << 27)) ORIP_FAIL(c, "canvas too large for stage 08-B index packing");
    // the stamp radius max(1, brush) / 2 must fit the pad, or a band along the canvas border is clipped by the raster (the reference's ROI never clips it)
    if (P.post_brush > 2 * PAD8 + 1) ORIP_FAIL(c, "postmerge brush %d out of range: at most %d (stamp radius brush / 2 <= the %d-px pad)", P.post_brush, 2 * PAD8 + 1, PAD8);
    if (!(P.post_step >= 1.0)) ORIP_FAIL(c, "postmerge_resample_step must be >= 1");
    ORIP_TRY(b_groups(c, P, lines2, b));                   T.tick("groups");
    ORIP_TRY(b_raster_thin(c, P, lines2, b, T));           T.tick("thin");      // (laps "raster" on its way)
    ORIP_TRY(b_components(c, b, T));                       // (laps "c:ccl", and with a skeleton "c:sort", "c:anchor", "comps")
    if (b.M > 0) ORIP_TRY(b_paths(c, P, b, merged, T));    // (laps "paths" on its way)
    else HIPC(c, merged.clear(LN(c).stream));
    HIPC(c, hipGetLastError());
    return 0;
}
