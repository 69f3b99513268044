// csrc/raster04.hip -- stage 04 (04_find_contours.py vectorize_layer, 04:214-230) on gfx950:
//   k_thin_bits04     : one Zhang-Suen sub-iteration on bit planes with the reference's rotated neighbour numbering (04:50-93; bitplane.h: zs_delete)
//   CCL               : orip_ccl_bits (bitplane.h; component order = block-raster)
//   k_bits_to_skel_state : skeleton bytes and per-pixel state byte (fg, endpoint deg==1, junction deg>=3)  (04:128-130)
//   compaction        : popcount / prefix-sum compaction of skeleton pixels in raster order (04:144,174; bitplane.h: bp_compact_count, k_compact_write_bits<Emit04>)
//   radix sort        : rocPRIM stable sort of (layer, component root) keys -> per-component pixel lists
//   k_trace / k_write_walks : the centerline walker (walker.h), exact serial semantics (04:137-205): one wave per component
//                       runs twice (count, then write); the guard-bounded "bounce" tails of phase-2 walks are
//                       detected as cycles of the (prev,cur) state and written by k_expand_cycles in parallel.
#include "bitplane.h"
#include "walker.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstdlib>

__global__ __launch_bounds__(256) void k_gather_head_layers(const unsigned* __restrict__ keys, const unsigned* __restrict__ cs, unsigned nc, unsigned* __restrict__ out) {
    unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < nc) out[i] = keys[cs[i]] >> 26;
}

// ------------------------------------------------------------------------------------------------
// Walker.  NEIGH8 order (dx,dy) from 04:12.
// ------------------------------------------------------------------------------------------------
// one wavefront per component; wave i takes component comp_order[i] (largest components first, so the long serial
// chains start immediately and the small ones fill in behind them)
__global__ __launch_bounds__(64) void k_trace(WalkArgs A) {
    unsigned i = blockIdx.x;
    if (i >= A.nc) return;
    trace_component(A, A.comp_order ? A.comp_order[i] : i);
}
// one wavefront per chunk of `chunk` output points
__global__ __launch_bounds__(64) void k_write_walks(WalkArgs A, int layer, const unsigned* __restrict__ kept_slots, const unsigned long long* __restrict__ kept_off, unsigned n_kept,
                                                    unsigned long long total, unsigned chunk) {
    for (unsigned long long ci = blockIdx.x; ci * chunk < total; ci += gridDim.x) {
        const unsigned long long p0 = ci * chunk, p1 = p0 + chunk < total ? p0 + chunk : total;
        write_chunk(A, layer, kept_slots, kept_off, n_kept, p0, p1);
    }
}
// lengths of the layer's walks (slots [slot0, slot0 + n)); walks that ended inside a recorded trajectory get their closing point settled here.
// opc: own points (n_own + 1) << 32 | tail pieces of a kept walk (one scan sizes both arrays of the walk-coded form)
__global__ void k_totals_flag(const int* __restrict__ over, unsigned* __restrict__ pad_of_total) { *pad_of_total = (unsigned)*over; }
struct WSum {       // what one walk slot adds to the layer's list: one scan sizes and places everything
    unsigned long long pts; unsigned paths, own, pieces, pad;
    __host__ __device__ WSum operator+(const WSum& o) const { WSum r; r.pts = pts + o.pts; r.paths = paths + o.paths; r.own = own + o.own; r.pieces = pieces + o.pieces; r.pad = 0; return r; }
};
__global__ __launch_bounds__(256) void k_winfo_lens(WalkArgs A, unsigned slot0, unsigned n, WSum* __restrict__ ws) {
    unsigned i = blockIdx.x * 256 + threadIdx.x;
    WSum s; s.pts = 0; s.paths = 0; s.own = 0; s.pieces = 0; s.pad = 0;
    if (i < n && !*A.overflow) {                       // (logs of a trace that ran out of room are not followed: the host retries it)
        WalkInfo w = A.winfo[slot0 + i];
        if (w.flags & 2u) { walk_close_tail(A, PlainReader(), slot0 + i, w); A.winfo[slot0 + i] = w; }
        if (w.len_kept) { s.pts = w.len_kept; s.paths = 1u; s.own = w.n_own + 1u; s.pieces = vwalk_pieces(A.logbuf, PlainReader(), w, [](unsigned, unsigned, unsigned, unsigned) {}); }
    }
    if (i <= n) ws[i] = s;
}
// pixel of every log entry in use, and the list of those entries (any order: blocks take their ranges with one atomic each).
// blockIdx.x = component of the layer, blockIdx.y = slice of its entries
__global__ __launch_bounds__(256) void k_ent_fill(WalkArgs A, unsigned c0, unsigned log_shift, int2* __restrict__ lxy, unsigned* __restrict__ ent_idx, unsigned* __restrict__ cnt, unsigned cap) {
    __shared__ unsigned base_s;
    if (*A.overflow) return;
    const unsigned c = c0 + blockIdx.x;
    const unsigned used = A.log_used[c];
    const unsigned per = (used + gridDim.y - 1) / gridDim.y, t0 = blockIdx.y * per, t1 = min(used, t0 + per);
    if (t0 >= t1) return;
    if (threadIdx.x == 0) base_s = atomicAdd(cnt, t1 - t0);
    __syncthreads();
    const unsigned base = base_s;
    const unsigned lb = A.cap_factor * A.comp_start[c] + 64u * c;           // first entry of the component (walker.h: trace_component)
    const unsigned W = (unsigned)A.W;
    for (unsigned t = t0 + threadIdx.x; t < t1; t += 256) {
        const unsigned e = lb + t, lin = A.logbuf[4ull * e] >> 3;
        const unsigned y = lin / W;
        lxy[e - log_shift] = make_int2((int)(lin - y * W), (int)y);
        if (base + (t - t0) < cap) ent_idx[base + (t - t0)] = e - log_shift;
    }
}
// the walk-coded form of the layer's contours: one VWalk per kept walk (path order = slot order), its tail pieces, its offset in the list
__global__ __launch_bounds__(256) void k_vwalk_fill(WalkArgs A, unsigned slot0, unsigned n, const WSum* __restrict__ wo /* exclusive scan */, unsigned log_shift,
                                                     VWalk* __restrict__ vw, VPiece* __restrict__ vp, unsigned* __restrict__ kept_slots, int64_t* __restrict__ off) {
    unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i == n) off[wo[n].paths] = (int64_t)wo[n].pts;
    if (i >= n) return;
    const WSum o = wo[i];
    if (wo[i + 1].paths == o.paths) return;            // not kept
    const WalkInfo w = A.winfo[slot0 + i];
    VWalk v; v.own_off = o.own; v.n_own = w.n_own; v.piece_off = o.pieces; v.len = w.len_kept; v.flags = w.flags & 1u; v.pad0 = v.pad1 = 0;
    VPiece* mine = vp + v.piece_off;
    v.n_piece = vwalk_pieces(A.logbuf, PlainReader(), w, [&](unsigned j, unsigned u0, unsigned ent, unsigned lam) { VPiece q; q.u0 = u0; q.ent = ent - log_shift; q.lam = lam; q.magic = lam > 1u ? (unsigned)(0x100000000ull / lam) : 0xffffffffu; mine[j] = q; });
    const unsigned pi = o.paths;
    vw[pi] = v; kept_slots[pi] = slot0 + i; off[pi] = (int64_t)o.pts;
}
// own points of the kept walks, one wavefront per chunk
__global__ __launch_bounds__(64) void k_vown(WalkArgs A, const unsigned* __restrict__ kept_slots, const VWalk* __restrict__ vw, unsigned n_kept, int2* __restrict__ own, unsigned total, unsigned chunk) {
    for (unsigned long long ci = blockIdx.x; ci * chunk < total; ci += gridDim.x) {
        const unsigned q0 = (unsigned)(ci * chunk), q1 = q0 + chunk < total ? q0 + chunk : total;
        own_chunk(A, kept_slots, vw, n_kept, own, q0, q1);
    }
}


// ---- thinning_zhangsuen (04:35-99) and the state bytes on bit planes: one bit per pixel, 64 pixels per word, blockIdx.z = layer.
// The reference numbers the neighbours from the south (P2 = (y+1, x), then clockwise as seen with y down: SW, W, NW, N, NE, E, SE);
// A(p) counts transitions around the same cycle wherever it starts, B(p) is symmetric, only the two product conditions differ from
// the usual orientation: zs_delete<ZS_ROTATED> of bitplane.h, where the bit-sliced evaluation is described.
__global__ __launch_bounds__(256) void k_thin_bits04(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, int H, int Ww, int sub, int* __restrict__ changed) {
    const size_t nw = (size_t)H * Ww, wi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (wi >= nw) return;
    const unsigned long long* s = src + nw * blockIdx.z; unsigned long long* d = dst + nw * blockIdx.z;
    const unsigned long long M = s[wi];
    if (!M) { d[wi] = 0; return; }
    const unsigned long long del = zs_delete<ZS_ROTATED>(M, neighbour_planes(s, H, Ww, (int)(wi / Ww), (int)(wi % Ww), M), sub);
    if (del) *changed = 1;
    d[wi] = M & ~del;
}
// skeleton bytes (0 / 255) and state bytes (ST_FG | ST_END for degree 1 | ST_JUN for degree >= 3) from the thinned bit planes
__global__ __launch_bounds__(256) void k_bits_to_skel_state(const unsigned long long* __restrict__ bits, u8* __restrict__ skel, u8* __restrict__ st, int H, int W, int Ww,
                                                            unsigned long long* __restrict__ d2bits /* optional: the degree-2 pixels as a bit plane (k_chain_ends_bits) */) {
    const size_t nw = (size_t)H * Ww, w0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (w0 >= nw) return;
    const unsigned long long* s = bits + nw * blockIdx.z;
    u8* sk = skel + (size_t)H * W * blockIdx.z; u8* so = st + (size_t)H * W * blockIdx.z;
    const int lane = threadIdx.x & 63;
    unsigned long long fg = 0, en = 0, ju = 0, d2 = 0;
    auto wi_of = [](size_t a, int l) { return a + (size_t)l; };
    if (w0 + lane < nw) {
        const size_t wi = w0 + lane;
        fg = s[wi];
        if (fg) {
            const Nb8 n = neighbour_planes(s, H, Ww, (int)(wi / Ww), (int)(wi % Ww), fg);
            unsigned long long b0, b1, b2, b3; count8(n, b0, b1, b2, b3);
            en = fg & b0 & ~b1 & ~b2 & ~b3;                   // exactly one neighbour
            ju = fg & (b2 | b3 | (b1 & b0));                  // three or more
            d2 = fg & ~b0 & b1 & ~b2 & ~b3;                   // exactly two: a walk passing through has no choice (walker.h: forced stretches)
        }
        if (d2bits) d2bits[nw * blockIdx.z + wi_of(w0, lane)] = d2;
    }
    if ((W & 63) == 0) {          // a word is 64 whole pixels of one row: every lane writes the 64 skeleton and 64 state bytes of its own word, 16 bytes per store
        if (w0 + lane >= nw) return;
        const size_t px = (w0 + lane) * 64;                 // == y * W + 64 xw
        uint4* ok = reinterpret_cast<uint4*>(sk + px); uint4* oo = reinterpret_cast<uint4*>(so + px);
        auto spread = [](unsigned long long v, int g) { return nib_spread((unsigned)(v >> (4 * g))); };      // 4 bits -> 0 / 1 in 4 bytes
#pragma unroll
        for (int q = 0; q < 4; q++) {
            unsigned a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int g = 4 * q + r;
                const unsigned F = spread(fg, g);
                a[r] = F * 0xffu;
                b[r] = (F << 7) | spread(en, g) | (spread(ju, g) << 1) | (spread(d2, g) << 2);      // ST_FG 0x80, ST_END 1, ST_JUN 2, ST_DEG2 4 (en, ju, d2 are subsets of fg)
            }
            ok[q] = make_uint4(a[0], a[1], a[2], a[3]); oo[q] = make_uint4(b[0], b[1], b[2], b[3]);
        }
        return;
    }
    for (int j = 0; j < 64; j++) {
        const size_t wi = w0 + j; if (wi >= nw) break;
        const unsigned long long f = bcast64(fg, j), e = bcast64(en, j), q = bcast64(ju, j), t2 = bcast64(d2, j);
        const int y = (int)(wi / Ww), x = (int)(wi % Ww) * 64 + lane;
        if (x < W) {
            const bool on = (f >> lane) & 1ULL;
            sk[(size_t)y * W + x] = on ? 255 : 0;
            so[(size_t)y * W + x] = on ? (u8)(ST_FG | (((e >> lane) & 1ULL) ? ST_END : 0) | (((q >> lane) & 1ULL) ? ST_JUN : 0) | (((t2 >> lane) & 1ULL) ? ST_DEG2 : 0)) : (u8)0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Forced stretches (walker.h: ST_CHAIN): maximal chains of degree-2 skeleton pixels, listed when at least ORIP_CHAIN_MIN long.
//   k_chain_ends_bits: a degree-2 pixel with a skeleton neighbour that is not degree-2 ends a chain (from the bit planes, 64 pixels at a time)
//   k_chain_build: one thread per end pixel walks its chain (each pixel has exactly one way on), stepping on the degree-2 bit planes; the end with the
//                  smaller pixel index owns the chain, takes room in cpix with one atomic, walks it again and writes cpix / cref / the state flags
// Runs on lane 0's side stream underneath the component labelling; the traces wait for it.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chain_ends_bits(const unsigned long long* __restrict__ bits, const unsigned long long* __restrict__ d2bits, int H, int W, int Ww,
                                                          unsigned* __restrict__ ends, unsigned* __restrict__ n_ends, unsigned cap) {
    const size_t nw = (size_t)H * Ww, wi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (wi >= nw) return;
    const unsigned long long* d2p = d2bits + nw * blockIdx.z;
    const unsigned long long D = d2p[wi];
    if (!D) return;
    const unsigned long long* fgp = bits + nw * blockIdx.z;
    const int y = (int)(wi / Ww), xw = (int)(wi % Ww);
    auto ND = [&](int yy, int xx) -> unsigned long long { return (yy < 0 || yy >= H || xx < 0 || xx >= Ww) ? 0ULL : (fgp[(size_t)yy * Ww + xx] & ~d2p[(size_t)yy * Ww + xx]); };      // skeleton, not degree 2
    const unsigned long long U = ND(y - 1, xw), UL = ND(y - 1, xw - 1), UR = ND(y - 1, xw + 1), M = ND(y, xw), ML = ND(y, xw - 1), MR = ND(y, xw + 1);
    const unsigned long long Dn = ND(y + 1, xw), DL = ND(y + 1, xw - 1), DR = ND(y + 1, xw + 1);
    const unsigned long long any = U | ((U >> 1) | (UR << 63)) | ((U << 1) | (UL >> 63)) | ((M >> 1) | (MR << 63)) | ((M << 1) | (ML >> 63)) | Dn | ((Dn >> 1) | (DR << 63)) | ((Dn << 1) | (DL >> 63));
    unsigned long long e = D & any;
    while (e) {
        const int j = __ffsll((long long)e) - 1; e &= e - 1;
        const int x = xw * 64 + j;
        if (x >= W) break;
        const unsigned k = atomicAdd(n_ends, 1u);
        if (k < cap) ends[k] = ((unsigned)blockIdx.z << 26) | ((unsigned)y * (unsigned)W + (unsigned)x);
    }
}
__global__ __launch_bounds__(64) void k_chain_build(u8* __restrict__ st, const unsigned long long* __restrict__ d2bits, int H, int W, int Ww, const unsigned* __restrict__ ends,
                                                     const unsigned* __restrict__ n_ends, unsigned cap_ends,
                                                     unsigned* __restrict__ cpix, unsigned* __restrict__ cref, unsigned* __restrict__ n_cpix, unsigned cap_cpix) {
    const unsigned ne = min(*n_ends, cap_ends);
    const unsigned e = blockIdx.x * 64 + threadIdx.x;
    if (e >= ne) return;
    const int layer = (int)(ends[e] >> 26); const unsigned p0 = ends[e] & 0x3ffffffu;
    const int64_t plane = (int64_t)H * W;
    u8* s = st + plane * layer; unsigned* cr = cref + plane * layer;
    const unsigned long long* d2 = d2bits + (size_t)H * Ww * layer;
    // The way on from (y, x), a degree-2 pixel: its degree-2 neighbour that is not the one it came from.  Everything the step tests is in the degree-2 bit
    // plane (ST_DEG2 implies ST_FG: k_bits_to_skel_state; the plane holds no bit outside the image): the word of each of the three rows around the pixel,
    // the word next to it only at bit 0 / 63, give the neighbourhood as nine bits in the scan order dy, dx = -1 .. 1 (bit 3 (dy + 1) + dx + 1); `from` is
    // the bit of the previous pixel (-1: none).  Returns the bit of the first neighbour left in that order, -1: the chain ends here.  No division, and
    // three independent 8-byte loads from 2 MB per layer where the state plane took up to eight dependent byte loads from 16 MB.
    auto next_of = [&](int y, int x, int from) -> int {
        const int xw = x >> 6, j = x & 63;
        auto row3 = [&](int yy) -> unsigned {
            if (yy < 0 || yy >= H) return 0u;
            const unsigned long long* r = d2 + (size_t)yy * Ww;
            const unsigned long long w = r[xw];
            unsigned f = j ? (unsigned)(w >> (j - 1)) & 7u : (unsigned)(w << 1) & 6u;
            if (j == 0 && xw > 0) f |= (unsigned)(r[xw - 1] >> 63);
            if (j == 63 && xw + 1 < Ww) f |= (unsigned)(r[xw + 1] & 1ULL) << 2;
            return f;
        };
        unsigned nb = (row3(y - 1) | (row3(y) << 3) | (row3(y + 1) << 6)) & ~(1u << 4);
        if (from >= 0) nb &= ~(1u << from);
        return nb ? __ffs((int)nb) - 1 : -1;
    };
    const int y0 = (int)(p0 / (unsigned)W), x0 = (int)(p0 % (unsigned)W);
    unsigned m = 1; int y = y0, x = x0, from = -1;
    for (;;) { const int k = next_of(y, x, from); if (k < 0 || m > (1u << 24)) break; y += k / 3 - 1; x += k % 3 - 1; from = 8 - k; m++; }      // (8 - k: the way back)
    const unsigned last = (unsigned)y * (unsigned)W + (unsigned)x;
    if (m < ORIP_CHAIN_MIN || !(p0 < last)) return;                  // short, or the other end owns it
    const unsigned base = atomicAdd(n_cpix, m + 2u);
    if (base + m + 2u > cap_cpix) return;
    cpix[base] = ORIP_CHAIN_SENTINEL; cpix[base + m + 1u] = ORIP_CHAIN_SENTINEL;
    y = y0; x = x0; from = -1;
    for (unsigned j = 0; j < m; j++) {
        const unsigned cur = (unsigned)y * (unsigned)W + (unsigned)x;
        cpix[base + 1u + j] = cur; cr[cur] = base + 1u + j;
        s[cur] = (u8)(s[cur] | ST_CHAIN | ((j == 0 || j == m - 1u) ? ST_CHAIN_END : 0));
        if (j + 1u == m) break;
        const int k = next_of(y, x, from); if (k < 0) break;         // (never: the first traversal took the same steps from the same plane)
        y += k / 3 - 1; x += k % 3 - 1; from = 8 - k;
    }
}

// State kept between orip_contours_prepare and the per-layer trace calls (device buffers live in lane 0's scratch).
struct Prep04 {
    bool ready = false;
    unsigned M = 0, NC = 0;
    int K = 0;                                      // layer count the schedule was built for (c->K may change afterwards)
    std::vector<unsigned> h_cs, layer_first;       // comp_start on the host; first component of every layer (+ sentinel)
    const unsigned* order = nullptr;                // components by (layer, size descending)
    WalkArgs A;                                     // shared arguments (state bytes, keys, lin, comp_start, memo, winfo, total_fg)
    unsigned F[ORIP_MAX_LAYERS];                    // log capacity factor of the layer's latest trace; 0: not traced since the prepare
    bool launched[ORIP_MAX_LAYERS];
    bool chains = false;                            // forced stretches are listed (cref / cpix) and flagged in the state plane
};
void orip_contours_free(orip_ctx* c) { delete static_cast<Prep04*>(c->prep04); c->prep04 = nullptr; }
// The schedule reads the state bytes (tmpC), chain lists and keys of lane 0's scratch, which the raster stages and the next prepare rewrite: a trace
// that prepare enqueued and nobody finished may still be running on its lane, so that lane is waited for first (the resident chain finishes every
// layer it traced, so nothing waits there).  Called by every entry point that replaces the image, masks, edges or layer count, and by prepare.
int orip_contours_invalidate(orip_ctx* c) {
    Prep04* R = static_cast<Prep04*>(c->prep04);
    if (!R) return 0;
    R->ready = false;
    for (int l = 0; l < ORIP_MAX_LAYERS; l++)
        if (R->launched[l]) { HIPC(c, hipStreamSynchronize(c->ln[l + 1].stream)); R->launched[l] = false; }
    return 0;
}
// initial log capacity factor of a trace (ORIP_TRACE_LOG_F: a test hook that makes the overflow retry of trace_finish run)
static unsigned trace_log_f0() {
    const char* e = getenv("ORIP_TRACE_LOG_F");
    const int f = e ? atoi(e) : 0;
    return f >= 1 && f <= 64 ? (unsigned)f : 64u;
}

__global__ __launch_bounds__(256) void k_comp_order_keys(const unsigned* __restrict__ keys, const unsigned* __restrict__ cs, unsigned nc, unsigned long long* __restrict__ k, unsigned* __restrict__ idx) {
    unsigned c = blockIdx.x * 256 + threadIdx.x;
    if (c < nc) { k[c] = ((unsigned long long)(keys[cs[c]] >> 26) << 32) | (unsigned)~(cs[c + 1] - cs[c]); idx[c] = c; }
}
__global__ __launch_bounds__(256) void k_clear_visited_layer(u8* __restrict__ st, const unsigned* __restrict__ lin, int64_t m) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) st[lin[i]] &= (u8)~ST_VIS;
}
// zeroes the eight memo words of every skeleton pixel of one layer (m2 = two 16-byte halves per pixel of lin; neighbouring lanes share a 32-byte line)
__global__ __launch_bounds__(256) void k_clear_memo_layer(uint4* __restrict__ memo, const unsigned* __restrict__ lin, int64_t m2) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m2) memo[((size_t)lin[i >> 1] << 1) | (size_t)(i & 1)] = make_uint4(0u, 0u, 0u, 0u);
}
__global__ __launch_bounds__(256) void k_kept_slots_base(const unsigned* __restrict__ kept, const unsigned* __restrict__ path_off, const unsigned long long* __restrict__ pts_off, unsigned n, unsigned base,
                                                         unsigned* __restrict__ slots, unsigned long long* __restrict__ slot_off) {
    unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && kept[i]) { slots[path_off[i]] = base + i; slot_off[path_off[i]] = pts_off[i]; }
}

// Everything of stage 04 that is batched over the layers: thinning, components, state bytes, the raster-ordered pixel list
// sorted by component, the per-layer schedule.  Runs on lane 0 and ends synchronised.
// Hint for the resident chain: the image is set and K layers will be traced.  Ends the schedule of the previous image and makes sure the K memo planes
// are allocated NOW, so that a growing hipMalloc happens at the start of a step and not in front of the walks.  It clears nothing: the planes are never
// cleared as a whole (WalkArgs::memo), every trace_launch zeroes the words its walk can read.
extern "C" int orip_contours_reserve(orip_ctx* c, int K) {
    orip_enter(c);
    if (!c->image.p || c->H <= 0 || c->W <= 0) ORIP_FAIL(c, "no image set");
    if (K < 1 || K > ORIP_MAX_LAYERS) ORIP_FAIL(c, "K=%d out of range 1..%d", K, ORIP_MAX_LAYERS);
    ORIP_TRY(orip_contours_invalidate(c));
    HIPC(c, LN(c).vtmp[VT0_MEMO].ensure((size_t)c->H * c->W * (size_t)K * 8 * 4 + 64));
    return 0;
}

static int trace_launch(orip_ctx* c, Prep04& R, int layer, unsigned F);
extern "C" int orip_contours_prepare(orip_ctx* c) {
    orip_enter(c);
    if (!c->edges.p || c->K < 1) ORIP_FAIL(c, "no edges resident (run orip_detect_edges or orip_set_edges)");
    const int H = c->H, W = c->W, K = c->K;
    if (H > 8192 || W > 8192) ORIP_FAIL(c, "image %dx%d exceeds the 8192x8192 limit of the component key packing", W, H);
    if (!c->prep04) c->prep04 = new Prep04();
    ORIP_TRY(orip_contours_invalidate(c));      // (traces of the previous prepare still in flight write the lane-0 state rewritten below)
    Prep04& R = *static_cast<Prep04*>(c->prep04);
    R.K = K;
    for (int l = 0; l < ORIP_MAX_LAYERS; l++) { R.launched[l] = false; R.F[l] = 0; }
    const size_t plane = (size_t)H * W; const int64_t n = (int64_t)plane * K;
    // the memo planes (one word per pixel and incoming direction, 0.5 GB per layer at 4096^2) are only sized here: trace_launch zeroes the words of the
    // layer's skeleton pixels, the only ones its walk reads (WalkArgs::memo)
    HIPC(c, LN(c).vtmp[VT0_MEMO].ensure(plane * (size_t)K * 8 * 4 + 64));
    // ---- thinning_zhangsuen (04:35-99): <=120 iterations of two sub-iterations, until nothing is deleted.  On bit planes (2 MB per 4096^2
    // layer): pack, iterate, then skeleton and state bytes in one unpacking pass
    HIPC(c, c->skel.ensure(plane * K + 16));
    HIPC(c, c->tmpB.ensure(plane * K + 16));
    LaneFlags* fl = LN(c).flags.as<LaneFlags>();
    dim3 block(256);
    const int Wb = (W + 1) >> 1, Hb = (H + 1) >> 1; const size_t pplane = (size_t)Wb * Hb * 4;
    HIPC(c, c->tmpC.ensure(plane * K + 16));   // state bytes
    const int Ww = (W + 63) >> 6; const size_t nw = (size_t)H * Ww, nwords = nw * K;
    unsigned long long *bA, *bB;
    HIPC(c, orip_edge_planes(c, nwords, bA, bB));
    dim3 gw((unsigned)cdiv((int64_t)nw, 256), 1, K);
    // bB's lifetime as the degree-2 planes: k_bits_to_skel_state below -> ev3, while k_chain_ends_bits and k_chain_build step on them on the side stream.
    // Its only writers are this call's thinning and k_bits_to_skel_state (orip_detect_edges, the other user of orip_edge_planes, sizes the second set and
    // writes the first only), so the thinning goes behind the chain work of the prepare before -- long finished in a resident chain, whose traces wait for ev3
    if (R.chains) HIPC(c, hipStreamWaitEvent(LN(c).stream, LN(c).ev3, 0));
    if (c->edge_bits != (const void*)bA) bp_pack_bytes(LN(c).stream, gw, c->edges.as<u8>(), bA, H, W, Ww);   // stage 03 may have left them
    c->edge_bits = nullptr;
    // two iterations per round trip to the host, each with its own flag (an iteration after an unchanged one changes nothing either)
    int* d_ch2 = fl->thin_changed;
    for (int it = 0; it < 120; it += 2) {
        HIPC(c, hipMemsetAsync(d_ch2, 0, 8, LN(c).stream));
        for (int b = 0; b < 2; b++) {
            { ProfScope ps(c, "k_thin_bits"); hipLaunchKernelGGL(k_thin_bits04, gw, block, 0, LN(c).stream, bA, bB, H, Ww, 0, d_ch2 + b); }
            { ProfScope ps(c, "k_thin_bits"); hipLaunchKernelGGL(k_thin_bits04, gw, block, 0, LN(c).stream, bB, bA, H, Ww, 1, d_ch2 + b); }
        }
        int h_changed[2] = {0, 0};
        HIPC(c, hipMemcpyAsync(h_changed, d_ch2, 8, hipMemcpyDeviceToHost, LN(c).stream));
        HIPC(c, hipStreamSynchronize(LN(c).stream));
        if (!(h_changed[0] && h_changed[1])) break;
    }
    // bA: the thinned planes; bB (the second thinning plane is free now): the degree-2 pixels
    { ProfScope ps(c, "k_skel_state"); hipLaunchKernelGGL(k_bits_to_skel_state, gw, block, 0, LN(c).stream, bA, c->skel.as<u8>(), c->tmpC.as<u8>(), H, W, Ww, bB); }
    // ---- forced stretches (walker.h: ST_CHAIN), on the side stream underneath the component work below; the traces wait for ev3.
    // Sized from the skeleton of the previous prepare of this context (a resident chain repeats itself), else from the pixel count: chains
    // that do not fit are simply not listed (k_chain_build), the walker then steps through them as before.
    R.chains = !getenv("ORIP_NO_CHAINS");
    if (R.chains) {
        const size_t m_guess = R.M ? (size_t)R.M + R.M / 4 + 4096 : (size_t)(n / 16 + 4096);
        const unsigned cap_ends = (unsigned)std::min<size_t>(m_guess, 0x3fffffffu), cap_cpix = (unsigned)std::min<size_t>(2 * m_guess + 256, 0x7fffffffu);
        HIPC(c, c->cref.ensure(plane * (size_t)K * 4 + 64));
        HIPC(c, c->cpix.ensure((size_t)cap_cpix * 4 + (size_t)cap_ends * 4 + 64));
        unsigned* cpix = c->cpix.as<unsigned>(); unsigned* ends = cpix + cap_cpix;
        unsigned* d_cn = fl->chain_counts;
        hipStream_t s2 = LN(c).stream2;
        HIPC(c, hipEventRecord(LN(c).ev2, LN(c).stream));                            // the state bytes
        HIPC(c, hipStreamWaitEvent(s2, LN(c).ev2, 0));
        HIPC(c, hipMemsetAsync(cpix, 0xff, (size_t)cap_cpix * 4, s2));             // sentinels everywhere, 64 of them in front of the first chain
        const unsigned init[2] = {0u, 64u};
        HIPC(c, hipMemcpyAsync(d_cn, init, 8, hipMemcpyHostToDevice, s2));
        hipLaunchKernelGGL(k_chain_ends_bits, dim3((unsigned)cdiv((int64_t)H * Ww, 256), 1, K), block, 0, s2, bA, bB, H, W, Ww, ends, d_cn, cap_ends);
        hipLaunchKernelGGL(k_chain_build, dim3(cdiv(cap_ends, 64)), dim3(64), 0, s2, c->tmpC.as<u8>(), bB, H, W, Ww, ends, d_cn, cap_ends, cpix, c->cref.as<unsigned>(), d_cn + 1, cap_cpix - 64u);
        HIPC(c, hipEventRecord(LN(c).ev3, s2));
    }
    // ---- components of the thinned bit planes
    HIPC(c, c->tmpD.ensure(pplane * K * sizeof(int)));
    ORIP_TRY(orip_ccl_bits(c, bA, c->tmpD.as<int>(), K));
    // ---- ordered compaction
    const int nblk = (int)cdiv((int64_t)nwords, 256);
    unsigned *d_cnt, *d_boff; { Carve L; L.each(nblk + 1, d_cnt, d_boff); HIPC(c, L.commit(LN(c).tmpE, 64)); }
    HIPC(c, hipMemsetAsync(d_cnt + nblk, 0, sizeof(unsigned), LN(c).stream));
    { ProfScope ps(c, "k_compact_count"); bp_compact_count(LN(c).stream, (unsigned)nblk, bA, nwords, d_cnt); }
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, (const unsigned*)d_cnt, d_boff, 0u, (size_t)nblk + 1, rocprim::plus<unsigned>(), LN(c).stream); }));
    unsigned M = 0;
    HIPC(c, hipMemcpyAsync(&M, d_boff + nblk, sizeof(unsigned), hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    for (int l = 0; l < K; l++) {
        DPolys& P = c->polys[ORIP_SLOT_CONTOURS][l];
        P.n = 0; P.total = 0; P.set_explicit();
        HIPC(c, P.off.ensure(8)); HIPC(c, hipMemsetAsync(P.off.p, 0, 8, LN(c).stream));
    }
    R.M = M; R.NC = 0;
    if (M == 0) { HIPC(c, hipStreamSynchronize(LN(c).stream)); R.ready = true; return 0; }
    // keys / lin (double buffers for the sort)
    unsigned *keys_in, *lin_in, *keys, *lin;
    { Carve L; L.each(M, keys_in, lin_in, keys, lin); HIPC(c, L.commit(LN(c).vtmp[VT0_KEYS], 64)); }
    { ProfScope ps(c, "k_compact_write"); hipLaunchKernelGGL(k_compact_write_bits<Emit04>, dim3(nblk), block, 0, LN(c).stream, bA, nwords, d_boff, Emit04{c->tmpD.as<int>(), nw, H, W, Ww}, keys_in, lin_in); }
    { ProfScope ps(c, "radix_sort_pairs"); HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys, lin_in, lin, (size_t)M, 0, 30, LN(c).stream); })); }
    // ---- component segmentation
    unsigned *head, *head_scan; { Carve L; L.each(M, head, head_scan); HIPC(c, L.commit(LN(c).vtmp[VT0_HEADS], 64)); }
    bp_heads(LN(c).stream, keys, (int64_t)M, (int64_t)M, head);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, (const unsigned*)head, head_scan, 0u, (size_t)M, rocprim::plus<unsigned>(), LN(c).stream); }));
    unsigned last2[2];
    HIPC(c, hipMemcpyAsync(&last2[0], head_scan + (M - 1), 4, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipMemcpyAsync(&last2[1], head + (M - 1), 4, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    const unsigned NC = last2[0] + last2[1];
    R.NC = NC;
    HIPC(c, LN(c).vtmp[VT0_COMP_START].ensure((size_t)(NC + 2) * 4 + 64));
    unsigned* comp_start = LN(c).vtmp[VT0_COMP_START].as<unsigned>();
    bp_comp_starts(LN(c).stream, head, head_scan, (int64_t)M, comp_start, NC);
    R.h_cs.assign(NC + 1, 0); std::vector<unsigned> h_keyfirst(NC);
    HIPC(c, hipMemcpyAsync(R.h_cs.data(), comp_start, (size_t)(NC + 1) * 4, hipMemcpyDeviceToHost, LN(c).stream));
    // layer of each component (key of its first element)
    HIPC(c, LN(c).vtmp[VT0_ORDER].ensure((size_t)NC * 4 + 64));       // (first the layer of each component, then the schedule)
    WalkArgs& A = R.A; memset(&A, 0, sizeof(A));
    A.H = H; A.W = W; A.plane = (int64_t)plane; A.st = c->tmpC.as<u8>(); A.keys = keys; A.lin = lin; A.comp_start = comp_start; A.nc = NC;
    if (R.chains) { A.cref = c->cref.as<unsigned>(); A.cpix = c->cpix.as<unsigned>(); }
    hipLaunchKernelGGL(k_gather_head_layers, dim3(cdiv(NC, 256)), block, 0, LN(c).stream, keys, comp_start, NC, LN(c).vtmp[VT0_ORDER].as<unsigned>());
    HIPC(c, hipMemcpyAsync(h_keyfirst.data(), LN(c).vtmp[VT0_ORDER].p, (size_t)NC * 4, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    std::vector<unsigned>& layer_first = R.layer_first; layer_first.assign(K + 1, NC);
    for (unsigned i = NC; i-- > 0;) layer_first[h_keyfirst[i]] = i;
    for (int l = K - 1; l >= 0; l--) if (layer_first[l] == NC && l + 1 <= K) layer_first[l] = layer_first[l + 1];
    layer_first[K] = NC;
    for (int l = 0; l < K; l++) A.total_fg[l] = (long long)R.h_cs[layer_first[l + 1]] - (long long)R.h_cs[layer_first[l]];
    // per-layer largest-first schedule: components sorted by (layer, size descending); layer l owns order[layer_first[l] .. layer_first[l+1])
    {
        unsigned long long *kin, *kout; unsigned *idin, *idout;
        { Carve L; L.each(NC, kin, kout, idin, idout); HIPC(c, L.commit(LN(c).vtmp[VT0_ORDER_SORT], 64)); }
        hipLaunchKernelGGL(k_comp_order_keys, dim3(cdiv(NC, 256)), block, 0, LN(c).stream, keys, comp_start, NC, kin, idin);
        HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, idin, idout, (size_t)NC, 0, 40, LN(c).stream); }));
        R.order = LN(c).vtmp[VT0_ORDER].as<unsigned>();
        HIPC(c, hipMemcpyAsync(LN(c).vtmp[VT0_ORDER].p, idout, (size_t)NC * 4, hipMemcpyDeviceToDevice, LN(c).stream));
    }
    // shared trace state: memo plane (one word per pixel and incoming direction) and walk records (two slots per skeleton pixel)
    HIPC(c, LN(c).vtmp[VT0_WINFO].ensure((size_t)2 * M * sizeof(WalkInfo) + 64));
    A.memo = LN(c).vtmp[VT0_MEMO].as<unsigned>(); A.winfo = LN(c).vtmp[VT0_WINFO].as<WalkInfo>();       // (the memo planes were sized at the top)
    HIPC(c, LN(c).vtmp[VT0_LOG_USED].ensure((size_t)(NC + 1) * 4 + 64));
    A.log_used = LN(c).vtmp[VT0_LOG_USED].as<unsigned>();         // written by every component's trace
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    R.ready = true;
    // The layers' traces start right here, from the calling thread, each on its layer's lane: the walks head every layer's chain, and the hand-over to the
    // layer threads (orip_contours_layer, which then only waits for its trace) costs 0.3-0.5 ms in which the card would sit idle.  A lane that another
    // thread holds is left to its orip_contours_layer call (ORIP_TRACE_LATE=1: all of them, as before).
    if (!getenv("ORIP_TRACE_LATE"))
        for (int l = 0; l < R.K; l++) {
            if (R.layer_first[l] == R.layer_first[l + 1]) continue;
            LaneGuard g(c, l + 1);
            if (!g.ok) continue;
            HIPC(c, orip_pf08_drain(c));
            ORIP_TRY(trace_launch(c, R, l, trace_log_f0()));
        }
    return 0;
}

// Enqueues the trace pass of one layer on the calling lane's stream (walker.h: one wave per component records step codes, bounce
// trajectories and one WalkInfo per walk).  The logs of the layer live in the lane's scratch; the kernel addresses them with the
// global formula (cap_factor * comp_start + ...), so the base pointers are shifted by the layer's first component.
static int trace_launch(orip_ctx* c, Prep04& R, int layer, unsigned F) {
    const unsigned c0 = R.layer_first[layer], c1 = R.layer_first[layer + 1];
    const unsigned b0 = R.h_cs[c0], b1 = R.h_cs[c1];
    const unsigned Ml = b1 - b0, NCl = c1 - c0;
    const size_t plane = (size_t)R.A.plane;
    if ((uint64_t)F * R.M + (uint64_t)256 * R.NC + 64 >= 0xffffffffull) ORIP_FAIL(c, "skeleton too large for the walk logs (factor %u)", F);
    const size_t nlog = (size_t)F * Ml + (size_t)64 * NCl + 8, nstep = (size_t)F * Ml + (size_t)256 * NCl + 8;
    WalkStore& WS = c->wstore[layer];
    WS.epoch++; WS.n = 0;                              // walk-coded lists built on the previous trace of this layer are stale from here on
    HIPC(c, WS.log.ensure(nlog * 16 + 64));
    HIPC(c, LN(c).vtmp[VTL_STEPLOG].ensure(nstep + 64));
    WalkArgs A = R.A;
    A.logbuf = WS.log.as<unsigned>() - 4 * ((size_t)F * b0 + (size_t)64 * c0);
    A.steplog = LN(c).vtmp[VTL_STEPLOG].as<u8>() - ((size_t)F * b0 + (size_t)256 * c0);
    A.cap_factor = F; A.comp_order = R.order + c0; A.nc = NCl;
    int* d_over = &LN(c).flags.as<LaneFlags>()->trace_overflow; A.overflow = d_over;
    if (R.chains) HIPC(c, hipStreamWaitEvent(LN(c).stream, c->ln[0].ev3, 0));            // the chain lists and flags (orip_contours_prepare, side stream)
    if (R.F[layer])                                  // a retry, or a second trace of the layer after one prepare: the previous walk left the ST_VIS bits of every pixel it reached
        hipLaunchKernelGGL(k_clear_visited_layer, dim3(cdiv(Ml, 256)), dim3(256), 0, LN(c).stream, A.st + plane * layer, A.lin + b0, (int64_t)Ml);
    // the memo words this walk can read: eight per skeleton pixel of the layer.  On EVERY launch -- the words hold what the previous step, an overflowed
    // trace or an earlier trace of this prepare left there
    hipLaunchKernelGGL(k_clear_memo_layer, dim3(cdiv((int64_t)2 * Ml, 256)), dim3(256), 0, LN(c).stream, reinterpret_cast<uint4*>(A.memo + plane * 8 * layer), A.lin + b0, (int64_t)2 * Ml);
    HIPC(c, hipMemsetAsync(A.winfo + 2 * (size_t)b0, 0, (size_t)2 * Ml * sizeof(WalkInfo), LN(c).stream));
    HIPC(c, hipMemsetAsync(d_over, 0, 4, LN(c).stream));
    if (getenv("ORIP_WALK_DBG")) {          // per-component counters (walks, steps, memo hits, closed cycles, tile loads, size), in the leaves' slot until trace_finish
        HIPC(c, LN(c).vtmp[VT_LEAVES].ensure((size_t)NCl * 256 + 64)); HIPC(c, hipMemsetAsync(LN(c).vtmp[VT_LEAVES].p, 0, (size_t)NCl * 256, LN(c).stream));
        A.dbg = LN(c).vtmp[VT_LEAVES].as<unsigned long long>() - 32ull * c0;
    }
    { ProfScope ps(c, "k_trace"); hipLaunchKernelGGL(k_trace, dim3(NCl), dim3(64), 0, LN(c).stream, A); }
    HIPC(c, hipGetLastError());
    R.F[layer] = F; R.launched[layer] = true;
    return 0;
}
// Waits for the trace of the layer (retrying with larger logs on overflow), then sizes, allocates and writes its contours.
static int trace_finish(orip_ctx* c, Prep04& R, int layer) {
    const unsigned c0 = R.layer_first[layer], c1 = R.layer_first[layer + 1];
    const unsigned b0 = R.h_cs[c0], b1 = R.h_cs[c1];
    const unsigned Ml = b1 - b0;
    dim3 block(256);
    int* d_over = &LN(c).flags.as<LaneFlags>()->trace_overflow;
    // offsets: exclusive scans over the layer's walk slots (slot order == output order: components by rank, endpoint walks then leftovers, each in raster order)
    // Nothing waits for the trace first: the sizing kernels are enqueued behind it and the one read below brings its overflow flag along
    // with the totals (an overflowed trace -- rare: the logs hold 64 entries per skeleton pixel -- is redone with larger logs).
    const unsigned nslots = 2u * Ml, sl0 = 2u * b0;
    const size_t ns1 = (size_t)nslots + 1;
    WSum *ws, *wo; { Carve L; L.each(ns1, ws, wo); HIPC(c, L.commit(LN(c).vtmp[VTL_CAPS], 256)); }
    WalkStore& WS = c->wstore[layer];
    WSum h_tot; unsigned log_shift = 0; WalkArgs A;
    for (;;) {
    log_shift = (unsigned)((size_t)R.F[layer] * b0 + (size_t)64 * c0);
    A = R.A;                        // the layer's logs as the trace addressed them (walk_close_tail / vwalk_pieces follow the recorded trajectories)
    A.logbuf = WS.log.as<unsigned>() - 4 * (size_t)log_shift;
    A.steplog = LN(c).vtmp[VTL_STEPLOG].as<u8>() - ((size_t)R.F[layer] * b0 + (size_t)256 * c0);
    A.cap_factor = R.F[layer]; A.overflow = d_over;
    hipLaunchKernelGGL(k_winfo_lens, dim3(cdiv(nslots + 1, 256)), block, 0, LN(c).stream, A, sl0, nslots, ws);
    { WSum zero; zero.pts = 0; zero.paths = zero.own = zero.pieces = zero.pad = 0; HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, ws, wo, zero, ns1, rocprim::plus<WSum>(), LN(c).stream); })); }
    hipLaunchKernelGGL(k_totals_flag, dim3(1), dim3(1), 0, LN(c).stream, d_over, &wo[nslots].pad);
    HIPC(c, hipMemcpyAsync(&h_tot, wo + nslots, sizeof(WSum), hipMemcpyDeviceToHost, LN(c).stream));
    // pixels of the log entries in use (needs nothing from the scan: it runs while the host waits for the totals)
    {
        const unsigned NCl = c1 - c0;
        WS.ent_cap = (int64_t)8 * Ml + 64;                       // a component logs at most one entry per (pixel, incoming direction)
        HIPC(c, WS.lxy.ensure(((size_t)R.F[layer] * Ml + (size_t)64 * NCl + 8) * 8 + 64));
        HIPC(c, WS.ent_idx.ensure((size_t)WS.ent_cap * 4 + 64));
        HIPC(c, WS.cnt.ensure(64));
        HIPC(c, hipMemsetAsync(WS.cnt.p, 0, 4, LN(c).stream));
        hipLaunchKernelGGL(k_ent_fill, dim3(NCl, 8), block, 0, LN(c).stream, A, c0, log_shift, WS.lxy.as<int2>(), WS.ent_idx.as<unsigned>(), WS.cnt.as<unsigned>(), (unsigned)WS.ent_cap);
    }
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    if (!h_tot.pad) break;
    if (h_tot.pad == 2) ORIP_FAIL(c, "internal error: the walker of layer %d stopped making progress", layer);
    ORIP_TRY(trace_launch(c, R, layer, R.F[layer] * 4));      // retry with larger logs
    }
    if (getenv("ORIP_WALK_DBG")) {
        const unsigned NCl = c1 - c0;
        std::vector<unsigned long long> h((size_t)NCl * 32);
        HIPC(c, hipMemcpy(h.data(), LN(c).vtmp[VT_LEAVES].p, h.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long tot[32] = {0}; size_t big = 0;
        for (size_t i = 0; i < h.size(); i++) tot[i % 32] += h[i];
        for (size_t i = 0; i < NCl; i++) if (h[i * 32 + 7] > h[big * 32 + 7]) big = i;
        const unsigned long long* d = &h[big * 32];
        fprintf(stderr, "[walk dbg] layer %d NC=%u M=%u F=%u: w1=%llu s1=%llu w2=%llu s2=%llu hit=%llu det=%llu tiles=%llu | largest fg=%llu: w1=%llu s1=%llu w2=%llu s2=%llu hit=%llu det=%llu tiles=%llu jumped=%llu calls=%llu rounds=%llu\n",
                layer, NCl, Ml, R.F[layer], tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], tot[6], d[7], d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[15], d[22], d[23]);
        if (d[8]) fprintf(stderr, "[walk prof] layer %d largest component: cycles total=%llu window loads=%llu scans=%llu look-ups=%llu | look-ups=%llu loop exits=%llu\n",
                          layer, d[8], d[9], d[10], d[11], d[12], d[13]);
        if (d[8]) fprintf(stderr, "[walk prof]   inside the look-ups: duplicate check %llu cycles (exact check in %llu look-ups); forced stretches %llu cycles in %llu calls, %llu rounds; stepping loop %llu cycles; walk start + end %llu cycles\n", d[14], d[20], d[16], d[17], d[18], d[19], d[21]);
    }
    const unsigned long long h_pts = h_tot.pts; const unsigned h_paths = h_tot.paths, h_own = h_tot.own, h_pieces = h_tot.pieces;
    // ---- the contours of the layer in walk-coded form (walker.h): nothing is expanded here
    DPolys& P = c->polys[ORIP_SLOT_CONTOURS][layer];
    P.total = (int64_t)h_pts; P.n = (int64_t)h_paths;
    P.virt = true; P.pts_ok = false; P.vident = true; P.vlayer = layer; P.vepoch = WS.epoch; P.scaled = false;
    HIPC(c, P.off.ensure((size_t)(P.n + 1) * 8 + 64));
    HIPC(c, WS.walk.ensure((size_t)std::max(h_paths, 1u) * sizeof(VWalk) + 64));
    HIPC(c, WS.piece.ensure((size_t)std::max(h_pieces, 1u) * sizeof(VPiece) + 64));
    HIPC(c, WS.own.ensure((size_t)std::max(h_own, 1u) * 8 + 64));
    HIPC(c, LN(c).vtmp[VTL_CELLS].ensure((size_t)std::max(h_paths, 1u) * 4 + 64));
    unsigned* kept_slots = LN(c).vtmp[VTL_CELLS].as<unsigned>();
    WS.n = P.n; WS.W = R.A.W; WS.n_own = h_own;
    hipLaunchKernelGGL(k_vwalk_fill, dim3(cdiv(nslots + 1, 256)), block, 0, LN(c).stream, A, sl0, nslots, wo, log_shift,
                       WS.walk.as<VWalk>(), WS.piece.as<VPiece>(), kept_slots, P.off.as<int64_t>());
    if (h_paths) {
        ProfScope ps(c, "k_write_walks");
        const unsigned chunk = 2048;
        hipLaunchKernelGGL(k_vown, dim3((unsigned)std::min<unsigned long long>(((unsigned long long)h_own + chunk - 1) / chunk, 262144ull)), dim3(64), 0, LN(c).stream, A, kept_slots, WS.walk.as<VWalk>(), h_paths,
                           WS.own.as<int2>(), h_own, chunk);
    }
    HIPC(c, hipGetLastError());
    R.launched[layer] = false;
    return 0;
}

// Contours of one layer (after orip_contours_prepare).  Runs on the layer's own lane, so different layers can be traced from
// different host threads at the same time and a finished layer can move on to stages 05-08 while others are still walking.
int orip_contours_layer_impl(orip_ctx* c, int layer, bool sync) {
    Prep04* R = static_cast<Prep04*>(c->prep04);
    if (!R || !R->ready) ORIP_FAIL(c, "orip_contours_prepare has not run");
    if (layer < 0 || layer >= R->K) ORIP_FAIL(c, "bad layer %d (prepared for %d layers)", layer, R->K);
    if (R->M == 0 || R->layer_first[layer] == R->layer_first[layer + 1]) return 0;
    ORIP_LANE(c, layer + 1);
    if (!R->launched[layer]) ORIP_TRY(trace_launch(c, *R, layer, trace_log_f0()));      // (normally enqueued by orip_contours_prepare already)
    ORIP_TRY(trace_finish(c, *R, layer));
    if (sync) HIPC(c, hipStreamSynchronize(LN(c).stream));
    return 0;
}
extern "C" int orip_contours_layer(orip_ctx* c, int layer) {
    orip_enter(c);
    return orip_contours_layer_impl(c, layer, true);
}

extern "C" int orip_find_contours(orip_ctx* c) {
    orip_enter(c);
    ORIP_TRY(orip_contours_prepare(c));
    Prep04& R = *static_cast<Prep04*>(c->prep04);
    if (R.M == 0) return 0;
    // every layer's trace is enqueued on its own stream first, so the long serial walks of all layers overlap
    for (int l = 0; l < R.K; l++) if (R.layer_first[l] != R.layer_first[l + 1] && !R.launched[l]) { ORIP_LANE(c, l + 1); ORIP_TRY(trace_launch(c, R, l, trace_log_f0())); }
    for (int l = 0; l < R.K; l++) if (R.launched[l]) { ORIP_LANE(c, l + 1); ORIP_TRY(trace_finish(c, R, l)); HIPC(c, hipStreamSynchronize(LN(c).stream)); }
    return 0;
}

extern "C" int orip_get_skeleton(orip_ctx* c, int layer, uint8_t* out) {
    orip_enter(c);
    if (!c->skel.p || layer < 0 || layer >= c->K) ORIP_FAIL(c, "no skeleton for layer %d", layer);
    size_t plane = (size_t)c->H * c->W;
    HIPC(c, hipMemcpyAsync(out, c->skel.as<u8>() + plane * layer, plane, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    return 0;
}
