// csrc/bitplane.h -- the building blocks of everything that works on BIT PLANES (one bit per pixel, 64 pixels per word, rows of Ww = ceil(W / 64)
// words, bit j of word xw = pixel 64 xw + j; bits past W in a row's last word are zero): raster stages 02-04 and stage 08-B ("Bit planes").
//   device-inline pieces  the union-find, the block-raster pixel id, the 64-bit readlane broadcast, the nibble <-> 4 bytes multiply, the eight neighbour
//                         planes of a word with their carry-save count and transition test, the Zhang-Suen delete word, the block-wide popcount position
//   kernel templates      k_ccl_bits<Ids>, k_pack_bits<Pred>, k_compact_write_bits<Emit> over small plain policy structs.  Each instantiation is compiled
//                         in exactly ONE unit (the rule of vec_common.h): <IdsBlockRaster> and <PackBytes> (stages 02 and 04 both pack bytes: bp_pack_bytes)
//                         in bitplane.hip, <PackLabels> in raster02.hip, <Emit04> in raster04.hip, <IdsLinear> / <Emit08> in vector08b.hip (whose stamps set their own bits: it packs nothing)
//   bitplane.hip          the kernels that need no policy (bits -> bytes, compaction count, segment heads, component starts) behind the bp_* launchers,
//                         and orip_ccl_bits, the CCL driver of stages 03 / 04
#pragma once
#include "orip_ctx.h"

// ---- lock-free union-find over int labels: the root of a set is its minimum id; a union hangs the larger root under the smaller with one atomicMin and
// retries from whatever it found there when another thread got in first
__device__ __forceinline__ int uf_find(const int* L, int a) {
    int p = L[a];
    while (p != a) { a = p; p = L[a]; }
    return a;
}
__device__ __forceinline__ void uf_unite(int* L, int a, int b) {
    bool done;
    do {
        a = uf_find(L, a); b = uf_find(L, b);
        if (a < b) { int old = atomicMin(&L[b], a); done = (old == b); b = old; }
        else if (b < a) { int old = atomicMin(&L[a], b); done = (old == a); a = old; }
        else done = true;
    } while (!done);
}
// BLOCK-RASTER id of a pixel, Wb = (W + 1) / 2: 2x2 blocks in raster order, the four pixels of a block in raster order inside it.  The minimum id of a
// component names the first 2x2 block that holds one of its pixels: the label order block-based CCL scanners produce
__device__ __forceinline__ int px_id(int y, int x, int Wb) { return (((y >> 1) * Wb + (x >> 1)) << 2) | ((y & 1) << 1) | (x & 1); }
// lane j's 64-bit value in every lane (j uniform): two scalar readlanes
__device__ __forceinline__ unsigned long long bcast64(unsigned long long v, int j) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), j) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, j);
}
// 4 bits -> 0 / 1 in 4 bytes and back: n * (1 + 2^7 + 2^14 + 2^21) drops bit i at position 8 i (no carries); the same multiply lifts the bits 0, 8, 16, 24
// of a word to bits 21 .. 24
__device__ __forceinline__ unsigned nib_spread(unsigned n4) { return ((n4 & 0xfu) * 0x00204081u) & 0x01010101u; }
__device__ __forceinline__ unsigned nib_gather(unsigned b4) { return ((b4 * 0x00204081u) >> 21) & 0xfu; }

// ---- the eight neighbour planes of a word M: bit j of n.NE = the pixel north-east of pixel j, ...  Built from the nine words of the 3x3 word
// neighbourhood (U / D: the rows above / below, L / R: the words left / right; out-of-image words are passed as 0) by shifts
struct Nb8 { unsigned long long N, NE, E, SE, S, SW, W, NW; };
__device__ __forceinline__ Nb8 nb8_of(unsigned long long M, unsigned long long U, unsigned long long UL, unsigned long long UR, unsigned long long ML, unsigned long long MR,
                                      unsigned long long D, unsigned long long DL, unsigned long long DR) {
    Nb8 n; n.N = U; n.NE = (U >> 1) | (UR << 63); n.E = (M >> 1) | (MR << 63); n.SE = (D >> 1) | (DR << 63);
    n.S = D; n.SW = (D << 1) | (DL >> 63); n.W = (M << 1) | (ML >> 63); n.NW = (U << 1) | (UL >> 63);
    return n;
}
// ... of word (y, xw) of a plane in global memory ([H][Ww] words)
__device__ __forceinline__ Nb8 neighbour_planes(const unsigned long long* __restrict__ s, int H, int Ww, int y, int xw, unsigned long long M) {
    auto W64 = [&](int yy, int xx) -> unsigned long long { return (yy < 0 || yy >= H || xx < 0 || xx >= Ww) ? 0ULL : s[(size_t)yy * Ww + xx]; };
    return nb8_of(M, W64(y - 1, xw), W64(y - 1, xw - 1), W64(y - 1, xw + 1), W64(y, xw - 1), W64(y, xw + 1), W64(y + 1, xw), W64(y + 1, xw - 1), W64(y + 1, xw + 1));
}
// bit-sliced neighbour count through a carry-save adder tree: b0 ones, b1 twos, b2 fours, b3 eights
__device__ __forceinline__ void count8(const Nb8& n, unsigned long long& b0, unsigned long long& b1, unsigned long long& b2, unsigned long long& b3) {
    auto FA = [](unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long& sum, unsigned long long& carry) { const unsigned long long t = a ^ b; sum = t ^ c; carry = (a & b) | (t & c); };
    unsigned long long s1, c1, s2, c2, s4, c4, s5, c5;
    FA(n.N, n.NE, n.E, s1, c1); FA(n.SE, n.S, n.SW, s2, c2);
    const unsigned long long s3 = n.W ^ n.NW, c3 = n.W & n.NW;
    FA(s1, s2, s3, s4, c4); FA(c1, c2, c3, s5, c5);
    const unsigned long long c6 = s5 & c4;
    b0 = s4; b1 = s5 ^ c4; b2 = c5 ^ c6; b3 = c5 & c6;
}
// A == 1: exactly one 0 -> 1 transition around the cycle N, NE, E, SE, S, SW, W, NW, N (the count does not depend on where the cycle is entered).
// `one`: some transition seen, `two`: a second one
__device__ __forceinline__ unsigned long long one_transition(const Nb8& n) {
    unsigned long long one = 0, two = 0;
    auto TR = [&](unsigned long long a, unsigned long long b) { const unsigned long long t = ~a & b; two |= one & t; one |= t; };
    TR(n.N, n.NE); TR(n.NE, n.E); TR(n.E, n.SE); TR(n.SE, n.S); TR(n.S, n.SW); TR(n.SW, n.W); TR(n.W, n.NW); TR(n.NW, n.N);
    return one & ~two;
}
// One Zhang-Suen sub-iteration (sub = 0 / 1) on a word: the pixels of M it deletes.  2 <= B <= 6 and A == 1 are the same in every numbering of the
// neighbours; the two product conditions are not.  ZS_STANDARD: P2 = north, then clockwise (08:349-366).  ZS_ROTATED: the numbering of stage 04's
// reference, P2 = south = (y + 1, x), then SW, W, NW, N, NE, E, SE (04:50-93), i.e. the standard one turned by half a turn.
enum ZsOrient { ZS_STANDARD = 0, ZS_ROTATED = 1 };
template <ZsOrient O>
__device__ __forceinline__ unsigned long long zs_delete(unsigned long long M, const Nb8& n, int sub) {
    unsigned long long b0, b1, b2, b3; count8(n, b0, b1, b2, b3);
    const unsigned long long Bok = (b1 | b2) & ~b3 & ~(b2 & b1 & b0);          // 2 <= B <= 6
    const unsigned long long P2 = O == ZS_STANDARD ? n.N : n.S, P4 = O == ZS_STANDARD ? n.E : n.W, P6 = O == ZS_STANDARD ? n.S : n.N, P8 = O == ZS_STANDARD ? n.W : n.E;
    const unsigned long long cnd = sub == 0 ? (~(P2 & P4 & P6) & ~(P4 & P6 & P8)) : (~(P2 & P4 & P8) & ~(P2 & P6 & P8));
    return M & one_transition(n) & Bok & cnd;
}
// Position of this thread's `cnt` items among those of its block of 256 threads, in thread order (exclusive): a shuffle scan inside the wave, LDS across
// the 4 waves.  Every thread of the block calls it; a thread without items gets 0 and reads no wave sums.
__device__ __forceinline__ unsigned block_excl_pos256(unsigned cnt) {
    __shared__ unsigned wsum[4];
    unsigned inc = cnt;
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) { unsigned t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (!cnt) return 0u;
    unsigned pos = inc - cnt;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) pos += wsum[w];
    return pos;
}

// ---- pixel ids of the CCL.  LAYERED: blockIdx.z = layer, planes of H * Ww words, labels of stride() ints per layer
struct IdsBlockRaster {          // stages 03 / 04: px_id, labels indexed by it with Wb * Hb * 4 per layer
    static constexpr bool LAYERED = true;
    int Wb, Hb;
    __device__ IdsBlockRaster(int H, int W) : Wb((W + 1) >> 1), Hb((H + 1) >> 1) {}
    __device__ size_t stride() const { return (size_t)Wb * Hb * 4; }
    __device__ int at(int y, int x) const { return px_id(y, x, Wb); }
};
struct IdsLinear {               // stage 08-B: y * W + x on the one padded raster
    static constexpr bool LAYERED = false;
    int W;
    __device__ IdsLinear(int, int W_) : W(W_) {}
    __device__ size_t stride() const { return 0; }
    __device__ int at(int y, int x) const { return y * W + x; }
};
// 8-connected components of bit planes by union-find: a thread owns a word, returns at once when it is empty and works on its RUNS (maximal stretches of
// set bits inside the word) otherwise.  An id grows with x along a row (both maps), so the first pixel of a run has the run's smallest id.  mode 0 init:
// every pixel of a run points at the run's first pixel (the forest in between is free: everything downstream reads only the flattened label, the
// component's minimum id).  mode 1 merge, one union per adjacency between runs instead of up to four per pixel: the run that starts at bit 0 with the word
// on its left when that one ends set, and every run with one pixel of each stretch of the row above inside its own extent widened by a pixel on either
// side (8-connectivity) -- a stretch there is part of one run of the row above, and the runs of that row are joined among themselves by their own
// threads.  mode 2 flatten.
template <class Ids>
__global__ __launch_bounds__(256) void k_ccl_bits(const unsigned long long* __restrict__ bits, int* __restrict__ par, int H, int W, int Ww, int mode) {
    const size_t nw = (size_t)H * Ww, wi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (wi >= nw) return;
    const unsigned layer = Ids::LAYERED ? blockIdx.z : 0u;
    const unsigned long long* b = bits + nw * layer;
    unsigned long long m = b[wi];
    if (!m) return;
    const Ids ids(H, W);
    int* L = par + ids.stride() * layer;
    const int y = (int)(wi / Ww), xw = (int)(wi % Ww), x0 = xw * 64;
    if (mode == 2) {
        while (m) { const int j = __ffsll((long long)m) - 1; m &= m - 1; const int id = ids.at(y, x0 + j); L[id] = uf_find(L, id); }
        return;
    }
    unsigned long long U = 0; bool left = false, nw_px = false, ne_px = false;
    if (mode == 1) {
        left = xw > 0 && (b[wi - 1] >> 63);
        if (y > 0) { U = b[wi - Ww]; nw_px = xw > 0 && (b[wi - Ww - 1] >> 63); ne_px = xw + 1 < Ww && (b[wi - Ww + 1] & 1ULL); }
    }
    unsigned long long starts = m & ~(m << 1);
    while (starts) {
        const int s = __ffsll((long long)starts) - 1; starts &= starts - 1;
        const unsigned long long inv = ~(m >> s);                          // (zero only for the full word)
        const int e = s + (inv ? __ffsll((long long)inv) - 1 : 64) - 1;     // last pixel of the run
        const int id = ids.at(y, x0 + s);
        if (mode == 0) { for (int j = s; j <= e; j++) L[ids.at(y, x0 + j)] = id; continue; }
        if (s == 0 && left) uf_unite(L, id, ids.at(y, x0 - 1));
        const int lo = s > 0 ? s - 1 : 0, hi = e < 63 ? e + 1 : 63;
        const unsigned long long up = U & ((2ULL << hi) - 1ULL) & ~((1ULL << lo) - 1ULL);
        if (s == 0 && nw_px && !(U & 1ULL)) uf_unite(L, id, ids.at(y - 1, x0 - 1));      // (with U's bit 0 set, the stretch that starts there is the same run)
        unsigned long long g = up & ~(up << 1);
        while (g) { const int j = __ffsll((long long)g) - 1; g &= g - 1; uf_unite(L, id, ids.at(y - 1, x0 + j)); }
        if (e == 63 && ne_px && !(U >> 63)) uf_unite(L, id, ids.at(y - 1, x0 + 64));
    }
}

// ---- elements -> bit plane: bit = Pred::on(element).  A wave packs 64 consecutive words: one coalesced read of 64 elements + one ballot per word, then
// one coalesced write of the 64 words; 4 waves x 64 words per block
// LAYERED: blockIdx.z = layer, one bit plane per layer; SRC_LAYERED: one source plane per layer as well (else all layers read the same plane)
struct PackBytes { typedef u8 E; static constexpr bool LAYERED = true, SRC_LAYERED = true; static __device__ bool on(u8 v, unsigned) { return v != 0; } };                 // stages 02 / 04: [K][H][W] bytes
struct PackLabels { typedef u8 E; static constexpr bool LAYERED = true, SRC_LAYERED = false; static __device__ bool on(u8 v, unsigned layer) { return v == layer; } };    // stage 02: one label plane -> K masks
template <class Pred>
__global__ __launch_bounds__(256) void k_pack_bits(const typename Pred::E* __restrict__ src, unsigned long long* __restrict__ bits, int H, int W, int Ww) {
    const size_t nw = (size_t)H * Ww, w0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (w0 >= nw) return;
    const unsigned layer = Pred::LAYERED ? blockIdx.z : 0u;
    const typename Pred::E* s = src + (Pred::SRC_LAYERED ? (size_t)H * W * layer : 0); unsigned long long* b = bits + nw * layer;
    const int lane = threadIdx.x & 63;
    unsigned long long mine = 0;
    for (int j = 0; j < 64; j++) {
        const size_t wi = w0 + j; bool fg = false;
        if (wi < nw) { const int y = (int)(wi / Ww), x = (int)(wi % Ww) * 64 + lane; fg = x < W && Pred::on(s[(size_t)y * W + x], layer); }
        const unsigned long long m = __ballot(fg);
        if (lane == j) mine = m;
    }
    if (w0 + lane < nw) b[w0 + lane] = mine;
}

// ---- ordered compaction of the set bits of `nwords` flattened words (raster order inside a plane, planes in order): a thread owns a word, a block 256
// consecutive words; popcounts (bp_compact_count), block offsets from an exclusive scan of the per-block counts, then every set bit writes what
// Emit makes of it at its position: Emit::word(wi) once per word, Emit::put(word, j, key, lin) per set bit j
struct Emit04 {                  // stage 04: key = layer << 26 | component root (block-raster id), lin = y * W + x inside the layer
    const int* par; size_t nw; int H, W, Ww;
    struct Word { int layer, y, x0, Wb; int64_t pplane; };
    __device__ Word word(size_t wi) const {
        Word w; w.Wb = (W + 1) >> 1; w.pplane = (int64_t)w.Wb * ((H + 1) >> 1) * 4;
        w.layer = (int)(wi / nw); const size_t wl = wi - (size_t)w.layer * nw;
        w.y = (int)(wl / Ww); w.x0 = (int)(wl % Ww) * 64;
        return w;
    }
    __device__ void put(const Word& w, int j, unsigned& key, unsigned& lin) const {
        const int x = w.x0 + j;
        key = ((unsigned)w.layer << 26) | (unsigned)par[w.pplane * w.layer + px_id(w.y, x, w.Wb)];
        lin = (unsigned)((int64_t)w.y * W + x);
    }
};
struct Emit08 {                  // stage 08-B: key = label of the pixel, lin = its index on the padded raster
    const int* L; int Wp, Wwp;
    struct Word { size_t p0; };
    __device__ Word word(size_t wi) const { Word w; w.p0 = (wi / Wwp) * (size_t)Wp + (wi % Wwp) * 64; return w; }
    __device__ void put(const Word& w, int j, unsigned& key, unsigned& lin) const { const size_t p = w.p0 + j; key = (unsigned)L[p]; lin = (unsigned)p; }
};
template <class Emit>
__global__ __launch_bounds__(256) void k_compact_write_bits(const unsigned long long* __restrict__ bits, size_t nwords, const unsigned* __restrict__ block_off, Emit em,
                                                            unsigned* __restrict__ keys, unsigned* __restrict__ lin) {
    const size_t wi = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long m = wi < nwords ? bits[wi] : 0ULL;
    const unsigned at = block_excl_pos256((unsigned)__popcll(m));
    if (!m) return;
    unsigned pos = block_off[blockIdx.x] + at;
    const typename Emit::Word w = em.word(wi);
    while (m) {
        const int j = __ffsll((long long)m) - 1; m &= m - 1;
        em.put(w, j, keys[pos], lin[pos]);
        pos++;
    }
}

// ---- bitplane.hip: launchers (block 256, on stream `st`; the grid is the caller's) and the CCL driver of stages 03 / 04
// [K][H][W] bytes -> K bit planes, bit = byte != 0 (k_pack_bits<PackBytes>); grid = (ceil(H * Ww / 256), 1, K)
void bp_pack_bytes(hipStream_t st, dim3 grid, const u8* src, unsigned long long* bits, int H, int W, int Ww);
// bit planes -> 0 / 255 bytes, any width: a wave takes 64 words in one coalesced read and writes 64 bytes per word; grid.z = planes
void bp_bits_to_bytes(hipStream_t st, dim3 grid, const unsigned long long* bits, u8* dst, int H, int W, int Ww);
// counts[b] = set bits of the words [256 b, 256 b + 256)
void bp_compact_count(hipStream_t st, unsigned nblk, const unsigned long long* bits, size_t nwords, unsigned* counts);
// head[i] = 1 where a new key starts in keys[0, m), for i < n (n = m, or m + 1: head[m] = 0 closes the scan that counts the segments)
void bp_heads(hipStream_t st, const unsigned* keys, int64_t m, int64_t n, unsigned* head);
// comp_start[c] = first element of segment c (head_scan: exclusive scan of head); comp_start[nc] = m
void bp_comp_starts(hipStream_t st, const unsigned* head, const unsigned* head_scan, int64_t m, unsigned* comp_start, unsigned nc);
// components of the K bit planes of the context's image size: par[layer][px_id] = the component's minimum id (init, merge, flatten: three launches)
int orip_ccl_bits(orip_ctx* c, const unsigned long long* bits, int* par, int K);
