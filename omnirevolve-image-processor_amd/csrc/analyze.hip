// csrc/analyze.hip -- analyze_colors.py on gfx950: the colour statistics behind the marker recommendation, from EVERY pixel of the image.
//   colors_table  : the filter of :58-67 and an exact colour table -- one u32 bin per R<<16|G<<8|B (64 MiB, integer atomics, equal keys of a wave merged
//                   before the atomic), compacted in key order into keys u32[D] + counts i64[D], which stay resident
//   colors_hue    : the eleven buckets of _build_hue_histogram (:128-167) per distinct colour, weighted by its count (OpenCV's 8-bit RGB2HSV, recalled)
//   colors_kmeans : weighted k-means over the table -- k-means++ seeding in exact integers, Lloyd with exact int64 sums; all inits side by side (blockIdx.y)
// A uint8 image has at most 2^24 colours, so every step after the first pass runs on the table with the pixel counts as weights, which is the same as
// running on every pixel.  Citations: image_processor/analyze_colors.py of the reference.  The definitions that are ours (seeding, stopping) are in
// include/orip.h and DESIGN 5; tests/analyze_double.py restates them in numpy.
#include "orip_ctx.h"
#include <algorithm>

#define AN_BINS (1u << 24)
#define AN_CB 4096                 // bins per block of the compaction (256 threads x 16)
#define AN_NCB (AN_BINS / AN_CB)   // 4096 blocks
#define AN_SEG 2048                // colours per block of the seeding (256 threads x 8)
#define AN_MAXK 32
#define AN_MAX_INIT 64

struct AnState {                   // small results of the table / hue calls
    unsigned long long nonwhite;   // pixels with a channel below the threshold
    unsigned long long kept;       // pixels of the kept colours
    unsigned D;                    // kept distinct colours
    unsigned pad;
    unsigned long long hue[11];
};
struct AnInit {                    // one k-means init
    double cen[AN_MAXK * 3];
    long long acc[AN_MAXK * 4];    // n, sum R, sum G, sum B of the running iteration
    long long res[AN_MAXK * 4];    // the same of the last finished iteration
    unsigned long long changed;
    unsigned long long x[AN_MAXK]; // the draws of the seeding
    int chosen[AN_MAXK];           // table index of each seed
    int done, iters;
};

__device__ __forceinline__ bool an_nonwhite(unsigned key, int thr) {
    return (int)(key >> 16) < thr || (int)((key >> 8) & 255) < thr || (int)(key & 255) < thr;
}

// 256 threads: exclusive prefix of v over the block, the block total in *total.  s: 256 words of LDS.
__device__ __forceinline__ unsigned long long an_block_scan(unsigned long long v, unsigned long long* s, unsigned long long* total) {
    const int t = threadIdx.x;
    s[t] = v; __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned long long a = t >= d ? s[t - d] : 0ull;
        __syncthreads();
        s[t] += a; __syncthreads();
    }
    const unsigned long long incl = s[t];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

// ---- the hot pass: every pixel into its bin.  Flat artwork puts millions of pixels into one bin, so the lanes of a wave that hold the leader's key are
// merged into one atomic (two rounds), the rest add one each.
__device__ __forceinline__ void an_bin_add(unsigned* __restrict__ table, unsigned key, bool valid) {
    const int lane = __lane_id();
    unsigned long long todo = __ballot(valid);
    for (int r = 0; r < 2 && todo; r++) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned lk = __shfl(key, leader);
        const bool mine = valid && key == lk;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&table[lk], (unsigned)__popcll(same));
        if (mine) valid = false;
        todo &= ~same;
    }
    if (valid) atomicAdd(&table[key], 1u);
}

__global__ __launch_bounds__(256) void k_an_hist(const u8* __restrict__ bgr, int64_t npx, int thr, unsigned* __restrict__ table, AnState* __restrict__ st) {
    const int64_t ngrp = (npx + 3) >> 2, stride = (int64_t)gridDim.x * 256;
    const int64_t rounds = (ngrp + stride - 1) / stride;           // the same for every lane: the ballots below need whole waves
    unsigned nw = 0;
    for (int64_t it = 0; it < rounds; it++) {
        const int64_t q = it * stride + (int64_t)blockIdx.x * 256 + threadIdx.x;
        unsigned k[4] = {0, 0, 0, 0}; int nv = 0;
        if (4 * q + 3 < npx) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(bgr) + 3 * q;
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            // bytes b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            k[0] = ((w0 >> 16) & 255) << 16 | ((w0 >> 8) & 255) << 8 | (w0 & 255);
            k[1] = ((w1 >> 8) & 255) << 16 | (w1 & 255) << 8 | (w0 >> 24);
            k[2] = (w2 & 255) << 16 | (w1 >> 24) << 8 | ((w1 >> 16) & 255);
            k[3] = (w2 >> 24) << 16 | ((w2 >> 16) & 255) << 8 | ((w2 >> 8) & 255);
            nv = 4;
        } else {
            for (int64_t i = 4 * q; i < npx; i++, nv++) k[nv] = (unsigned)bgr[3 * i + 2] << 16 | (unsigned)bgr[3 * i + 1] << 8 | bgr[3 * i];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            an_bin_add(table, k[j], j < nv);
            if (j < nv && an_nonwhite(k[j], thr)) nw++;
        }
    }
    for (int d = 32; d; d >>= 1) nw += __shfl_down(nw, d);
    if (__lane_id() == 0 && nw) atomicAdd(&st->nonwhite, (unsigned long long)nw);
}

__device__ __forceinline__ bool an_keep_all(const AnState* st, int ignore_white, long long min_kept) {
    return !ignore_white || (long long)st->nonwhite < min_kept;       // :63-67
}

// kept bins per block of AN_CB bins, and the pixels in them
__global__ __launch_bounds__(256) void k_an_count(const unsigned* __restrict__ table, int thr, int ignore_white, long long min_kept, AnState* __restrict__ st,
                                                   unsigned* __restrict__ blockcnt) {
    __shared__ unsigned long long s[256];
    const bool all = an_keep_all(st, ignore_white, min_kept);
    const unsigned base = blockIdx.x * AN_CB + threadIdx.x * 16;
    unsigned n = 0; unsigned long long px = 0;
    for (int j = 0; j < 16; j++) {
        const unsigned cnt = table[base + j];
        if (cnt && (all || an_nonwhite(base + j, thr))) { n++; px += cnt; }
    }
    unsigned long long tot;
    an_block_scan(n, s, &tot);
    const unsigned nblk = (unsigned)tot;
    an_block_scan(px, s, &tot);
    if (threadIdx.x == 0) { blockcnt[blockIdx.x] = nblk; if (tot) atomicAdd(&st->kept, tot); }
}
// exclusive prefix of the AN_NCB block counts (one block), D
__global__ __launch_bounds__(256) void k_an_offsets(const unsigned* __restrict__ blockcnt, unsigned* __restrict__ blockoff, AnState* __restrict__ st) {
    __shared__ unsigned long long s[256];
    const int per = AN_NCB / 256;
    unsigned long long loc = 0;
    for (int j = 0; j < per; j++) loc += blockcnt[threadIdx.x * per + j];
    unsigned long long tot;
    unsigned long long pre = an_block_scan(loc, s, &tot);
    for (int j = 0; j < per; j++) { blockoff[threadIdx.x * per + j] = (unsigned)pre; pre += blockcnt[threadIdx.x * per + j]; }
    if (threadIdx.x == 0) st->D = (unsigned)tot;
}
__global__ __launch_bounds__(256) void k_an_emit(const unsigned* __restrict__ table, int thr, int ignore_white, long long min_kept, const AnState* __restrict__ st,
                                                  const unsigned* __restrict__ blockoff, unsigned D, unsigned* __restrict__ keys, long long* __restrict__ counts) {
    __shared__ unsigned long long s[256];
    const bool all = an_keep_all(st, ignore_white, min_kept);
    const unsigned base = blockIdx.x * AN_CB + threadIdx.x * 16;
    unsigned cnt[16]; unsigned n = 0;
    for (int j = 0; j < 16; j++) {
        cnt[j] = table[base + j];
        if (!(cnt[j] && (all || an_nonwhite(base + j, thr)))) cnt[j] = 0;
        n += cnt[j] != 0;
    }
    unsigned long long tot;
    unsigned o = blockoff[blockIdx.x] + (unsigned)an_block_scan(n, s, &tot);
    for (int j = 0; j < 16; j++)
        if (cnt[j] && o < D) { keys[o] = base + j; counts[o] = cnt[j]; o++; }
}

// ---- hue buckets (:128-167).  cv2.cvtColor(COLOR_RGB2HSV) on uint8 as OpenCV's integer path computes it (recalled, not pinned: DESIGN 5).
__device__ __forceinline__ int an_hue_bucket(int r, int g, int b, const int* sdiv, const int* hdiv) {
    const int v = max(r, max(g, b)), diff = v - min(r, min(g, b));
    const int s = (diff * sdiv[v] + (1 << 11)) >> 12;
    int h = v == r ? g - b : v == g ? b - r + 2 * diff : r - g + 4 * diff;
    h = (h * hdiv[diff] + (1 << 11)) >> 12;
    if (h < 0) h += 180;
    if (v < 50) return 10;                          // black
    if (s < 30) return 9;                           // gray
    const int hf = 2 * h;
    if (hf < 15 || hf >= 345) return 0;             // red
    if (hf < 25) return s > 150 && v < 150 ? 8 : 1; // brown / orange
    if (hf < 45) return 1;                          // orange
    if (hf < 75) return 2;                          // yellow
    if (hf < 150) return 3;                         // green
    if (hf < 200) return 4;                         // cyan
    if (hf < 270) return 5;                         // blue
    if (hf < 330) return s < 100 ? 7 : 6;           // pink / purple
    return 7;                                       // pink
}
__global__ __launch_bounds__(256) void k_an_hue(const unsigned* __restrict__ keys, const long long* __restrict__ counts, unsigned D, AnState* __restrict__ st) {
    __shared__ int sdiv[256], hdiv[256];
    __shared__ unsigned long long hb[11];
    const int t = threadIdx.x;                      // round(x / t) of positive integers: (2 x + t) / (2 t); no ties occur for these x
    sdiv[t] = t ? (2 * (255 << 12) + t) / (2 * t) : 0;
    hdiv[t] = t ? (2 * (180 << 12) + 6 * t) / (12 * t) : 0;
    if (t < 11) hb[t] = 0;
    __syncthreads();
    for (unsigned i = blockIdx.x * 256 + t; i < D; i += gridDim.x * 256) {
        const unsigned k = keys[i];
        atomicAdd(&hb[an_hue_bucket(k >> 16, (k >> 8) & 255, k & 255, sdiv, hdiv)], (unsigned long long)counts[i]);
    }
    __syncthreads();
    if (t < 11 && hb[t]) atomicAdd(&st->hue[t], hb[t]);
}

// ---- k-means++ seeding, exact integers.  Step s of every init: the weight of colour i is count_i (s = 0) or count_i * mind2_i.
__device__ __forceinline__ int an_d2(unsigned a, unsigned b) {
    const int dr = (int)(a >> 16) - (int)(b >> 16), dg = (int)((a >> 8) & 255) - (int)((b >> 8) & 255), db = (int)(a & 255) - (int)(b & 255);
    return dr * dr + dg * dg + db * db;
}
// folds the centre chosen at step - 1 into mind2 and leaves the weight sum of each AN_SEG colours
__global__ __launch_bounds__(256) void k_an_seed_weights(const unsigned* __restrict__ keys, const long long* __restrict__ counts, unsigned D, int step, const AnInit* __restrict__ inits,
                                                          int* __restrict__ mind2, unsigned long long* __restrict__ segsum, unsigned nseg) {
    __shared__ unsigned long long s[256];
    const int init = blockIdx.y;
    int* md = mind2 + (size_t)init * D;
    const unsigned ck = step ? keys[inits[init].chosen[step - 1]] : 0u;
    const unsigned base = blockIdx.x * AN_SEG + threadIdx.x * 8;
    unsigned long long w = 0;
    for (int j = 0; j < 8; j++) {
        const unsigned i = base + j;
        if (i >= D) break;
        if (step == 0) { w += (unsigned long long)counts[i]; continue; }
        int m = an_d2(keys[i], ck);
        if (step > 1) m = min(m, md[i]);
        md[i] = m;
        w += (unsigned long long)counts[i] * (unsigned long long)m;
    }
    unsigned long long tot;
    an_block_scan(w, s, &tot);
    if (threadIdx.x == 0) segsum[(size_t)init * nseg + blockIdx.x] = tot;
}
// t = x mod total; the first colour in key order whose inclusive prefix sum exceeds t.  One block per init.
__global__ __launch_bounds__(256) void k_an_seed_pick(const long long* __restrict__ counts, unsigned D, int step, AnInit* __restrict__ inits, const int* __restrict__ mind2,
                                                      const unsigned long long* __restrict__ segsum, unsigned nseg) {
    __shared__ unsigned long long s[256];
    __shared__ unsigned long long sh_rest; __shared__ unsigned sh_seg; __shared__ int sh_pick;
    const int init = blockIdx.x, t = threadIdx.x;
    const int* md = mind2 + (size_t)init * D;
    const unsigned long long* ss = segsum + (size_t)init * nseg;
    const unsigned per = (nseg + 255) / 256;
    unsigned long long loc = 0;
    for (unsigned j = 0; j < per; j++) { const unsigned b = t * per + j; if (b < nseg) loc += ss[b]; }
    unsigned long long total;
    unsigned long long pre = an_block_scan(loc, s, &total);
    if (t == 0) { sh_pick = -1; sh_seg = 0; sh_rest = 0; }
    __syncthreads();
    if (total == 0) { if (t == 0) inits[init].chosen[step] = -1; return; }          // cannot happen with D >= K distinct colours; the host reports it
    const unsigned long long target = inits[init].x[step] % total;
    if (pre <= target && target < pre + loc) {
        for (unsigned j = 0; j < per; j++) {
            const unsigned b = t * per + j;
            if (b >= nseg) break;
            if (target < pre + ss[b]) { sh_seg = b; sh_rest = target - pre; break; }
            pre += ss[b];
        }
    }
    __syncthreads();
    const unsigned base = sh_seg * AN_SEG + t * 8;
    const unsigned long long rest = sh_rest;
    unsigned long long w[8]; loc = 0;
    for (int j = 0; j < 8; j++) {
        const unsigned i = base + j;
        w[j] = i < D ? (unsigned long long)counts[i] * (step ? (unsigned long long)md[i] : 1ull) : 0ull;
        loc += w[j];
    }
    pre = an_block_scan(loc, s, &total);
    if (pre <= rest && rest < pre + loc) {
        for (int j = 0; j < 8; j++) {
            if (rest < pre + w[j]) { sh_pick = (int)(base + j); break; }
            pre += w[j];
        }
    }
    __syncthreads();
    if (t == 0) inits[init].chosen[step] = sh_pick;
}
__global__ void k_an_seed_centres(const unsigned* __restrict__ keys, int K, AnInit* __restrict__ inits) {
    AnInit& I = inits[blockIdx.x];
    const int k = threadIdx.x;
    if (k < K) {
        const unsigned key = keys[max(I.chosen[k], 0)];
        I.cen[3 * k] = (double)(key >> 16); I.cen[3 * k + 1] = (double)((key >> 8) & 255); I.cen[3 * k + 2] = (double)(key & 255);
    }
    for (int j = k; j < AN_MAXK * 4; j += blockDim.x) I.acc[j] = 0;
    if (k == 0) { I.changed = 0; I.done = 0; I.iters = 0; }
}

// ---- Lloyd.  One iteration = k_an_assign (nearest centre in double, ties to the lowest index; n / sums of count * channel per cluster: per wave in LDS, one
// atomic per block and value) + k_an_update (centre = sum / n, an empty cluster keeps its centre; done when no colour changed cluster).
__global__ __launch_bounds__(256) void k_an_assign(const unsigned* __restrict__ keys, const long long* __restrict__ counts, unsigned D, int K, int first,
                                                    AnInit* __restrict__ inits, u8* __restrict__ labels) {
    __shared__ double cen[AN_MAXK * 3];
    __shared__ unsigned long long acc[4][AN_MAXK * 4];
    __shared__ unsigned chg[4];
    AnInit& I = inits[blockIdx.y];
    if (I.done) return;
    u8* lab = labels + (size_t)blockIdx.y * D;
    const int t = threadIdx.x, wv = t >> 6;
    if (t < 3 * K) cen[t] = I.cen[t];
    for (int j = t; j < 4 * AN_MAXK * 4; j += 256) (&acc[0][0])[j] = 0;
    if (t < 4) chg[t] = 0;
    __syncthreads();
    unsigned changed = 0;
    for (unsigned i = blockIdx.x * 256 + t; i < D; i += gridDim.x * 256) {
        const unsigned key = keys[i];
        const double r = (double)(key >> 16), g = (double)((key >> 8) & 255), b = (double)(key & 255);
        double best = 0; int kb = 0;
        for (int k = 0; k < K; k++) {
            const double dr = r - cen[3 * k], dg = g - cen[3 * k + 1], db = b - cen[3 * k + 2];
            const double d = (dr * dr + dg * dg) + db * db;
            if (k == 0 || d < best) { best = d; kb = k; }
        }
        if (first || lab[i] != kb) changed++;
        lab[i] = (u8)kb;
        const unsigned long long n = (unsigned long long)counts[i];
        atomicAdd(&acc[wv][4 * kb], n); atomicAdd(&acc[wv][4 * kb + 1], n * (key >> 16));
        atomicAdd(&acc[wv][4 * kb + 2], n * ((key >> 8) & 255)); atomicAdd(&acc[wv][4 * kb + 3], n * (key & 255));
    }
    if (changed) atomicAdd(&chg[wv], changed);
    __syncthreads();
    if (t < 4 * K) {
        const unsigned long long v = acc[0][t] + acc[1][t] + acc[2][t] + acc[3][t];
        if (v) atomicAdd((unsigned long long*)&I.acc[t], v);
    }
    if (t == 0) { const unsigned c = chg[0] + chg[1] + chg[2] + chg[3]; if (c) atomicAdd(&I.changed, (unsigned long long)c); }
}
__global__ void k_an_update(int K, AnInit* __restrict__ inits) {
    AnInit& I = inits[blockIdx.x];
    if (I.done) return;
    const int k = threadIdx.x;
    const bool still = I.changed == 0;
    __syncthreads();
    if (k < K) {
        const long long n = I.acc[4 * k];
        for (int j = 0; j < 4; j++) { I.res[4 * k + j] = I.acc[4 * k + j]; }
        if (n > 0) for (int j = 0; j < 3; j++) I.cen[3 * k + j] = (double)I.acc[4 * k + 1 + j] / (double)n;
        for (int j = 0; j < 4; j++) I.acc[4 * k + j] = 0;
    }
    __syncthreads();
    if (k == 0) { I.iters++; I.changed = 0; if (still) I.done = 1; }
}

// ------------------------------------------------------------------------------------------------ host entry points
static int an_scratch(orip_ctx* c, AnState*& st, unsigned*& blockcnt, unsigned*& blockoff) {
    Carve L; L.take(st, 1); L.take(blockcnt, AN_NCB); L.take(blockoff, AN_NCB);
    HIPC(c, L.commit(c->an_tmp, 0));
    return 0;
}

extern "C" int orip_colors_table(orip_ctx* c, int ignore_white, int white_threshold, int64_t min_kept, int64_t* n_colors, int64_t* kept_pixels, int* used_all) {
    orip_enter(c);
    c->an_ready = false;
    if (!c->image.p) ORIP_FAIL(c, "no image set");
    if (!n_colors || !kept_pixels || !used_all) ORIP_FAIL(c, "NULL result pointer");
    const int64_t npx = (int64_t)c->H * c->W;
    hipStream_t s = LN(c).stream;
    AnState* st; unsigned *blockcnt, *blockoff;
    ORIP_TRY(an_scratch(c, st, blockcnt, blockoff));
    HIPC(c, c->an_table.ensure((size_t)AN_BINS * 4));
    HIPC(c, hipMemsetAsync(c->an_table.p, 0, (size_t)AN_BINS * 4, s));
    HIPC(c, hipMemsetAsync(st, 0, sizeof(AnState), s));
    const int thr = white_threshold; const int iw = ignore_white ? 1 : 0;
    {
        ProfScope ps(c, "k_an_hist");
        hipLaunchKernelGGL(k_an_hist, dim3((unsigned)std::min<int64_t>(4096, cdiv(cdiv(npx, 4), 256))), dim3(256), 0, s, c->image.as<u8>(), npx, thr, c->an_table.as<unsigned>(), st);
    }
    {
        ProfScope ps(c, "k_an_count");
        hipLaunchKernelGGL(k_an_count, dim3(AN_NCB), dim3(256), 0, s, c->an_table.as<unsigned>(), thr, iw, (long long)min_kept, st, blockcnt);
    }
    hipLaunchKernelGGL(k_an_offsets, dim3(1), dim3(256), 0, s, blockcnt, blockoff, st);
    HIPC(c, hipGetLastError());
    AnState h;
    HIPC(c, hipMemcpyAsync(&h, st, sizeof(AnState), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    const unsigned D = h.D;
    if ((int64_t)D > npx || D > AN_BINS) ORIP_FAIL(c, "colour table: %u colours from %lld pixels", D, (long long)npx);
    HIPC(c, c->an_keys.ensure((size_t)D * 4 + 16));
    HIPC(c, c->an_counts.ensure((size_t)D * 8 + 16));
    {
        ProfScope ps(c, "k_an_emit");
        hipLaunchKernelGGL(k_an_emit, dim3(AN_NCB), dim3(256), 0, s, c->an_table.as<unsigned>(), thr, iw, (long long)min_kept, st, blockoff, D, c->an_keys.as<unsigned>(),
                           c->an_counts.as<long long>());
    }
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    c->an_D = D; c->an_kept = (int64_t)h.kept; c->an_ready = true;
    *n_colors = D; *kept_pixels = (int64_t)h.kept;
    *used_all = (iw && (int64_t)h.nonwhite < min_kept) ? 1 : 0;
    return 0;
}

extern "C" int orip_colors_fetch(orip_ctx* c, uint32_t* keys_out, int64_t* counts_out, int64_t* kept_pixels) {
    orip_enter(c);
    if (!c->an_ready) ORIP_FAIL(c, "no colour table: call orip_colors_table after orip_set_image");
    hipStream_t s = LN(c).stream;
    if (keys_out && c->an_D) HIPC(c, hipMemcpyAsync(keys_out, c->an_keys.p, (size_t)c->an_D * 4, hipMemcpyDeviceToHost, s));
    if (counts_out && c->an_D) HIPC(c, hipMemcpyAsync(counts_out, c->an_counts.p, (size_t)c->an_D * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (kept_pixels) *kept_pixels = c->an_kept;
    return 0;
}

extern "C" int orip_colors_hue(orip_ctx* c, int64_t* counts_out) {
    orip_enter(c);
    if (!c->an_ready) ORIP_FAIL(c, "no colour table: call orip_colors_table after orip_set_image");
    if (!counts_out) ORIP_FAIL(c, "NULL result pointer");
    hipStream_t s = LN(c).stream;
    AnState* st; unsigned *blockcnt, *blockoff;
    ORIP_TRY(an_scratch(c, st, blockcnt, blockoff));
    HIPC(c, hipMemsetAsync(st->hue, 0, sizeof(st->hue), s));
    const unsigned D = (unsigned)c->an_D;
    if (D) {
        ProfScope ps(c, "k_an_hue");
        hipLaunchKernelGGL(k_an_hue, dim3((unsigned)std::min<int64_t>(1024, cdiv(D, 256))), dim3(256), 0, s, c->an_keys.as<unsigned>(), c->an_counts.as<long long>(), D, st);
    }
    HIPC(c, hipGetLastError());
    unsigned long long h[11];
    HIPC(c, hipMemcpyAsync(h, st->hue, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    for (int i = 0; i < 11; i++) counts_out[i] = (int64_t)h[i];
    return 0;
}

static inline uint64_t an_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

extern "C" int orip_colors_kmeans(orip_ctx* c, int K, int n_init, int max_iter, uint64_t seed, double* centers_out, int64_t* n_out, int64_t* sums_out, int32_t* iters_out) {
    orip_enter(c);
    if (!c->an_ready) ORIP_FAIL(c, "no colour table: call orip_colors_table after orip_set_image");
    if (K < 2 || K > AN_MAXK) ORIP_FAIL(c, "K=%d out of range 2..%d", K, AN_MAXK);
    if (n_init < 1 || n_init > AN_MAX_INIT) ORIP_FAIL(c, "n_init=%d out of range 1..%d", n_init, AN_MAX_INIT);
    if (max_iter < 1) ORIP_FAIL(c, "max_iter=%d must be at least 1", max_iter);
    if (!centers_out || !n_out || !sums_out) ORIP_FAIL(c, "NULL result pointer");
    const unsigned D = (unsigned)c->an_D;
    if ((int64_t)D < K) ORIP_FAIL(c, "%u distinct colours are fewer than K=%d clusters", D, K);
    hipStream_t s = LN(c).stream;
    const unsigned nseg = (unsigned)cdiv(D, AN_SEG);
    AnInit* inits; int* mind2; unsigned long long* segsum; u8* labels;
    {
        Carve L; L.take(inits, (size_t)n_init); L.take(segsum, (size_t)n_init * nseg); L.take(mind2, (size_t)n_init * D); L.take(labels, (size_t)n_init * D);
        HIPC(c, L.commit(c->an_km, 0));
    }
    std::vector<AnInit> h((size_t)n_init);
    memset(h.data(), 0, sizeof(AnInit) * n_init);
    for (int i = 0; i < n_init; i++)
        for (int k = 0; k < K; k++) h[i].x[k] = an_splitmix64(seed ^ (((uint64_t)i << 32) + (uint64_t)k));
    HIPC(c, hipMemcpyAsync(inits, h.data(), sizeof(AnInit) * n_init, hipMemcpyHostToDevice, s));
    const unsigned* keys = c->an_keys.as<unsigned>(); const long long* counts = c->an_counts.as<long long>();
    {
        ProfScope ps(c, "an_seed");
        for (int step = 0; step < K; step++) {
            hipLaunchKernelGGL(k_an_seed_weights, dim3(nseg, n_init), dim3(256), 0, s, keys, counts, D, step, inits, mind2, segsum, nseg);
            hipLaunchKernelGGL(k_an_seed_pick, dim3(n_init), dim3(256), 0, s, counts, D, step, inits, mind2, segsum, nseg);
        }
        hipLaunchKernelGGL(k_an_seed_centres, dim3(n_init), dim3(64), 0, s, keys, K, inits);
    }
    HIPC(c, hipGetLastError());
    const unsigned nb = (unsigned)std::min<int64_t>(1024, cdiv(D, 256));
    const int LOOK = 8;                 // the host looks at the done flags every LOOK iterations
    {
        ProfScope ps(c, "an_lloyd");
        for (int it = 0; it < max_iter;) {
            const int upto = std::min(max_iter, it + LOOK);
            for (; it < upto; it++) {
                hipLaunchKernelGGL(k_an_assign, dim3(nb, n_init), dim3(256), 0, s, keys, counts, D, K, it == 0 ? 1 : 0, inits, labels);
                hipLaunchKernelGGL(k_an_update, dim3(n_init), dim3(64), 0, s, K, inits);
            }
            HIPC(c, hipGetLastError());
            HIPC(c, hipMemcpyAsync(h.data(), inits, sizeof(AnInit) * n_init, hipMemcpyDeviceToHost, s));
            HIPC(c, hipStreamSynchronize(s));
            bool all_done = true;
            for (int i = 0; i < n_init; i++) all_done = all_done && h[i].done;
            if (all_done) break;
        }
    }
    for (int i = 0; i < n_init; i++) {
        for (int k = 0; k < K; k++) {
            if (h[i].chosen[k] < 0) ORIP_FAIL(c, "seeding of init %d found no colour at step %d", i, k);
            n_out[(size_t)i * K + k] = h[i].res[4 * k];
            for (int j = 0; j < 3; j++) { sums_out[((size_t)i * K + k) * 3 + j] = h[i].res[4 * k + 1 + j]; centers_out[((size_t)i * K + k) * 3 + j] = h[i].cen[3 * k + j]; }
        }
        if (iters_out) iters_out[i] = h[i].iters;
    }
    return 0;
}
