// csrc/raster02.hip -- stage 02 (02_color_extract.py) on gfx950:
//   lab_assign   : BGR u8 -> Lab u8 (cv2.cvtColor, 02:35) -> nearest centre (02:53-55) -> dark->light label (02:120-127)
//   lab_gather   : Lab of the k-means subsample (02:39-44); rgb_gather: its R, G, B bytes for process_colors.py.  The fit itself is kmeans02.hip
//   morph_pass   : erode / dilate with an arbitrary <=7x7 structuring element (02:151-154, 03:25-30), on bit planes when the input is binary
// All float arithmetic mirrors numpy / OpenCV evaluation order: compiled with -ffp-contract=off and written
// with explicit __fmul_rn/__fadd_rn where the order matters.
#include "bitplane.h"
#include <cmath>
#include <algorithm>

// ------------------------------------------------------------------------------------------------
// Lab tables, built on the host once per context.
// ------------------------------------------------------------------------------------------------
struct LabTabs { uint16_t gamma[256]; uint16_t cbrt[3072]; int32_t coef[9]; };

int orip_raster02_lab_tables(orip_ctx* c) {
    if (c->tabs_ready) return 0;
    static LabTabs t;
    for (int i = 0; i < 256; i++) {
        double x = i / 255.0;
        double g = x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4);
        long v = std::lrint(255.0 * 8.0 * g);
        t.gamma[i] = (uint16_t)std::min<long>(std::max<long>(v, 0), 65535);
    }
    for (int i = 0; i < 3072; i++) {
        double x = i / (255.0 * 8.0);
        double y = x < 0.008856 ? x * 7.787 + 0.13793103448275862 : std::cbrt(x);
        long v = std::lrint(32768.0 * y);
        t.cbrt[i] = (uint16_t)std::min<long>(std::max<long>(v, 0), 65535);
    }
    const double M[9] = {0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227};
    const double D65[3] = {0.950456, 1.0, 1.088754};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) t.coef[i * 3 + j] = (int32_t)std::lrint(4096.0 * M[i * 3 + j] / D65[i]);
    HIPC(c, c->lab_tabs.ensure(sizeof(LabTabs)));
    HIPC(c, hipMemcpyAsync(c->lab_tabs.p, &t, sizeof(LabTabs), hipMemcpyHostToDevice, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    c->tabs_ready = true;
    return 0;
}

struct LabLds { uint16_t gamma[256]; uint16_t cbrt[3072]; };

__device__ __forceinline__ void lab_lds_load(LabLds* s, const LabTabs* t) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s->gamma[i] = t->gamma[i];
    for (int i = threadIdx.x; i < 3072; i += blockDim.x) s->cbrt[i] = t->cbrt[i];
    __syncthreads();
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

__device__ __forceinline__ void bgr2lab_px(const LabLds* s, const int32_t* C, int b8, int g8, int r8, int& L, int& a, int& b) {
    int B = s->gamma[b8], G = s->gamma[g8], R = s->gamma[r8];
    int fX = s->cbrt[descale(R * C[0] + G * C[1] + B * C[2], 12)];
    int fY = s->cbrt[descale(R * C[3] + G * C[4] + B * C[5], 12)];
    int fZ = s->cbrt[descale(R * C[6] + G * C[7] + B * C[8], 12)];
    const int Lscale = (116 * 255 + 50) / 100;
    const int Lshift = -((16 * 255 * (1 << 15) + 50) / 100);
    L = min(max(descale(Lscale * fY + Lshift, 15), 0), 255);
    a = min(max(descale(500 * (fX - fY) + 128 * (1 << 15), 15), 0), 255);
    b = min(max(descale(200 * (fY - fZ) + 128 * (1 << 15), 15), 0), 255);
}

struct Centers { float c[ORIP_MAX_LAYERS * 3]; uint8_t lut[ORIP_MAX_LAYERS]; int K; };

__device__ __forceinline__ int nearest_center(const Centers& cs, int L, int a, int b) {
    float p0 = (float)L, p1 = (float)a, p2 = (float)b;
    float best = 0.f; int kb = 0;
    for (int k = 0; k < cs.K; k++) {
        float d0 = __fsub_rn(p0, cs.c[3 * k]), d1 = __fsub_rn(p1, cs.c[3 * k + 1]), d2 = __fsub_rn(p2, cs.c[3 * k + 2]);
        float s = __fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2));
        if (k == 0 || s < best) { best = s; kb = k; }
    }
    return cs.lut[kb];
}

// 4 pixels per thread: 12 B in (3 dwords), 4 B out (1 dword).  Algorithmic traffic 3+1 B/px.
__global__ __launch_bounds__(256) void k_lab_assign(const u8* __restrict__ bgr, u8* __restrict__ labels, int64_t npx,
                                                     const LabTabs* __restrict__ tabs, Centers cs) {
    __shared__ LabLds s;
    __shared__ int32_t C[9];
    if (threadIdx.x < 9) C[threadIdx.x] = tabs->coef[threadIdx.x];
    lab_lds_load(&s, tabs);
    int64_t ngrp = npx >> 2;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngrp; g += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(bgr + g * 12);
        uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
        u8 px[12] = {(u8)w0, (u8)(w0 >> 8), (u8)(w0 >> 16), (u8)(w0 >> 24), (u8)w1, (u8)(w1 >> 8), (u8)(w1 >> 16), (u8)(w1 >> 24),
                     (u8)w2, (u8)(w2 >> 8), (u8)(w2 >> 16), (u8)(w2 >> 24)};
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int L, a, b; bgr2lab_px(&s, C, px[3 * j], px[3 * j + 1], px[3 * j + 2], L, a, b);
            out |= (uint32_t)nearest_center(cs, L, a, b) << (8 * j);
        }
        reinterpret_cast<uint32_t*>(labels)[g] = out;
    }
    // tail (npx % 4)
    if (blockIdx.x == 0 && threadIdx.x < (npx & 3)) {
        int64_t i = (npx & ~(int64_t)3) + threadIdx.x;
        int L, a, b; bgr2lab_px(&s, C, bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], L, a, b);
        labels[i] = (u8)nearest_center(cs, L, a, b);
    }
}

// Lab of selected pixels (idx == nullptr: pixel i itself)
__global__ __launch_bounds__(256) void k_lab_gather(const u8* __restrict__ bgr, const int64_t* __restrict__ idx, int64_t n,
                                                     u8* __restrict__ lab, const LabTabs* __restrict__ tabs) {
    __shared__ LabLds s;
    __shared__ int32_t C[9];
    if (threadIdx.x < 9) C[threadIdx.x] = tabs->coef[threadIdx.x];
    lab_lds_load(&s, tabs);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t p = idx ? idx[i] : i;
        int L, a, b; bgr2lab_px(&s, C, bgr[3 * p], bgr[3 * p + 1], bgr[3 * p + 2], L, a, b);
        lab[3 * i] = (u8)L; lab[3 * i + 1] = (u8)a; lab[3 * i + 2] = (u8)b;
    }
}

// process_colors.py kmeans_palette (:31-46) clusters RGB bytes, not Lab: the sampled pixels in R, G, B order
__global__ __launch_bounds__(256) void k_rgb_gather(const u8* __restrict__ bgr, const int64_t* __restrict__ idx, int64_t n, u8* __restrict__ rgb) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = idx ? idx[i] : i;
        rgb[3 * i] = bgr[3 * p + 2]; rgb[3 * i + 1] = bgr[3 * p + 1]; rgb[3 * i + 2] = bgr[3 * p];
    }
}
void orip_raster02_gather(orip_ctx* c, bool rgb, const int64_t* d_idx, int64_t n, uint8_t* dst) {      // (declared in orip_ctx.h; the k-means fit's samples)
    const dim3 grid(std::min<int64_t>(2048, cdiv(n, 256))), block(256);
    if (rgb) hipLaunchKernelGGL(k_rgb_gather, grid, block, 0, LN(c).stream, c->image.as<u8>(), d_idx, n, dst);
    else hipLaunchKernelGGL(k_lab_gather, grid, block, 0, LN(c).stream, c->image.as<u8>(), d_idx, n, dst, c->lab_tabs.as<LabTabs>());
}
// process_colors.py assign_labels (:69-77): nearest palette colour in RGB with the reference's int16 arithmetic -- the squares of differences
// above 181 wrap to negative values before they are summed (in int64), and np.argmin takes the first minimum.  Four pixels per thread (12 bytes in,
// 4 bytes out), the palette in LDS.
__global__ __launch_bounds__(256) void k_assign_palette(const u8* __restrict__ bgr, int64_t npx, const u8* __restrict__ pal_rgb, int K, u8* __restrict__ labels) {
    __shared__ int pr[ORIP_MAX_LAYERS], pg[ORIP_MAX_LAYERS], pb[ORIP_MAX_LAYERS];
    if (threadIdx.x < K) { pr[threadIdx.x] = pal_rgb[3 * threadIdx.x]; pg[threadIdx.x] = pal_rgb[3 * threadIdx.x + 1]; pb[threadIdx.x] = pal_rgb[3 * threadIdx.x + 2]; }
    __syncthreads();
    auto sq16 = [](int d) { return (int)(int16_t)(uint16_t)(d * d); };
    auto nearest = [&](int b, int g, int r) {
        int best = 0x7fffffff, bi = 0;
        for (int k = 0; k < K; k++) { const int d = sq16(r - pr[k]) + sq16(g - pg[k]) + sq16(b - pb[k]); if (d < best) { best = d; bi = k; } }
        return bi;
    };
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;                  // group of four pixels
    if (4 * q + 3 < npx) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(bgr) + 3 * q;    // hipMalloc'd, 12-byte groups: dword aligned
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        const unsigned l0 = nearest(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255);
        const unsigned l1 = nearest(w0 >> 24, w1 & 255, (w1 >> 8) & 255);
        const unsigned l2 = nearest((w1 >> 16) & 255, w1 >> 24, w2 & 255);
        const unsigned l3 = nearest((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24);
        reinterpret_cast<uint32_t*>(labels)[q] = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
    } else {
        for (int64_t i = 4 * q; i < npx; i++) labels[i] = (u8)nearest(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2]);
    }
}

__global__ void k_count_labels(const u8* __restrict__ labels, int64_t n, unsigned long long* counts) {
    __shared__ unsigned int h[ORIP_MAX_LAYERS];
    if (threadIdx.x < ORIP_MAX_LAYERS) h[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&h[labels[i] & 15], 1u);
    __syncthreads();
    if (threadIdx.x < ORIP_MAX_LAYERS && h[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------
// Morphology: one erode/dilate pass with a k x k structuring element given as a bit mask (bit i*k+j).
// Out-of-image neighbours never win (cv2 default border).  If labels_mode, the source is the label
// map and the pixel value is (label == layer) ? 255 : 0  -- fuses `mask=(labels==k)*255` (02:150).
// grid.z = layer.
// ------------------------------------------------------------------------------------------------
#define MT_X 64
#define MT_Y 16
__global__ __launch_bounds__(256) void k_morph_pass(const u8* __restrict__ src, u8* __restrict__ dst, int H, int W, int k,
                                                     unsigned long long se, int dilate, int labels_mode) {
    __shared__ u8 tile[MT_Y + 6][MT_X + 8];
    const int r = k >> 1;
    const int layer = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const u8* s = labels_mode ? src : src + plane * layer;
    u8* d = dst + plane * layer;
    const int x0 = blockIdx.x * MT_X, y0 = blockIdx.y * MT_Y;
    const u8 neutral = dilate ? 0 : 255;
    for (int i = threadIdx.x; i < (MT_Y + 2 * r) * (MT_X + 2 * r); i += blockDim.x) {
        int ty = i / (MT_X + 2 * r), tx = i % (MT_X + 2 * r);
        int y = y0 + ty - r, x = x0 + tx - r;
        u8 v = neutral;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            u8 raw = s[(size_t)y * W + x];
            v = labels_mode ? (raw == layer ? 255 : 0) : raw;
        }
        tile[ty][tx] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MT_Y * MT_X; i += blockDim.x) {
        int ty = i / MT_X, tx = i % MT_X;
        int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        int v = neutral;
        for (int a = 0; a < k; a++)
            for (int b = 0; b < k; b++)
                if ((se >> (a * k + b)) & 1ULL) { int t = tile[ty + a][tx + b]; v = dilate ? max(v, t) : min(v, t); }
        d[(size_t)y * W + x] = (u8)v;
    }
}

static unsigned long long make_se_bits(int shape, int k) {
    unsigned long long se = 0;
    if (shape == 0) { for (int i = 0; i < k * k; i++) se |= 1ULL << i; return se; }
    int r = k / 2, c = k / 2; double inv_r2 = r ? 1.0 / ((double)r * r) : 0;
    for (int i = 0; i < k; i++) {
        int dy = i - r, j1 = 0, j2 = 0;
        if (std::abs(dy) <= r) { int dx = (int)std::lrint(c * std::sqrt((r * r - dy * dy) * inv_r2)); j1 = std::max(c - dx, 0); j2 = std::min(c + dx + 1, k); }
        for (int j = j1; j < j2; j++) se |= 1ULL << (i * k + j);
    }
    return se;
}

// ------------------------------------------------------------------------------------------------
// Binary fast path of the same chain: a 0/255 mask packs to one bit per pixel (64 pixels per word, 2 MB per 4096^2 layer, so the
// whole chain of passes runs out of L2), dilation = OR and erosion = AND of shifted rows.  Out-of-image pixels are neutral
// (erode: ones, dilate: zeros), exactly as in k_morph_pass.  Rows that are no multiple of 64 wide pack and unpack through the shared kernels of
// bitplane.h (k_pack_bits<PackLabels>, bp_pack_bytes, bp_bits_to_bytes); multiples of 64 through the one-pass kernels below.
// ------------------------------------------------------------------------------------------------
// labels -> K bit planes in ONE pass over the label plane (rows that are multiples of 64 wide): a thread takes the 64 labels of a word as four 16-byte
// loads and emits the word of every layer -- per layer and 4 labels an exact "byte equals l" test on the 32-bit word (zero-byte detection of w ^ l l l l) and a
// multiply that gathers the four flag bits (nib_gather).  The per-layer pack reads the plane once per layer (0.25 ms at 4096^2 x 8 in front of the walks).
__global__ __launch_bounds__(256) void k_bits_pack_labels(const u8* __restrict__ labels, unsigned long long* __restrict__ bits, int H, int W, int Ww, int K) {
    const size_t wi = (size_t)blockIdx.x * 256 + threadIdx.x, nw = (size_t)H * Ww;
    if (wi >= nw) return;
    const uint4* p = reinterpret_cast<const uint4*>(labels + wi * 64);          // W == 64 * Ww: word wi holds the pixels 64 wi .. 64 wi + 63 of the plane
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 4; q++) { const uint4 v = p[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    for (int l = 0; l < K; l++) {
        const uint32_t rep = 0x01010101u * (uint32_t)l;
        unsigned long long b = 0;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const uint32_t x = w[q] ^ rep;
            const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);          // 0x80 in every byte of x that is zero, 0 elsewhere
            const uint32_t nib = nib_gather(z >> 7);                                            // bits 0, 8, 16, 24 -> bits 0 .. 3
            b |= (unsigned long long)nib << (4 * q);
        }
        bits[nw * l + wi] = b;
    }
}
// one bit per pixel -> 0 / 255 bytes, 16 pixels (ONE 16-byte store) per thread: rows that are multiples of 64 wide (nw words per plane = H * W / 64),
// blockIdx.z = plane.  Four bits become four bytes through nib_spread (bitplane.h).
__global__ __launch_bounds__(256) void k_bits_expand16(const unsigned long long* __restrict__ bits, uint8_t* __restrict__ dst, size_t nw) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nw * 4) return;
    const unsigned long long w = bits[nw * blockIdx.z + (t >> 2)];
    const unsigned n16 = (unsigned)(w >> ((t & 3) * 16)) & 0xffffu;
    auto four = [](unsigned n4) { return nib_spread(n4) * 0xffu; };
    uint4 o; o.x = four(n16); o.y = four(n16 >> 4); o.z = four(n16 >> 8); o.w = four(n16 >> 12);
    reinterpret_cast<uint4*>(dst + nw * 64 * blockIdx.z)[t] = o;
}
void orip_bits_expand16(orip_ctx* c, const unsigned long long* bits, uint8_t* dst, size_t nw, int K) {      // (stage 03 expands its edge planes with it too)
    hipLaunchKernelGGL(k_bits_expand16, dim3((unsigned)cdiv((int64_t)nw * 4, 256), 1, K), dim3(256), 0, LN(c).stream, bits, dst, nw);
}
__global__ __launch_bounds__(256) void k_morph_bits(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, int H, int W, int Ww, int k,
                                                     unsigned long long se, int dilate) {
    const int layer = blockIdx.z;
    const size_t wi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (wi >= (size_t)H * Ww) return;
    const int y = (int)(wi / Ww), xw = (int)(wi % Ww), r = k >> 1;
    const unsigned long long* s = src + (size_t)H * Ww * layer;
    const unsigned long long neutral = dilate ? 0ULL : ~0ULL;
    const int tail = W - (Ww - 1) * 64;                                       // valid bits of the last word of a row
    const unsigned long long tail_mask = tail >= 64 ? ~0ULL : ((1ULL << tail) - 1ULL);
    auto word = [&](int yy, int xx) -> unsigned long long {                   // row yy, word xx with out-of-image bits made neutral
        if (yy < 0 || yy >= H || xx < 0 || xx >= Ww) return neutral;
        unsigned long long w = s[(size_t)yy * Ww + xx];
        if (xx == Ww - 1) w = dilate ? (w & tail_mask) : (w | ~tail_mask);
        return w;
    };
    unsigned long long out = neutral;
    for (int a = 0; a < k; a++) {
        if (!((se >> (a * k)) & ((1ULL << k) - 1ULL))) continue;
        const int yy = y + a - r;
        const unsigned long long L = word(yy, xw - 1), M = word(yy, xw), Rw = word(yy, xw + 1);
        for (int b = 0; b < k; b++) {
            if (!((se >> (a * k + b)) & 1ULL)) continue;
            const int sft = b - r;                                             // output bit x takes source bit x + sft
            unsigned long long v = sft == 0 ? M : (sft > 0 ? ((M >> sft) | (Rw << (64 - sft))) : ((M << -sft) | (L >> (64 + sft))));
            out = dilate ? (out | v) : (out & v);
        }
    }
    dst[(size_t)H * Ww * layer + wi] = out;
}
// 1 if any byte of the planes is neither 0 nor 255
__global__ __launch_bounds__(256) void k_not_binary(const u8* __restrict__ src, size_t n, int* __restrict__ flag) {
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    bool bad = false;
    for (int j = 0; j < 16 && i + j < n; j++) { const u8 v = src[i + j]; bad |= (v != 0 && v != 255); }
    if (bad) *flag = 1;
}

// open (erode^n, dilate^n) then close (dilate^n, erode^n); src plane(s) -> dst plane(s); uses tmpA as ping-pong
// unpack == false: when the chain ran on bit planes, leave the result there (c->morphed_bits) and do not write the byte planes (stage 03)
int orip_morph_open_close(orip_ctx* c, const u8* src, u8* dst, int K, int shape, int k, int open_iters, int close_iters, bool labels_mode, bool unpack) {
    if (k < 1 || k > 7 || (k & 1) == 0) ORIP_FAIL(c, "structuring element size %d unsupported (odd, 1..7)", k);
    int H = c->H, W = c->W; size_t plane = (size_t)H * W;
    unsigned long long se = make_se_bits(shape, k);
    std::vector<int> passes;   // 0 erode, 1 dilate
    for (int i = 0; i < std::max(open_iters, 0); i++) passes.push_back(0);
    for (int i = 0; i < std::max(open_iters, 0); i++) passes.push_back(1);
    for (int i = 0; i < std::max(close_iters, 0); i++) passes.push_back(1);
    for (int i = 0; i < std::max(close_iters, 0); i++) passes.push_back(0);
    if (passes.empty()) passes.push_back(-1);   // identity copy via 1x1 "erode"
    // binary input (label masks always are; explicit masks are checked): the chain runs on bit planes
    const bool have_bits = !labels_mode && c->mask_bits != nullptr && src == c->masks.as<u8>() && !getenv("ORIP_MORPH_BYTES");   // stage 02 left them
    bool binary = labels_mode || have_bits;
    if (!binary && !getenv("ORIP_MORPH_BYTES")) {
        int* d_flag = &LN(c).flags.as<LaneFlags>()->not_binary;
        HIPC(c, hipMemsetAsync(d_flag, 0, 4, LN(c).stream));
        hipLaunchKernelGGL(k_not_binary, dim3((unsigned)cdiv((int64_t)(plane * K), 4096)), dim3(256), 0, LN(c).stream, src, plane * K, d_flag);
        int h = 1; HIPC(c, hipMemcpyAsync(&h, d_flag, 4, hipMemcpyDeviceToHost, LN(c).stream)); HIPC(c, hipStreamSynchronize(LN(c).stream));
        binary = h == 0;
    }
    if (binary && passes[0] >= 0 && !getenv("ORIP_MORPH_BYTES")) {
        const int Ww = (W + 63) >> 6; const size_t nw = (size_t)H * Ww;
        HIPC(c, c->tmpA.ensure(std::max(plane * K, nw * K * 16 + 64)));
        unsigned long long* A = c->tmpA.as<unsigned long long>(); unsigned long long* B = A + nw * K;
        dim3 gw((unsigned)cdiv((int64_t)nw, 256), 1, K), block(256);
        if (have_bits) { if (c->mask_bits == (const void*)B) std::swap(A, B); }        // the planes are already there (first or second half)
        else if (labels_mode && (W & 63) == 0 && !getenv("ORIP_PACK_BYTES")) hipLaunchKernelGGL(k_bits_pack_labels, dim3(gw.x), block, 0, LN(c).stream, src, A, H, W, Ww, K);
        else if (labels_mode) hipLaunchKernelGGL(k_pack_bits<PackLabels>, gw, block, 0, LN(c).stream, src, A, H, W, Ww);
        else bp_pack_bytes(LN(c).stream, gw, src, A, H, W, Ww);
        c->mask_bits = nullptr;
        for (size_t i = 0; i < passes.size(); i++) {
            ProfScope ps(c, "k_morph_bits");
            hipLaunchKernelGGL(k_morph_bits, gw, block, 0, LN(c).stream, A, B, H, W, Ww, k, se, passes[i] == 1 ? 1 : 0);
            std::swap(A, B);
        }
        if (unpack && (W & 63) == 0 && !getenv("ORIP_PACK_BYTES")) orip_bits_expand16(c, A, dst, nw, K);
        else if (unpack) bp_bits_to_bytes(LN(c).stream, gw, A, dst, H, W, Ww);
        else c->morphed_bits = A;
        HIPC(c, hipGetLastError());
        if (labels_mode && dst == c->masks.as<u8>()) c->mask_bits = A;      // stage 03 can start from the bit planes
        return 0;
    }
    c->mask_bits = nullptr;                       // the byte passes ping-pong through tmpA
    HIPC(c, c->tmpA.ensure(plane * K));
    dim3 grid(cdiv(W, MT_X), cdiv(H, MT_Y), K), block(256);
    const u8* cur = src; bool lm = labels_mode;
    int np_ = (int)passes.size();
    for (int i = 0; i < np_; i++) {
        // choose outputs so that the last pass lands in dst
        u8* out = ((np_ - 1 - i) % 2 == 0) ? dst : c->tmpA.as<u8>();
        if (out == cur) ORIP_FAIL(c, "internal: in-place morph pass");
        int kk = passes[i] < 0 ? 1 : k; unsigned long long ss = passes[i] < 0 ? 1ULL : se;
        {
            ProfScope ps(c, "k_morph_pass");
            hipLaunchKernelGGL(k_morph_pass, grid, block, 0, LN(c).stream, cur, out, H, W, kk, ss, passes[i] == 1 ? 1 : 0, lm ? 1 : 0);
        }
        cur = out; lm = false;
    }
    HIPC(c, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// host entry points
// ------------------------------------------------------------------------------------------------
extern "C" int orip_set_image(orip_ctx* c, const uint8_t* bgr, int H, int W) {
    orip_enter(c);
    ORIP_TRY(orip_contours_invalidate(c));
    c->mask_bits = nullptr; c->an_ready = false;
    if (!bgr || H <= 0 || W <= 0) ORIP_FAIL(c, "bad image %dx%d", W, H);
    ORIP_TRY(orip_raster02_lab_tables(c));
    c->H = H; c->W = W;
    c->km_drop_unless((int64_t)H * W);          // (a sample set made for another pixel count)
    HIPC(c, c->image.ensure((size_t)H * W * 3 + 16));
    HIPC(c, hipMemcpyAsync(c->image.p, bgr, (size_t)H * W * 3, hipMemcpyHostToDevice, LN(c).stream));
    return 0;
}

extern "C" int orip_lab_of(orip_ctx* c, const int64_t* idx, int64_t n, uint8_t* lab_out) {
    orip_enter(c);
    if (!c->image.p) ORIP_FAIL(c, "no image set");
    ORIP_TRY(orip_contours_invalidate(c));       // (the index list goes to tmpC, the state bytes of stage 04's schedule)
    if (!idx) n = (int64_t)c->H * c->W;
    HIPC(c, c->tmpB.ensure((size_t)n * 3 + 16));
    if (idx) { HIPC(c, c->tmpC.ensure((size_t)n * 8)); HIPC(c, hipMemcpyAsync(c->tmpC.p, idx, (size_t)n * 8, hipMemcpyHostToDevice, LN(c).stream)); }
    hipLaunchKernelGGL(k_lab_gather, dim3(std::min<int64_t>(2048, cdiv(n, 256))), dim3(256), 0, LN(c).stream, c->image.as<u8>(),
                       idx ? c->tmpC.as<int64_t>() : nullptr, n, c->tmpB.as<u8>(), c->lab_tabs.as<LabTabs>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(lab_out, c->tmpB.p, (size_t)n * 3, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    return 0;
}

// analyze_colors.py: the same BGR2LAB for a short list of R, G, B triples (palette colours, cluster centres), so the palette logic measures in stage 02's Lab
extern "C" int orip_lab_of_rgb(orip_ctx* c, const uint8_t* rgb, int64_t n, uint8_t* lab_out) {
    orip_enter(c);
    if (n < 0 || n > (1 << 24) || (n && (!rgb || !lab_out))) ORIP_FAIL(c, "bad colour list (n = %lld)", (long long)n);
    if (n == 0) return 0;
    ORIP_TRY(orip_raster02_lab_tables(c));
    std::vector<u8> bgr((size_t)n * 3);
    for (int64_t i = 0; i < n; i++) { bgr[3 * i] = rgb[3 * i + 2]; bgr[3 * i + 1] = rgb[3 * i + 1]; bgr[3 * i + 2] = rgb[3 * i]; }
    HIPC(c, LN(c).tmpE.ensure((size_t)n * 6 + 32));
    u8* d_in = LN(c).tmpE.as<u8>(); u8* d_out = d_in + (size_t)n * 3 + 16;
    HIPC(c, hipMemcpyAsync(d_in, bgr.data(), (size_t)n * 3, hipMemcpyHostToDevice, LN(c).stream));
    hipLaunchKernelGGL(k_lab_gather, dim3(std::min<int64_t>(2048, cdiv(n, 256))), dim3(256), 0, LN(c).stream, d_in, (const int64_t*)nullptr, n, d_out, c->lab_tabs.as<LabTabs>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(lab_out, d_out, (size_t)n * 3, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));       // (also keeps `bgr` alive until the upload is done)
    return 0;
}

// process_colors.py assign_labels: labels u8 [H,W] of the image against an RGB palette, resident (orip_get_labels) and optionally on the host
extern "C" int orip_assign_palette(orip_ctx* c, const uint8_t* palette_rgb, int K, uint8_t* labels_out, int64_t* counts_out) {
    orip_enter(c);
    c->mask_bits = nullptr;
    if (!c->image.p) ORIP_FAIL(c, "no image set");
    if (!palette_rgb || K < 1 || K > ORIP_MAX_LAYERS) ORIP_FAIL(c, "K=%d out of range 1..%d", K, ORIP_MAX_LAYERS);
    const int64_t npx = (int64_t)c->H * c->W;
    hipStream_t s = LN(c).stream;
    HIPC(c, c->labels.ensure((size_t)npx + 16));
    LaneFlags* fl = LN(c).flags.as<LaneFlags>(); u8* d_pal = fl->palette;
    HIPC(c, hipMemcpyAsync(d_pal, palette_rgb, (size_t)K * 3, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(c, "k_assign_palette");
        hipLaunchKernelGGL(k_assign_palette, dim3((unsigned)cdiv(cdiv(npx, 4), 256)), dim3(256), 0, s, c->image.as<u8>(), npx, d_pal, K, c->labels.as<u8>());
    }
    HIPC(c, hipGetLastError());
    if (counts_out) {
        unsigned long long* d_counts = fl->palette_counts;
        HIPC(c, hipMemsetAsync(d_counts, 0, sizeof(LaneFlags::palette_counts), s));
        hipLaunchKernelGGL(k_count_labels, dim3(512), dim3(256), 0, s, c->labels.as<u8>(), npx, d_counts);
        unsigned long long h[ORIP_MAX_LAYERS];
        HIPC(c, hipMemcpyAsync(h, d_counts, sizeof(h), hipMemcpyDeviceToHost, s));
        HIPC(c, hipStreamSynchronize(s));
        for (int k = 0; k < K; k++) counts_out[k] = (int64_t)h[k];
    }
    if (labels_out) HIPC(c, hipMemcpyAsync(labels_out, c->labels.p, (size_t)npx, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}

extern "C" int orip_extract_layers(orip_ctx* c, const float* centers, int K, int open_iters, int close_iters,
                                   float* centers_sorted_out, int64_t* counts_out) {
    orip_enter(c);
    if (!c->image.p) ORIP_FAIL(c, "no image set");
    if (K < 1 || K > ORIP_MAX_LAYERS) ORIP_FAIL(c, "K=%d out of range", K);
    ORIP_TRY(orip_contours_invalidate(c));
    int H = c->H, W = c->W; int64_t npx = (int64_t)H * W;
    // order = argsort(L) (stable), lut[order] = arange (02:121-127)
    std::vector<int> order(K);
    for (int i = 0; i < K; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return centers[3 * a] < centers[3 * b]; });
    Centers cs; cs.K = K;
    for (int i = 0; i < K * 3; i++) cs.c[i] = centers[i];
    for (int r = 0; r < K; r++) cs.lut[order[r]] = (uint8_t)r;
    if (centers_sorted_out) for (int r = 0; r < K; r++) for (int j = 0; j < 3; j++) centers_sorted_out[3 * r + j] = centers[3 * order[r] + j];
    c->K = K;
    HIPC(c, c->labels.ensure((size_t)npx + 16));
    HIPC(c, c->masks.ensure((size_t)npx * K));
    {
        ProfScope ps(c, "k_lab_assign");
        hipLaunchKernelGGL(k_lab_assign, dim3(std::min<int64_t>(4096, std::max<int64_t>(1, cdiv(npx / 4, 256)))), dim3(256), 0, LN(c).stream,
                           c->image.as<u8>(), c->labels.as<u8>(), npx, c->lab_tabs.as<LabTabs>(), cs);
    }
    HIPC(c, hipGetLastError());
    if (counts_out) {
        unsigned long long* d_cnt = LN(c).flags.as<LaneFlags>()->label_counts;
        HIPC(c, hipMemsetAsync(d_cnt, 0, ORIP_MAX_LAYERS * 8, LN(c).stream));
        hipLaunchKernelGGL(k_count_labels, dim3(1024), dim3(256), 0, LN(c).stream, c->labels.as<u8>(), npx, d_cnt);
        unsigned long long h[ORIP_MAX_LAYERS];
        HIPC(c, hipMemcpyAsync(h, d_cnt, ORIP_MAX_LAYERS * 8, hipMemcpyDeviceToHost, LN(c).stream));
        HIPC(c, hipStreamSynchronize(LN(c).stream));
        for (int k = 0; k < K; k++) counts_out[k] = (int64_t)h[k];
    }
    return orip_morph_open_close(c, c->labels.as<u8>(), c->masks.as<u8>(), K, 0, 3, open_iters, close_iters, true);
}

extern "C" int orip_get_labels(orip_ctx* c, uint8_t* out) {
    orip_enter(c);
    if (!c->labels.p) ORIP_FAIL(c, "no labels resident");
    HIPC(c, hipMemcpyAsync(out, c->labels.p, (size_t)c->H * c->W, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    return 0;
}
extern "C" int orip_get_mask(orip_ctx* c, int layer, uint8_t* out) {
    orip_enter(c);
    if (!c->masks.p || layer < 0 || layer >= c->K) ORIP_FAIL(c, "no mask for layer %d", layer);
    size_t plane = (size_t)c->H * c->W;
    HIPC(c, hipMemcpyAsync(out, c->masks.as<u8>() + plane * layer, plane, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    return 0;
}
extern "C" int orip_set_masks(orip_ctx* c, const uint8_t* masks, int K, int H, int W) {
    orip_enter(c);
    c->mask_bits = nullptr;
    if (K < 1 || K > ORIP_MAX_LAYERS || H <= 0 || W <= 0) ORIP_FAIL(c, "bad shape");
    ORIP_TRY(orip_contours_invalidate(c));
    c->H = H; c->W = W; c->K = K;
    HIPC(c, c->masks.ensure((size_t)H * W * K));
    HIPC(c, hipMemcpyAsync(c->masks.p, masks, (size_t)H * W * K, hipMemcpyHostToDevice, LN(c).stream));
    return 0;
}

extern "C" int orip_keep_layers(orip_ctx* c, const int32_t* layers, int n) {
    orip_enter(c);
    c->edge_bits = nullptr;
    c->mask_bits = nullptr;
    if (!c->masks.p || n < 1 || n > c->K) ORIP_FAIL(c, "bad layer subset (n=%d, K=%d)", n, c->K);
    ORIP_TRY(orip_contours_invalidate(c));
    size_t plane = (size_t)c->H * c->W;
    for (int i = 0; i < n; i++) {
        if (layers[i] < i || layers[i] >= c->K || (i && layers[i] <= layers[i - 1])) ORIP_FAIL(c, "layer subset must be strictly increasing and within range");
        if (layers[i] != i) HIPC(c, hipMemcpyAsync(c->masks.as<u8>() + plane * i, c->masks.as<u8>() + plane * layers[i], plane, hipMemcpyDeviceToDevice, LN(c).stream));
    }
    c->K = n;
    return 0;
}
