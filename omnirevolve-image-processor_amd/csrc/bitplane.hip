// csrc/bitplane.hip -- the bit-plane kernels that need no policy, behind the bp_* launchers of bitplane.h, and the CCL driver of stages 03 / 04
// (k_ccl_bits<IdsBlockRaster> and k_pack_bits<PackBytes> are compiled here and nowhere else).
#include "bitplane.h"

__global__ __launch_bounds__(256) void k_bits_to_bytes(const unsigned long long* __restrict__ bits, u8* __restrict__ dst, int H, int W, int Ww) {
    const size_t nw = (size_t)H * Ww, w0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (w0 >= nw) return;
    const unsigned long long* b = bits + nw * blockIdx.z; u8* d = dst + (size_t)H * W * blockIdx.z;
    const int lane = threadIdx.x & 63;
    const unsigned long long mine = (w0 + lane < nw) ? b[w0 + lane] : 0ULL;
    for (int j = 0; j < 64; j++) {
        const size_t wi = w0 + j; if (wi >= nw) break;
        const unsigned long long v = bcast64(mine, j);
        const int y = (int)(wi / Ww), x = (int)(wi % Ww) * 64 + lane;
        if (x < W) d[(size_t)y * W + x] = ((v >> lane) & 1ULL) ? 255 : 0;
    }
}
__global__ __launch_bounds__(256) void k_compact_count_bits(const unsigned long long* __restrict__ bits, size_t nwords, unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[4];
    const size_t wi = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned cnt = wi < nwords ? (unsigned)__popcll(bits[wi]) : 0u;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__global__ __launch_bounds__(256) void k_heads(const unsigned* __restrict__ keys, int64_t m, int64_t n, unsigned* __restrict__ head) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    head[i] = (i < m && (i == 0 || keys[i] != keys[i - 1])) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_comp_starts(const unsigned* __restrict__ head, const unsigned* __restrict__ head_scan, int64_t m,
                                                     unsigned* __restrict__ comp_start, unsigned nc) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) comp_start[nc] = (unsigned)m;
    if (i < m && head[i]) comp_start[head_scan[i]] = (unsigned)i;
}

void bp_pack_bytes(hipStream_t st, dim3 grid, const u8* src, unsigned long long* bits, int H, int W, int Ww) {
    hipLaunchKernelGGL(k_pack_bits<PackBytes>, grid, dim3(256), 0, st, src, bits, H, W, Ww);
}
void bp_bits_to_bytes(hipStream_t st, dim3 grid, const unsigned long long* bits, u8* dst, int H, int W, int Ww) {
    hipLaunchKernelGGL(k_bits_to_bytes, grid, dim3(256), 0, st, bits, dst, H, W, Ww);
}
void bp_compact_count(hipStream_t st, unsigned nblk, const unsigned long long* bits, size_t nwords, unsigned* counts) {
    hipLaunchKernelGGL(k_compact_count_bits, dim3(nblk), dim3(256), 0, st, bits, nwords, counts);
}
void bp_heads(hipStream_t st, const unsigned* keys, int64_t m, int64_t n, unsigned* head) {
    hipLaunchKernelGGL(k_heads, dim3(cdiv(n, 256)), dim3(256), 0, st, keys, m, n, head);
}
void bp_comp_starts(hipStream_t st, const unsigned* head, const unsigned* head_scan, int64_t m, unsigned* comp_start, unsigned nc) {
    hipLaunchKernelGGL(k_comp_starts, dim3(cdiv(m, 256)), dim3(256), 0, st, head, head_scan, m, comp_start, nc);
}

int orip_ccl_bits(orip_ctx* c, const unsigned long long* bits, int* par, int K) {
    const int H = c->H, W = c->W, Ww = (W + 63) >> 6;
    dim3 g((unsigned)cdiv((int64_t)H * Ww, 256), 1, K), block(256);
    { ProfScope ps(c, "k_ccl_init"); hipLaunchKernelGGL(k_ccl_bits<IdsBlockRaster>, g, block, 0, LN(c).stream, bits, par, H, W, Ww, 0); }
    { ProfScope ps(c, "k_ccl_bits"); hipLaunchKernelGGL(k_ccl_bits<IdsBlockRaster>, g, block, 0, LN(c).stream, bits, par, H, W, Ww, 1); }
    { ProfScope ps(c, "k_ccl_flatten"); hipLaunchKernelGGL(k_ccl_bits<IdsBlockRaster>, g, block, 0, LN(c).stream, bits, par, H, W, Ww, 2); }
    HIPC(c, hipGetLastError());
    return 0;
}
