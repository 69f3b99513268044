// csrc/stream.hip -- the data-parallel part of 13_build_stream.py: direction codes of every move of a plot (pen-up travels and the
// segments of every polyline), shared/omnirevolve_plotter_stream_creator_helper.py bresenham_dir_codes (:183-207).
//
// The reference walks each segment with an error accumulator (one iteration per step, serial).  The accumulator has a closed form: with
// dx = |x1 - x0| >= dy = |y1 - y0| the major axis moves in every iteration and the minor axis has moved
//     m(j) = max(0, ceil((2 j dy - dx) / (2 dx)))          times after j iterations
// (the minor move of iteration k happens iff m(k) < (2 (k + 1) dy - dx) / (2 dx), which is the helper's strict test `e2 < dx` with the
// error written out; symmetric for dy > dx with its strict `e2 > -dy`).  Step k of a segment is therefore independent of every other step:
// one thread per step over the concatenated moves of the whole plot, 64-bit integer arithmetic, no serial chain.
// Codes (helper :24-25): 0 +Y, 1 NE, 2 +X, 3 SE, 4 -Y, 5 SW, 6 -X, 7 NW.
//
// Pack (orip_stream_pack): the bytes of the finished stream (StreamWriter.add_steps / finalize, helper :55-68, :166-175).  The host plans the pieces (first
// code, step count, byte position, speed byte or none) and the service bytes; one thread per output byte finds its piece by binary search over the byte
// positions and writes the speed byte or the step byte (two codes per byte, paired inside the piece; the last byte of an odd piece holds one), or zero; a
// second kernel drops the service bytes (the end byte among them) in.  The direction codes are the resident result of orip_stream_codes and never leave
// the device.
#include "orip_ctx.h"
#include <rocprim/rocprim.hpp>

__global__ __launch_bounds__(256) void k_seg_counts(const int4* __restrict__ segs, int64_t n, unsigned long long* __restrict__ cnt) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { cnt[i] = 0; return; }
    const int4 s = segs[i];
    const long long dx = llabs((long long)s.z - s.x), dy = llabs((long long)s.w - s.y);
    cnt[i] = (unsigned long long)(dx > dy ? dx : dy);
}

__device__ __forceinline__ long long ceil_div_pos(long long a, long long b) {      // ceil(a / b), b > 0, clamped at 0 from below
    return a <= 0 ? 0 : (a + b - 1) / b;
}

__global__ __launch_bounds__(256) void k_seg_codes(const int4* __restrict__ segs, int64_t n, const unsigned long long* __restrict__ off, unsigned long long total,
                                                   uint8_t* __restrict__ codes) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    // segment of step t: the last i with off[i] <= t (segments without steps have off[i] == off[i + 1] and are skipped by the search)
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= t) lo = mid; else hi = mid; }
    const int4 s = segs[lo];
    const long long k = (long long)(t - off[lo]);
    const long long dx = llabs((long long)s.z - s.x), dy = llabs((long long)s.w - s.y);
    const bool xpos = s.x < s.z, ypos = s.y < s.w;                  // helper: sx = 1 if x0 < x1 else -1 (same for y)
    bool mx, my;
    if (dx >= dy) { mx = true; my = ceil_div_pos(2 * (k + 1) * dy - dx, 2 * dx) != ceil_div_pos(2 * k * dy - dx, 2 * dx); }
    else { my = true; mx = ceil_div_pos(2 * (k + 1) * dx - dy, 2 * dy) != ceil_div_pos(2 * k * dx - dy, 2 * dy); }
    int c;
    if (mx && my) c = xpos ? (ypos ? 1 : 3) : (ypos ? 7 : 5);
    else if (mx) c = xpos ? 2 : 6;
    else c = ypos ? 0 : 4;
    codes[t] = (uint8_t)c;
}

// Direction codes of n moves (x0, y0, x1, y1), resident until the next call; *total = number of steps.
extern "C" int orip_stream_codes(orip_ctx* c, const int32_t* segs, int64_t n, int64_t* total) {
    orip_enter(c);
    if (!total || n < 0 || (n > 0 && !segs)) ORIP_FAIL(c, "bad arguments");
    *total = 0; c->stream_n = 0; c->stream_total = 0;
    if (n == 0) return 0;
    hipStream_t s = LN(c).stream;
    HIPC(c, c->stream_segs.ensure((size_t)n * 16 + 64));
    HIPC(c, c->stream_off.ensure((size_t)(n + 1) * 16 + 64));
    unsigned long long* cnt = c->stream_off.as<unsigned long long>() + (n + 1); unsigned long long* off = c->stream_off.as<unsigned long long>();
    HIPC(c, hipMemcpyAsync(c->stream_segs.p, segs, (size_t)n * 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_seg_counts, dim3(cdiv(n + 1, 256)), dim3(256), 0, s, c->stream_segs.as<int4>(), n, cnt);
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, cnt, off, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), s); }));
    unsigned long long h_total = 0;
    HIPC(c, hipMemcpyAsync(&h_total, off + n, 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    HIPC(c, c->stream_codes.ensure((size_t)h_total + 64));
    if (h_total) {
        ProfScope ps(c, "k_seg_codes");
        hipLaunchKernelGGL(k_seg_codes, dim3((unsigned)((h_total + 255) / 256)), dim3(256), 0, s, c->stream_segs.as<int4>(), n, off, h_total, c->stream_codes.as<uint8_t>());
    }
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    c->stream_n = n; c->stream_total = (int64_t)h_total; *total = (int64_t)h_total;
    return 0;
}

extern "C" int orip_stream_codes_fetch(orip_ctx* c, int64_t* off_out, uint8_t* codes_out) {
    orip_enter(c);
    if (!off_out) ORIP_FAIL(c, "bad arguments");
    if (c->stream_n == 0) { off_out[0] = 0; return 0; }
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(off_out, c->stream_off.p, (size_t)(c->stream_n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (c->stream_total && codes_out) HIPC(c, hipMemcpyAsync(codes_out, c->stream_codes.p, (size_t)c->stream_total, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}

// ------------------------------------------------------------------------------------------------ pack
__global__ __launch_bounds__(256) void k_pk_bytes(const long long* __restrict__ pos, const long long* __restrict__ code0, const int* __restrict__ cnt,
                                                  const int* __restrict__ speed, int64_t np, const uint8_t* __restrict__ codes, int64_t nbytes, uint8_t* __restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nbytes) return;
    unsigned v = 0;
    if (np > 0 && b >= pos[0]) {
        int64_t lo = 0, hi = np;                                             // last piece that starts at or before this byte
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (pos[mid] <= b) lo = mid; else hi = mid; }
        const int c = cnt[lo], sp = speed[lo];
        const int64_t j = b - pos[lo] - (sp >= 0 ? 1 : 0);                   // step byte j of the piece; -1: its speed byte
        if (j < 0) v = (unsigned)sp;
        else if (2 * j < c) {
            const uint8_t* q = codes + code0[lo] + 2 * j;
            const unsigned a = q[0] & 7u;
            v = 2 * j + 1 < c ? (0xC0u | (a << 3) | (q[1] & 7u)) : (0x80u | (a << 3));
        }
    }
    out[b] = (uint8_t)v;
}
__global__ __launch_bounds__(256) void k_pk_service(const long long* __restrict__ pos, const uint8_t* __restrict__ val, int64_t ns, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ns) out[pos[i]] = val[i];
}

// the bytes of a stream from the resident direction codes of orip_stream_codes and the host's plan
extern "C" int orip_stream_pack(orip_ctx* c, int64_t n_pieces, const int64_t* code0, const int32_t* cnt, const int64_t* pos, const int32_t* speed, int64_t n_service,
                                const int64_t* svc_pos, const uint8_t* svc_val, int64_t nbytes) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    c->pk_bytes = -1;
    if (n_pieces < 0 || n_service < 0 || nbytes < 0 || (n_pieces > 0 && (!code0 || !cnt || !pos || !speed)) || (n_service > 0 && (!svc_pos || !svc_val))) ORIP_FAIL(c, "bad arguments");
    // every piece reads inside the resident codes and writes inside the stream, behind the piece before it: nothing below can leave its buffers
    int64_t end = 0;
    for (int64_t i = 0; i < n_pieces; i++) {
        const int64_t size = (speed[i] >= 0 ? 1 : 0) + ((int64_t)cnt[i] + 1) / 2;
        if (cnt[i] < 0 || speed[i] > 255 || size < 1 || code0[i] < 0 || code0[i] + cnt[i] > c->stream_total || pos[i] < end || pos[i] + size > nbytes)
            ORIP_FAIL(c, "piece %lld does not fit (%lld codes from %lld of %lld resident, %lld bytes at %lld of %lld, previous piece ends at %lld)", (long long)i, (long long)cnt[i],
                      (long long)code0[i], (long long)c->stream_total, (long long)size, (long long)pos[i], (long long)nbytes, (long long)end);
        end = pos[i] + size;
    }
    for (int64_t i = 0; i < n_service; i++) if (svc_pos[i] < 0 || svc_pos[i] >= nbytes) ORIP_FAIL(c, "service byte %lld at %lld of %lld", (long long)i, (long long)svc_pos[i], (long long)nbytes);
    if (nbytes == 0) { c->pk_bytes = 0; return 0; }
    hipStream_t s = LN(c).stream;
    long long *d_pos, *d_code0, *d_spos; int *d_cnt, *d_speed; uint8_t* d_sval;
    { Carve L; L.take(d_pos, (size_t)n_pieces); L.take(d_code0, (size_t)n_pieces); L.take(d_spos, (size_t)n_service); L.take(d_cnt, (size_t)n_pieces); L.take(d_speed, (size_t)n_pieces);
      L.take(d_sval, (size_t)n_service); HIPC(c, L.commit(c->pk_tab, 64)); }
    HIPC(c, c->pk_out.ensure((size_t)nbytes + 64));
    if (n_pieces) {
        HIPC(c, hipMemcpyAsync(d_pos, pos, (size_t)n_pieces * 8, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_code0, code0, (size_t)n_pieces * 8, hipMemcpyHostToDevice, s));
        HIPC(c, hipMemcpyAsync(d_cnt, cnt, (size_t)n_pieces * 4, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_speed, speed, (size_t)n_pieces * 4, hipMemcpyHostToDevice, s));
    }
    if (n_service) { HIPC(c, hipMemcpyAsync(d_spos, svc_pos, (size_t)n_service * 8, hipMemcpyHostToDevice, s)); HIPC(c, hipMemcpyAsync(d_sval, svc_val, (size_t)n_service, hipMemcpyHostToDevice, s)); }
    { ProfScope ps(c, "k_pk_bytes");
      hipLaunchKernelGGL(k_pk_bytes, dim3((unsigned)((nbytes + 255) / 256)), dim3(256), 0, s, d_pos, d_code0, d_cnt, d_speed, n_pieces, c->stream_codes.as<uint8_t>(), nbytes,
                         c->pk_out.as<uint8_t>()); }
    if (n_service) hipLaunchKernelGGL(k_pk_service, dim3((unsigned)((n_service + 255) / 256)), dim3(256), 0, s, d_spos, d_sval, n_service, c->pk_out.as<uint8_t>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(s));
    c->pk_bytes = nbytes;
    return 0;
}

extern "C" int orip_stream_pack_fetch(orip_ctx* c, uint8_t* out) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (c->pk_bytes < 0) ORIP_FAIL(c, "no packed stream: orip_stream_pack has not succeeded since the last failure");
    if (c->pk_bytes == 0) return 0;
    if (!out) ORIP_FAIL(c, "bad arguments");
    hipStream_t s = LN(c).stream;
    HIPC(c, hipMemcpyAsync(out, c->pk_out.p, (size_t)c->pk_bytes, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
