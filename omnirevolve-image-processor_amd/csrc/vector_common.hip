// csrc/vector_common.hip -- the plumbing the vector stages (05, 07, 08, 10, 12) share (vec_common.h): the rocPRIM wrappers, the point source of a list,
// the descriptor-driven gather and the runs-to-polylines helper, with the kernels behind them (internal to this unit).  The features are in
// vector_features.hip, the greedy order in vector_greedy.hip.
#include "vec_common.h"
#include <rocprim/rocprim.hpp>

namespace {
// exclusive prefix sums of up to 32 768 integers by ONE workgroup (thread t owns the items [t * per, (t + 1) * per)): the lists of this path are a few
// thousand polylines long, and rocPRIM's scan is two dispatches (look-back state, scan) at ~50 us each on a queue that shares the card.  in == out is fine.
// (256 threads: a 1024-thread workgroup waits for a CU with sixteen free wave slots, which costs ~0.5 ms on a card the other layers keep full.)
template <class T>
__global__ __launch_bounds__(256) void k_scan_small(const T* in, T* out, unsigned n, unsigned per) {
    __shared__ T wsum[16];
    const unsigned tid = threadIdx.x, lo = tid * per, hi = min(n, lo + per);
    T mine = 0;
    for (unsigned i = lo; i < hi; i++) mine += in[i];
    T inc = mine;
    for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_up(inc, o, 64); if ((int)(tid & 63u) >= o) inc += t; }
    if ((tid & 63u) == 63u) wsum[tid >> 6] = inc;
    __syncthreads();
    T base = 0;
    for (unsigned w = 0; w < (tid >> 6); w++) base += wsum[w];
    T run = base + inc - mine;
    __syncthreads();
    for (unsigned i = lo; i < hi; i++) { const T v = in[i]; out[i] = run; run += v; }
}
}  // namespace
template <class T>
int vscan_excl(orip_ctx* c, const T* in, T* out, size_t n) {
    if (n == 0) return 0;
    if (n <= 32768) {
        hipLaunchKernelGGL(k_scan_small<T>, dim3(1), dim3(256), 0, LN(c).stream, in, out, (unsigned)n, (unsigned)cdiv((int64_t)n, 256));
        HIPC(c, hipGetLastError());
        return 0;
    }
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, in, out, T(0), n, rocprim::plus<T>(), LN(c).stream); }));
    return 0;
}
template <class K, class V>
int vsort_pairs(orip_ctx* c, const K* kin, K* kout, const V* vin, V* vout, size_t n, int begin_bit, int end_bit, bool desc) {
    if (n == 0) return 0;
    HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) {
        return !desc ? rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, LN(c).stream)
                     : rocprim::radix_sort_pairs_desc(tmp, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, LN(c).stream); }));
    return 0;
}
template int vscan_excl<int64_t>(orip_ctx*, const int64_t*, int64_t*, size_t);
template int vscan_excl<unsigned>(orip_ctx*, const unsigned*, unsigned*, size_t);
template int vsort_pairs<unsigned, unsigned>(orip_ctx*, const unsigned*, unsigned*, const unsigned*, unsigned*, size_t, int, int, bool);
template int vsort_pairs<float, unsigned>(orip_ctx*, const float*, float*, const unsigned*, unsigned*, size_t, int, int, bool);
template int vsort_pairs<unsigned long long, unsigned>(orip_ctx*, const unsigned long long*, unsigned long long*, const unsigned*, unsigned*, size_t, int, int, bool);

int vsrc_of(orip_ctx* c, const DPolys& P, VSrc& out) {
    const WalkStore& WS = c->wstore[P.vlayer];
    if (P.vepoch != WS.epoch) ORIP_FAIL(c, "the walk records of layer %d this list was built on have been replaced by a newer orip_contours_layer", P.vlayer);
    out.off = P.off.as<int64_t>(); out.view = P.vident ? nullptr : P.vview.as<VView>(); out.walk = WS.walk.as<VWalk>();
    if (P.scaled && P.vsepoch != WS.sepoch) ORIP_FAIL(c, "the scaled walk records of layer %d this list was built on have been replaced by a newer orip_scale_vectors", P.vlayer);
    out.g.piece = WS.piece.as<VPiece>();
    out.g.own = P.scaled ? WS.own_s.as<int2>() : WS.own.as<int2>(); out.g.lxy = P.scaled ? WS.lxy_s.as<int2>() : WS.lxy.as<int2>();
    return 0;
}

namespace {
__global__ __launch_bounds__(256) void k_gather_lens(const GatherDesc* __restrict__ d, int64_t n, int64_t* __restrict__ lens) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) lens[i] = d[i].len;
    if (i == n) lens[i] = 0;
}
// flat form: a block copies 4096 consecutive OUTPUT points whatever polylines they belong to (one block per polyline would leave
// the long polylines as the tail of the launch); the polyline of a point is found by bisecting the output offsets once per block
// and walking forward from there
__global__ __launch_bounds__(256) void k_gather_pts(const GatherDesc* __restrict__ d, int64_t n, const int32_t* __restrict__ src,
                                                     const int64_t* __restrict__ out_off, int32_t* __restrict__ dst, int64_t total) {
    const int64_t start = (int64_t)blockIdx.x * 4096;
    if (start >= total) return;
    int64_t k = last_le(out_off, n, start);
    const int2* s2 = reinterpret_cast<const int2*>(src); int2* o2 = reinterpret_cast<int2*>(dst);
    for (int64_t idx = start + threadIdx.x; idx < min(total, start + 4096); idx += 256) {
        while (out_off[k + 1] <= idx) k++;           // empty polylines are skipped too
        const GatherDesc g = d[k];
        const int64_t j = idx - out_off[k];
        o2[idx] = s2[g.begin + (g.rev ? g.len - 1 - j : j)];
    }
}
__global__ __launch_bounds__(256) void k_view_select(const GatherDesc* __restrict__ d, int64_t n, const VView* __restrict__ sview, const VWalk* __restrict__ walk,
                                                      VView* __restrict__ out, int64_t* __restrict__ lens) {
    int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k == n) lens[k] = 0;
    if (k >= n) return;
    const GatherDesc g = d[k];
    VView s;
    if (sview) s = sview[g.src]; else { s.wid = (unsigned)g.src; s.first = 0u; s.len = walk[g.src].len; s.rev = 0u; }
    VView o; o.wid = s.wid; o.len = (unsigned)g.len; o.rev = s.rev ^ (g.rev ? 1u : 0u);
    o.first = s.rev ? s.first + s.len - (unsigned)g.len : s.first;
    out[k] = o; lens[k] = g.len;
}
// explicit points of a list of either kind: 4096 consecutive output points per block (as k_gather_pts)
template <class Src>
__global__ __launch_bounds__(256) void k_expand_pts(Src src, int64_t n, int2* __restrict__ dst, int64_t total) {
    const int64_t start = (int64_t)blockIdx.x * 4096;
    if (start >= total) return;
    int64_t k = last_le(src.off, n, start), kc = -1;
    auto cu = src.cur(k);
    for (int64_t idx = start + threadIdx.x; idx < min(total, start + 4096); idx += 256) {
        while (src.off[k + 1] <= idx) k++;
        if (k != kc) { cu = src.cur(k); kc = k; }
        dst[idx] = cu.at(idx - src.off[k]);
    }
}
}  // namespace

// the offsets of a gathered list: launch_lens(lens) enqueues the kernel that writes the n lengths and a 0 behind them (lens: tmpE), dst.off = their
// exclusive scan, dst.total = known_total or, when that is negative, the scan's last word read back
template <class LaunchLens>
static int gather_offsets(orip_ctx* c, int64_t n, DPolys& dst, int64_t known_total, LaunchLens launch_lens) {
    HIPC(c, dst.off.ensure((size_t)(n + 1) * 8 + 64));
    HIPC(c, LN(c).tmpE.ensure((size_t)(n + 1) * 8 + 64));
    ORIP_TRY(launch_lens(LN(c).tmpE.as<int64_t>()));
    ORIP_TRY(vscan_excl<int64_t>(c, LN(c).tmpE.as<int64_t>(), dst.off.as<int64_t>(), (size_t)n + 1));
    int64_t total = known_total;
    if (total < 0) ORIP_TRY(vread(c, &total, dst.off.as<int64_t>() + n));
    dst.total = total;
    return 0;
}
int vgather(orip_ctx* c, const GatherDesc* d, int64_t n, const int32_t* src, DPolys& dst, int64_t known_total) {
    if (n == 0) { HIPC(c, dst.clear(LN(c).stream)); return 0; }
    dst.n = n; dst.total = 0; dst.set_explicit();
    ORIP_TRY(gather_offsets(c, n, dst, known_total, [&](int64_t* lens) {
        hipLaunchKernelGGL(k_gather_lens, dim3(cdiv(n + 1, 256)), dim3(256), 0, LN(c).stream, d, n, lens); return 0; }));
    HIPC(c, dst.pts.ensure((size_t)std::max<int64_t>(dst.total, 1) * 8 + 64));
    if (dst.total > 0) hipLaunchKernelGGL(k_gather_pts, dim3((unsigned)cdiv(dst.total, 4096)), dim3(256), 0, LN(c).stream, d, n, src, dst.off.as<int64_t>(), dst.pts.as<int32_t>(), dst.total);
    HIPC(c, hipGetLastError());
    return 0;
}
int vgather_views(orip_ctx* c, const GatherDesc* d, int64_t n, const DPolys& src, DPolys& dst, int64_t known_total) {
    VSrc vs_; ORIP_TRY(vsrc_of(c, src, vs_));
    if (n == 0) { HIPC(c, dst.clear(LN(c).stream)); return 0; }      // (an empty list is explicit)
    dst.n = n; dst.total = 0;
    dst.virt = true; dst.pts_ok = false; dst.vident = false; dst.vlayer = src.vlayer; dst.vepoch = src.vepoch;
    dst.scaled = src.scaled; dst.vsepoch = src.vsepoch; dst.pf_tag = src.pf_tag;      // the views keep naming the source's walks: what was computed per walk and direction stays addressable
    HIPC(c, dst.vview.ensure((size_t)n * sizeof(VView) + 64));
    ORIP_TRY(gather_offsets(c, n, dst, known_total, [&](int64_t* lens) {
        hipLaunchKernelGGL(k_view_select, dim3(cdiv(n + 1, 256)), dim3(256), 0, LN(c).stream, d, n, vs_.view, vs_.walk, dst.vview.as<VView>(), lens); return 0; }));
    HIPC(c, hipGetLastError());
    return 0;
}
int vgather_list(orip_ctx* c, const GatherDesc* d, int64_t n, const DPolys& src, DPolys& dst, int64_t known_total) {
    if (is_coded(src)) return vgather_views(c, d, n, src, dst, known_total);
    return vgather(c, d, n, src.pts.as<int32_t>(), dst, known_total);
}
// ---- runs of accepted slots -> polylines (stage 08-A: samples; stage 10: cut steps)
__global__ __launch_bounds__(256) void k_run_starts(const uint8_t* __restrict__ sflag, unsigned n, unsigned* __restrict__ start) {
    unsigned s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    uint8_t f = sflag[s];
    start[s] = ((f & 1) && ((f & 2) || s == 0 || !(sflag[s - 1] & 1))) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_run_accum(const uint8_t* __restrict__ sflag, const unsigned* __restrict__ start, const unsigned* __restrict__ start_scan,
                                                    unsigned n, unsigned* __restrict__ rlen, unsigned* __restrict__ rbegin) {
    unsigned s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    if (!(sflag[s] & 1)) return;
    unsigned rid = start_scan[s] + start[s] - 1;      // inclusive scan - 1
    atomicAdd(&rlen[rid], 1u);
    if (start[s]) rbegin[rid] = s;
}
__global__ __launch_bounds__(256) void k_run_keep(const unsigned* __restrict__ rlen, unsigned n_runs, unsigned min_len, unsigned* __restrict__ keep) {
    unsigned r = blockIdx.x * 256 + threadIdx.x;
    if (r < n_runs) keep[r] = rlen[r] >= min_len ? 1u : 0u;
    if (r == n_runs) keep[r] = 0;
}
__global__ __launch_bounds__(256) void k_run_desc(const unsigned* __restrict__ rlen, const unsigned* __restrict__ rbegin, const unsigned* __restrict__ keep,
                                                   const unsigned* __restrict__ keep_scan, unsigned n_runs, GatherDesc* __restrict__ d) {
    unsigned r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_runs || !keep[r]) return;
    GatherDesc g; g.begin = rbegin[r]; g.len = rlen[r]; g.rev = 0; g.src = 0;
    d[keep_scan[r]] = g;
}

// Shared by stage 08-A and stage 10 (vec_common.h): turn per-slot flags (bit0 accepted, bit1 sequence start) + points into a DPolys of runs with >= 2 points
int orip_runs_to_polys(orip_ctx* c, const int2* spt, const uint8_t* sflag, unsigned n_slots, DPolys& dst) {
    HIPC(c, dst.clear(LN(c).stream));
    if (n_slots == 0) return 0;
    unsigned *start, *start_scan; { Carve L; L.each(n_slots, start, start_scan); HIPC(c, L.commit(LN(c).vtmp[VTL_RUN_STARTS], 64)); }
    hipLaunchKernelGGL(k_run_starts, dim3(cdiv(n_slots, 256)), dim3(256), 0, LN(c).stream, sflag, n_slots, start);
    ORIP_TRY(vscan_excl<unsigned>(c, start, start_scan, n_slots));
    unsigned a[2];
    HIPC(c, hipMemcpyAsync(&a[0], start_scan + (n_slots - 1), 4, hipMemcpyDeviceToHost, LN(c).stream));      // both words, one wait
    ORIP_TRY(vread(c, &a[1], start + (n_slots - 1)));
    unsigned n_runs = a[0] + a[1];
    if (n_runs == 0) return 0;
    unsigned *rlen, *rbegin, *keep, *keep_scan; GatherDesc* desc;
    { Carve L; L.each((size_t)n_runs + 1, rlen, rbegin, keep, keep_scan); L.take(desc, n_runs); HIPC(c, L.commit(LN(c).vtmp[VTL_TAIL_RUNS], 256)); }
    HIPC(c, hipMemsetAsync(rlen, 0, (size_t)(n_runs + 1) * 4, LN(c).stream));
    hipLaunchKernelGGL(k_run_accum, dim3(cdiv(n_slots, 256)), dim3(256), 0, LN(c).stream, sflag, start, start_scan, n_slots, rlen, rbegin);
    hipLaunchKernelGGL(k_run_keep, dim3(cdiv(n_runs + 1, 256)), dim3(256), 0, LN(c).stream, rlen, n_runs, 2u, keep);
    ORIP_TRY(vscan_excl<unsigned>(c, keep, keep_scan, (size_t)n_runs + 1));
    unsigned n_keep = 0;
    ORIP_TRY(vread(c, &n_keep, keep_scan + n_runs));
    if (n_keep == 0) return 0;
    hipLaunchKernelGGL(k_run_desc, dim3(cdiv(n_runs, 256)), dim3(256), 0, LN(c).stream, rlen, rbegin, keep, keep_scan, n_runs, desc);
    HIPC(c, hipGetLastError());
    return vgather(c, desc, n_keep, reinterpret_cast<const int32_t*>(spt), dst);
}

// explicit points of a walk-coded list, on request (orip_get_polys, consumers that read int32 pairs); enqueued on the calling lane's stream
int orip_polys_materialize(orip_ctx* c, DPolys& P) {
    if (!is_coded(P)) return 0;
    VSrc src; ORIP_TRY(vsrc_of(c, P, src));
    HIPC(c, P.pts.ensure((size_t)std::max<int64_t>(P.total, 1) * 8 + 64));
    if (P.n > 0 && P.total > 0) {
        ProfScope ps(c, "k_expand_pts");
        hipLaunchKernelGGL(k_expand_pts<VSrc>, dim3((unsigned)cdiv(P.total, 4096)), dim3(256), 0, LN(c).stream, src, P.n, reinterpret_cast<int2*>(P.pts.p), P.total);
    }
    HIPC(c, hipGetLastError());
    P.pts_ok = true;
    return 0;
}
