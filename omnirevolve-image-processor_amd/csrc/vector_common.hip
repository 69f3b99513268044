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
// A run is a stretch of consecutive accepted slots, so its first slot and the number of accepted slots in front of it say everything: its length is the
// distance to the next run's count.  Nothing is written per slot; both passes over the flags write per tile or per run.
namespace {
// bit `bit` of each of the four flag bytes of w, as bits 0 .. 3
__device__ __forceinline__ unsigned flag_bits4(unsigned w, int bit) { return ((((w >> bit) & 0x01010101u) * 0x01020408u) >> 24) & 0xfu; }
// The 16 slots of one lane, from s0 on: acc = accepted (bit i: slot s0 + i), st = accepted and first of a run.  One 16-byte load where the flags allow it
// (wide: sflag is 16-byte aligned, which Carve gives both callers; s0 is a multiple of 16), byte loads for the last, partial group or an unaligned array.
// Every lane of the wave must call it (the slot in front of s0 comes from the lane before).
__device__ __forceinline__ void run_lane_flags(const uint8_t* __restrict__ sflag, unsigned n, unsigned s0, bool wide, unsigned& acc, unsigned& st) {
    unsigned seq = 0; acc = 0;
    if (wide && s0 < n && n - s0 >= 16u) {
        const uint4 q = *reinterpret_cast<const uint4*>(sflag + s0);
        acc = flag_bits4(q.x, 0) | flag_bits4(q.y, 0) << 4 | flag_bits4(q.z, 0) << 8 | flag_bits4(q.w, 0) << 12;
        seq = flag_bits4(q.x, 1) | flag_bits4(q.y, 1) << 4 | flag_bits4(q.z, 1) << 8 | flag_bits4(q.w, 1) << 12;
    } else {
        for (unsigned i = 0; i < 16u && s0 < n && i < n - s0; i++) { const unsigned f = sflag[s0 + i]; acc |= (f & 1u) << i; seq |= ((f >> 1) & 1u) << i; }
    }
    unsigned before = __shfl_up(acc >> 15, 1, 64);          // slot s0 - 1: the last slot of the lane before, or (first lane of the wave) one byte
    if ((threadIdx.x & 63u) == 0) before = (s0 > 0 && s0 <= n) ? (sflag[s0 - 1] & 1u) : 0u;
    st = acc & (seq | ~((acc << 1) | before)) & 0xffffu;
}
// One block per tile of ORIP_RUN_TILE slots.  Counting pass (LIST = false): tiles[b] = runs that start in the tile << 32 | accepted slots of the tile, and a
// zero behind the last tile; their exclusive scan, in place, is the listing pass's input (LIST = true): rbegin[r] = first slot of run r, rpos[r] = accepted
// slots in front of it, rpos[n_runs] = n_acc.
template <bool LIST>
__global__ __launch_bounds__(256) void k_run_tiles(const uint8_t* __restrict__ sflag, unsigned n, unsigned nb, int64_t* __restrict__ tiles,
                                                    unsigned n_acc, unsigned n_runs, unsigned* __restrict__ rbegin, unsigned* __restrict__ rpos) {
    static_assert(ORIP_RUN_TILE == 256u * 16u, "a lane takes 16 slots of its block's tile");
    __shared__ unsigned wsum[4];
    const unsigned tid = threadIdx.x, s0 = blockIdx.x * ORIP_RUN_TILE + tid * 16u;
    unsigned acc, st;
    run_lane_flags(sflag, n, s0, (reinterpret_cast<uintptr_t>(sflag) & 15u) == 0, acc, st);
    const unsigned mine = (unsigned)__popc(acc) | (unsigned)__popc(st) << 16;      // both sums of a tile are <= 4096: 16 bits each
    unsigned inc = mine;
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(inc, o, 64); if ((int)(tid & 63u) >= o) inc += t; }
    if ((tid & 63u) == 63u) wsum[tid >> 6] = inc;
    __syncthreads();
    if (!LIST) {
        if (tid == 0) { const unsigned t = wsum[0] + wsum[1] + wsum[2] + wsum[3]; tiles[blockIdx.x] = (int64_t)(t >> 16) << 32 | (int64_t)(t & 0xffffu); if (blockIdx.x == 0) tiles[nb] = 0; }
        return;
    }
    unsigned ex = inc - mine;
    for (unsigned w = 0; w < (tid >> 6); w++) ex += wsum[w];
    const int64_t base = tiles[blockIdx.x];
    const unsigned pos0 = (unsigned)(base & 0xffffffffll) + (ex & 0xffffu), run0 = (unsigned)(base >> 32) + (ex >> 16);
    for (unsigned m = st; m; m &= m - 1u) {
        const unsigned i = (unsigned)__ffs((int)m) - 1u, below = (1u << i) - 1u;
        const unsigned r = run0 + (unsigned)__popc(st & below);
        if (r < n_runs) { rbegin[r] = s0 + i; rpos[r] = pos0 + (unsigned)__popc(acc & below); }
    }
    if (blockIdx.x == 0 && tid == 0) rpos[n_runs] = n_acc;
}
// key[r] = 1 << 32 | length for a run of at least min_len slots, else 0, and 0 behind the last run: the exclusive scan, in place, gives a kept run its
// index among the kept runs (high word) and the offset of its points (low word), and behind the last run both totals
__global__ __launch_bounds__(256) void k_run_keys(const unsigned* __restrict__ rpos, unsigned n_runs, unsigned min_len, int64_t* __restrict__ key) {
    const unsigned r = blockIdx.x * 256 + threadIdx.x;
    if (r > n_runs) return;
    const unsigned len = r < n_runs ? rpos[r + 1] - rpos[r] : 0u;
    key[r] = len >= min_len ? ((int64_t)1 << 32 | (int64_t)len) : 0;
}
__global__ __launch_bounds__(256) void k_run_offsets(const unsigned* __restrict__ rbegin, const unsigned* __restrict__ rpos, const int64_t* __restrict__ key, unsigned n_runs, unsigned min_len,
                                                      unsigned n_keep, int64_t* __restrict__ off, unsigned* __restrict__ kbegin) {
    const unsigned r = blockIdx.x * 256 + threadIdx.x;
    if (r > n_runs) return;
    const int64_t v = key[r]; const unsigned k = (unsigned)(v >> 32);
    if (r == n_runs) { if (k == n_keep) off[k] = v & 0xffffffffll; return; }
    if (rpos[r + 1] - rpos[r] < min_len || k >= n_keep) return;
    off[k] = v & 0xffffffffll; kbegin[k] = rbegin[r];
}
// 4096 consecutive output points per block (as k_gather_pts): point j of kept run k is slot kbegin[k] + j of the caller's source
template <class Pts>
__global__ __launch_bounds__(256) void k_run_gather(Pts pts, const unsigned* __restrict__ kbegin, int64_t n, const int64_t* __restrict__ off, int2* __restrict__ dst, int64_t total) {
    const int64_t start = (int64_t)blockIdx.x * 4096;
    if (start >= total) return;
    int64_t k = last_le(off, n, start);
    for (int64_t idx = start + threadIdx.x; idx < min(total, start + 4096); idx += 256) {
        while (off[k + 1] <= idx) k++;           // (kept runs have at least two points: none is empty)
        dst[idx] = pts.at(kbegin[k] + (unsigned)(idx - off[k]));
    }
}
}  // namespace

// Shared by stage 08-A and stage 10 (vec_common.h).  Two host reads: (accepted slots, runs) and (kept runs, their points).
template <class Pts>
int orip_runs_to_polys(orip_ctx* c, Pts pts, const uint8_t* sflag, unsigned n_slots, DPolys& dst) {
    HIPC(c, dst.clear(LN(c).stream));
    if (n_slots == 0) return 0;
    const hipStream_t st = LN(c).stream;
    const unsigned nb = (unsigned)cdiv(n_slots, ORIP_RUN_TILE);
    int64_t* tiles; { Carve L; L.take(tiles, (size_t)nb + 1); HIPC(c, L.commit(LN(c).vtmp[VTL_RUN_STARTS], 64)); }
    hipLaunchKernelGGL(k_run_tiles<false>, dim3(nb), dim3(256), 0, st, sflag, n_slots, nb, tiles, 0u, 0u, (unsigned*)nullptr, (unsigned*)nullptr);
    ORIP_TRY(vscan_excl<int64_t>(c, tiles, tiles, (size_t)nb + 1));
    int64_t sums = 0;
    ORIP_TRY(vread(c, &sums, tiles + nb));
    const unsigned n_acc = (unsigned)(sums & 0xffffffffll), n_runs = (unsigned)(sums >> 32);
    if (n_runs == 0) return 0;
    unsigned *rbegin, *rpos, *kbegin; int64_t* key;
    { Carve L; L.take(key, (size_t)n_runs + 1); L.take(rpos, (size_t)n_runs + 1); L.each(n_runs, rbegin, kbegin); HIPC(c, L.commit(LN(c).vtmp[VTL_TAIL_RUNS], 64)); }
    hipLaunchKernelGGL(k_run_tiles<true>, dim3(nb), dim3(256), 0, st, sflag, n_slots, nb, tiles, n_acc, n_runs, rbegin, rpos);
    hipLaunchKernelGGL(k_run_keys, dim3(cdiv((int64_t)n_runs + 1, 256)), dim3(256), 0, st, rpos, n_runs, 2u, key);
    ORIP_TRY(vscan_excl<int64_t>(c, key, key, (size_t)n_runs + 1));
    int64_t kept = 0;
    ORIP_TRY(vread(c, &kept, key + n_runs));
    const unsigned n_keep = (unsigned)(kept >> 32); const int64_t total = kept & 0xffffffffll;
    if (n_keep == 0) return 0;
    HIPC(c, dst.off.ensure((size_t)(n_keep + 1) * 8 + 64));
    HIPC(c, dst.pts.ensure((size_t)total * 8 + 64));
    dst.n = n_keep; dst.total = total; dst.set_explicit();
    hipLaunchKernelGGL(k_run_offsets, dim3(cdiv((int64_t)n_runs + 1, 256)), dim3(256), 0, st, rbegin, rpos, key, n_runs, 2u, n_keep, dst.off.as<int64_t>(), kbegin);
    hipLaunchKernelGGL(k_run_gather<Pts>, dim3((unsigned)cdiv(total, 4096)), dim3(256), 0, st, pts, kbegin, (int64_t)n_keep, dst.off.as<int64_t>(), reinterpret_cast<int2*>(dst.pts.p), total);
    HIPC(c, hipGetLastError());
    return 0;
}
template int orip_runs_to_polys<SlotPtsI2>(orip_ctx*, SlotPtsI2, const uint8_t*, unsigned, DPolys&);
template int orip_runs_to_polys<SlotPtsF64>(orip_ctx*, SlotPtsF64, const uint8_t*, unsigned, DPolys&);

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
