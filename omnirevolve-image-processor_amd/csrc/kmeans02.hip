// csrc/kmeans02.hip -- the k-means fit of stage 02 (02_color_extract.py 02:46-49) and of process_colors.py on gfx950: cv2.kmeans with
// KMEANS_PP_CENTERS as ONE kernel, k_kmeans_fit_mb, and its entry points.  Samples are u8 triples (Lab or RGB, gathered by
// raster02.hip: orip_raster02_gather), so kmeans++ works on exact integers; the sequential scans of the CPU algorithm are replaced by order-independent
// exact equivalents ("k-means exactness notes").  Float arithmetic mirrors OpenCV's evaluation order: -ffp-contract=off and explicit
// __fmul_rn / __fadd_rn where the order matters.
//
// The fit is spread over KMB_B workgroups with a device-wide barrier (km_grid_sync) between phases; a single workgroup spends 13 ms of pure ALU time on
// one CU at the head of the whole path.  Integer sums are order-free; the only floating-point reduction (compactness) is evaluated by workgroup 0 with
// the fixed tree of a 1024-thread workgroup.
//
// THE BARRIER RULE.  A barrier that one workgroup skips does not fail, it hangs the card.  So every workgroup of a group takes the same path to every
// barrier: km_grid_sync is called only from the top level of a phase function (km_grid_sum is the one helper that holds a call), never under a condition
// on bid, tid or lane, and only under conditions on kernel arguments, loop counters every workgroup shares, and words every workgroup read from G behind
// a barrier (or LDS copies of such words that every workgroup updates alike).  Work of one workgroup or lane stands BETWEEN barriers, in an `if` that holds
// no barrier.  Every phase states its barriers in the comment above it.
#include "orip_ctx.h"
#include <algorithm>

// cv::RNG (multiply with carry)
__device__ __forceinline__ unsigned km_next(unsigned long long& st) {
    st = (unsigned long long)(unsigned)st * 4164903690ULL + (unsigned)(st >> 32);
    return (unsigned)st;
}
__device__ __forceinline__ double km_double(unsigned long long& st) {
    unsigned t = km_next(st);
    unsigned long long v = ((unsigned long long)t << 32) | km_next(st);
    return (double)v * 5.4210108624275221700372640043497e-20;
}

__device__ __forceinline__ int isq3(const u8* a, const u8* b) {
    int d0 = (int)a[0] - b[0], d1 = (int)a[1] - b[1], d2 = (int)a[2] - b[2];
    return d0 * d0 + d1 * d1 + d2 * d2;
}
// hal::normL2Sqr_(sample, centre, 3) in float: s=0; s+=t*t per component
__device__ __forceinline__ float fsq3(const u8* a, const float* c) {
    float s = 0.f;
    for (int j = 0; j < 3; j++) { float t = __fsub_rn((float)a[j], c[j]); s = __fadd_rn(s, __fmul_rn(t, t)); }
    return s;
}

#define KMB_B 64
#define KMB_T 256
// Attempts are independent but for the random draws, and every attempt makes the same number of them (one index, 3 (K - 1) doubles): up to KM_GROUPS groups
// of KMB_B workgroups take the attempts a = group, group + groups, ... side by side (the fit is bound by its grid barriers, not by the card), each with its
// own barrier, accumulators and work arrays; the host takes the first attempt with the smallest compactness, as the sequential loop does (02:46-49).
enum { KM_GROUPS = 4 };
// The barrier spins: it needs every workgroup of the launch resident at once.  A plain launch checks nothing of that; residency comes from the grid size
// alone, at most one workgroup per CU of the card's 256.
static_assert(KMB_B * KM_GROUPS <= 256, "k_kmeans_fit_mb: more workgroups than CUs, the grid barrier would wait for workgroups that cannot start");

struct alignas(16) KmGlobal {                      // (whole 16-byte words: the memset that clears the groups' records is one fill kernel)
    unsigned bar_count, bar_gen;
    long long acc[8][4];                           // rotating accumulators of the integer passes (km_grid_sum), up to three values per pass
    int ci3[4];                                    // the three trial centres of a ++ step
    long long tot[2][ORIP_MAX_LAYERS * 4];         // cluster sums (L, a, b, count), double-buffered by iteration parity
    unsigned long long key;                        // farthest-point search of the empty-cluster repair
    double compact;
    float slow_centers[ORIP_MAX_LAYERS * 3];
    long long blockpart[KMB_B];
};
struct KmResult { float cen[ORIP_MAX_LAYERS * 3]; double compact; int attempt; int status; int pad[2]; };
// static LDS of the kernel, widest alignment first (no padding)
struct KmLds {
    double ptree[1024];                            // compactness tree
    long long tot[ORIP_MAX_LAYERS * 4];            // this iteration's cluster sums, as every workgroup read them from G
    long long red[KMB_T / 64];                     // kmb_block_sum
    double shift;
    int csum[KMB_T / 64][ORIP_MAX_LAYERS * 4];     // per-wave cluster sums
    float centers[ORIP_MAX_LAYERS * 3], old_centers[ORIP_MAX_LAYERS * 3];
    int pp_idx[ORIP_MAX_LAYERS];                   // the samples kmeans++ chose
};
// What a thread is and owns, for one group's fit
struct KmThread {
    int tid, wave, bid, gtid;                      // in the workgroup; workgroup in the group; thread in the group
    int N, K, chunk, lo, hi;                       // thread g owns the samples [g * chunk, (g + 1) * chunk) below N: [lo, hi)
    const u8* data; int32_t* dist; int32_t* labels; double* dd; long long* parts; KmGlobal* G;      // the group's arrays
    KmLds* s;
    unsigned pass;                                 // integer passes so far: selects the accumulator of km_grid_sum
};
enum { KM_GSZ = KMB_B * KMB_T };                   // threads of a group

__device__ __forceinline__ void km_grid_sync(KmGlobal* G) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned gen = atomicAdd(&G->bar_gen, 0u);
        if (atomicAdd(&G->bar_count, 1u) == KMB_B - 1) { atomicExch(&G->bar_count, 0u); __threadfence(); atomicAdd(&G->bar_gen, 1u); }
        else while (atomicAdd(&G->bar_gen, 0u) == gen) __builtin_amdgcn_s_sleep(1);
    }
    __syncthreads();
    __threadfence();
}
__device__ __forceinline__ long long kmb_block_sum(long long v, long long* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = 0;
    for (int w = 0; w < KMB_T / 64; w++) r += red[w];
    return r;
}
// Grid-wide integer sums of NV values per thread.  Barriers: 1.
// Pass p adds into slot p mod 8 and workgroup 0 clears slot p + 4 in front of the barrier.  A slot may be cleared only when nobody reads or adds to it:
// slot p is in use, and slot p - 1 (= p + 7) may still be read by a workgroup that has left barrier p - 1 and not yet loaded its sum.  Slots p + 1 ... p + 6
// are free -- their last readers (pass p - 7 ... p - 2) arrived at barrier p - 1 after reading, which workgroup 0 has left, and their next adders start
// behind barrier p, which workgroup 0 enters after the clear; p + 4 lies in the middle of them.
template <int NV> __device__ __forceinline__ void km_grid_sum(KmThread& t, const long long (&v)[NV], long long (&r)[NV]) {
    long long b[NV];
    for (int j = 0; j < NV; j++) b[j] = kmb_block_sum(v[j], t.s->red);
    const unsigned slot = t.pass & 7u;
    if (t.tid == 0) {
        for (int j = 0; j < NV; j++) atomicAdd((unsigned long long*)&t.G->acc[slot][j], (unsigned long long)b[j]);
        if (t.bid == 0) { const unsigned z = (t.pass + 4u) & 7u; for (int j = 0; j < 3; j++) t.G->acc[z][j] = 0; }
    }
    km_grid_sync(t.G);
    for (int j = 0; j < NV; j++) r[j] = *(volatile long long*)&t.G->acc[slot][j];
    t.pass++;
}

// ---- the prefix descent of a ++ draw (first wave of workgroup 0; no barriers) ----
// Lane index of the first lane whose inclusive prefix base + v[0 .. lane] reaches p as a double, -1: none; `before` = the prefix in front of that lane, or
// base + the whole window when there is none.  Every test is "(double)(inclusive integer prefix) >= p" on exact integers.
__device__ __forceinline__ int km_first_cross(int lane, double p, long long base, long long v, bool valid, long long& before) {
    if (!valid) v = 0;
    long long inc = v;
    for (int o = 1; o < 64; o <<= 1) { long long u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    const unsigned long long m = __ballot(valid && (double)(base + inc) >= p);
    const int f = m ? __ffsll((long long)m) - 1 : -1;
    const int src = f >= 0 ? f : 63;
    const long long incf = __shfl(inc, src, 64), vf = __shfl(v, src, 64);
    before = base + (f >= 0 ? incf - vf : incf);
    return f;
}
// One level: the first index of [begin, end) at which the prefix run + value(begin .. index) reaches p, in windows of 64; -1: none.  `run` moves up to the
// prefix in front of the crossing (all of the level when there is none).
template <class F> __device__ __forceinline__ int km_descend_level(int lane, double p, long long& run, int begin, int end, F value) {
    for (int i0 = begin; i0 < end; i0 += 64) {
        const bool valid = i0 + lane < end;
        long long before;
        const int f = km_first_cross(lane, p, run, valid ? (long long)value(i0 + lane) : 0, valid, before);
        run = before;
        if (f >= 0) return i0 + f;
    }
    return -1;
}
// ci = first sample whose inclusive prefix of dist reaches p, else N - 1: over the workgroups' totals, the threads of the crossing workgroup, the samples
// of the crossing thread's chunk
__device__ __forceinline__ int km_descend(const KmThread& t, double p) {
    long long run = 0;
    const int b = km_descend_level(t.tid, p, run, 0, KMB_B, [&](int i) { return *(volatile long long*)&t.G->blockpart[i]; });
    if (b < 0) return t.N - 1;
    const int g = km_descend_level(t.tid, p, run, b * KMB_T, (b + 1) * KMB_T, [&](int i) { return *(volatile long long*)&t.parts[i]; });
    if (g < 0) return t.N - 1;
    const int l2 = min(t.N, g * t.chunk), h2 = min(t.N, l2 + t.chunk);
    const int ci = km_descend_level(t.tid, p, run, l2, h2, [&](int i) { return t.dist[i]; });
    return ci < 0 ? t.N - 1 : ci;
}

// ---- generateCentersPP ----
// The first centre: one draw, every sample's distance to it.  Returns the sum of the distances.  Barriers: 1.
__device__ __forceinline__ long long km_seed_first(KmThread& t, unsigned long long& rng) {
    if (t.bid == 0 && t.tid < 2 * ORIP_MAX_LAYERS * 4) (&t.G->tot[0][0])[t.tid] = 0;     // both sum buffers start an attempt empty (barriers follow)
    const int c0 = (int)(km_next(rng) % (unsigned)t.N);
    if (t.tid == 0) t.s->pp_idx[0] = c0;
    long long ls[1] = {0}, sum0[1];
    for (int i = t.gtid; i < t.N; i += KM_GSZ) { int d = isq3(t.data + 3 * i, t.data + 3 * c0); t.dist[i] = d; ls[0] += d; }
    km_grid_sum(t, ls, sum0);
    return sum0[0];
}
// Centre k >= 1.  Its three trials (cv::generateCentersPP, 3 trials per centre) share the distances they start from, so they run side by side: ONE pass of
// partial sums, the three descents in one phase, the three candidate sums in one reduction (the fit is barrier-bound: 200 000 samples on 16 384 threads).
// Every thread keeps its own contiguous chunk [lo, hi) from the update of the distances through the partial sums to the candidate sums, so no barrier is
// needed between a centre's update and the next centre's sums.  Same draws in the same order, same integer arithmetic.  Returns the new sum of distances.
// Barriers: 3 (partial sums | descents | candidate sums).
__device__ __forceinline__ long long km_seed_next(KmThread& t, unsigned long long& rng, int k, long long sum0) {
    double pj[3];
    for (int j = 0; j < 3; j++) pj[j] = km_double(rng) * (double)sum0;
    long long cs = 0;
    for (int i = t.lo; i < t.hi; i++) cs += t.dist[i];
    t.parts[t.gtid] = cs;
    const long long bs = kmb_block_sum(cs, t.s->red);
    if (t.tid == 0) t.G->blockpart[t.bid] = bs;
    km_grid_sync(t.G);
    if (t.bid == 0 && t.tid < 64)
        for (int j = 0; j < 3; j++) { const int ci = km_descend(t, pj[j]); if (t.tid == 0) t.G->ci3[j] = ci; }
    km_grid_sync(t.G);
    int cj[3]; for (int j = 0; j < 3; j++) cj[j] = *(volatile int*)&t.G->ci3[j];
    long long sj[3] = {0, 0, 0}, Sj[3];
    for (int i = t.lo; i < t.hi; i++) {
        const int d0 = t.dist[i];
        for (int j = 0; j < 3; j++) sj[j] += min(isq3(t.data + 3 * i, t.data + 3 * cj[j]), d0);
    }
    km_grid_sum(t, sj, Sj);
    long long bestSum = 0x7fffffffffffffffLL; int bestCenter = -1;
    for (int j = 0; j < 3; j++) if (Sj[j] < bestSum) { bestSum = Sj[j]; bestCenter = cj[j]; }
    if (t.tid == 0) t.s->pp_idx[k] = bestCenter;
    if (k + 1 < t.K) for (int i = t.lo; i < t.hi; i++) t.dist[i] = min(isq3(t.data + 3 * i, t.data + 3 * bestCenter), t.dist[i]);      // own chunk: read next by this thread only, then (after a barrier) by the descent
    __syncthreads();
    return bestSum;
}
// Barriers: 1 + 3 (K - 1).
__device__ __forceinline__ void km_seed(KmThread& t, unsigned long long& rng) {
    long long sum0 = km_seed_first(t, rng);
    for (int k = 1; k < t.K; k++) sum0 = km_seed_next(t, rng, k, sum0);
    __syncthreads();
    if (t.tid < t.K * 3) t.s->centers[t.tid] = (float)t.data[3 * t.s->pp_idx[t.tid / 3] + t.tid % 3];
    __syncthreads();
}

// ---- one iteration's new centres ----
// Centre sums from the labels: integer sums per cluster (L, a, b, count) into G->tot[par], read back into LDS by every workgroup; centers = the sums as
// float.  Float accumulation in sample order is exact (== the integer sum) while every partial sum < 2^24; when a sum reaches it, one lane replays the
// literal sequential float32 accumulation.  Barriers: 1, +1 when the replay runs (decided from the totals every workgroup read).
__device__ __forceinline__ void km_update(KmThread& t, int par) {
    KmLds& s = *t.s;
    for (int i = t.tid; i < (KMB_T / 64) * ORIP_MAX_LAYERS * 4; i += KMB_T) (&s.csum[0][0])[i] = 0;
    __syncthreads();
    for (int i = t.gtid; i < t.N; i += KM_GSZ) {
        int k = t.labels[i];
        atomicAdd(&s.csum[t.wave][k * 4 + 0], (int)t.data[3 * i]);
        atomicAdd(&s.csum[t.wave][k * 4 + 1], (int)t.data[3 * i + 1]);
        atomicAdd(&s.csum[t.wave][k * 4 + 2], (int)t.data[3 * i + 2]);
        atomicAdd(&s.csum[t.wave][k * 4 + 3], 1);
    }
    __syncthreads();
    if (t.tid < t.K * 4) {
        long long v = 0; for (int w = 0; w < KMB_T / 64; w++) v += s.csum[w][t.tid];
        atomicAdd((unsigned long long*)&t.G->tot[par][t.tid], (unsigned long long)v);
        if (t.bid == 0) t.G->tot[par ^ 1][t.tid] = 0;        // the other buffer was last read two barriers ago
    }
    if (t.bid == 0 && t.tid == 0) t.G->key = 0;                // for km_repair
    km_grid_sync(t.G);
    if (t.tid < t.K * 4) s.tot[t.tid] = *(volatile long long*)&t.G->tot[par][t.tid];
    __syncthreads();
    bool bad = false;
    for (int k = 0; k < t.K; k++) for (int j = 0; j < 3; j++) if (s.tot[k * 4 + j] >= (1LL << 24)) bad = true;
    if (bad) {
        if (t.bid == 0 && t.tid == 0) {
            float acc[ORIP_MAX_LAYERS * 3];
            for (int q = 0; q < t.K * 3; q++) acc[q] = 0.f;
            for (int i = 0; i < t.N; i++) { int k = t.labels[i]; for (int j = 0; j < 3; j++) acc[k * 3 + j] = __fadd_rn(acc[k * 3 + j], (float)t.data[3 * i + j]); }
            for (int q = 0; q < t.K * 3; q++) t.G->slow_centers[q] = acc[q];
        }
        km_grid_sync(t.G);
        if (t.tid < t.K * 3) s.centers[t.tid] = *(volatile float*)&t.G->slow_centers[t.tid];
    } else if (t.tid < t.K * 3) s.centers[t.tid] = (float)s.tot[(t.tid / 3) * 4 + t.tid % 3];
    __syncthreads();
}
// Empty-cluster repair, sequential over k as the reference: an empty cluster takes the point of the largest cluster that lies farthest from that
// cluster's centre.  s.tot is the same in every workgroup (read behind km_update's barrier, then changed by every workgroup's thread 0 alike), so every
// workgroup repairs the same clusters.  Barriers: 3 per empty cluster (farthest point | everybody has read the key | key cleared).
__device__ __forceinline__ void km_repair(KmThread& t) {
    KmLds& s = *t.s;
    for (int k = 0; k < t.K; k++) {
        if (s.tot[k * 4 + 3] != 0) continue;
        int max_k = 0;
        for (int k1 = 1; k1 < t.K; k1++) if (s.tot[max_k * 4 + 3] < s.tot[k1 * 4 + 3]) max_k = k1;
        float nb[3]; float scale = 1.f / (float)s.tot[max_k * 4 + 3];
        for (int j = 0; j < 3; j++) nb[j] = __fmul_rn(s.centers[max_k * 3 + j], scale);
        // farthest point: max_dist <= dist  => last index among maxima
        unsigned long long key = 0;
        for (int i = t.gtid; i < t.N; i += KM_GSZ) {
            if (t.labels[i] != max_k) continue;
            float d = fsq3(t.data + 3 * i, nb);
            unsigned long long kk = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
            if (kk >= key) key = kk;
        }
        atomicMax(&t.G->key, key);
        km_grid_sync(t.G);
        const int far_i = (int)(*(volatile unsigned long long*)&t.G->key & 0xffffffffu);
        __syncthreads();
        if (t.tid == 0) {
            s.tot[max_k * 4 + 3]--; s.tot[k * 4 + 3]++;
            if (t.bid == 0) t.labels[far_i] = k;
            for (int j = 0; j < 3; j++) {
                float v = (float)t.data[3 * far_i + j];
                s.centers[max_k * 3 + j] = __fsub_rn(s.centers[max_k * 3 + j], v);
                s.centers[k * 3 + j] = __fadd_rn(s.centers[k * 3 + j], v);
            }
        }
        km_grid_sync(t.G);
        if (t.bid == 0 && t.tid == 0) t.G->key = 0;
        km_grid_sync(t.G);
    }
}
// Sums -> means; returns the largest squared shift of a centre against the iteration before.  No barriers.
__device__ __forceinline__ double km_scale_shift(KmThread& t) {
    KmLds& s = *t.s;
    if (t.tid == 0) {
        double max_shift = 0.0;
        for (int k = 0; k < t.K; k++) {
            float scale = 1.f / (float)s.tot[k * 4 + 3];
            for (int j = 0; j < 3; j++) s.centers[k * 3 + j] = __fmul_rn(s.centers[k * 3 + j], scale);
            double d = 0;
            for (int j = 0; j < 3; j++) { double u = (double)__fsub_rn(s.centers[k * 3 + j], s.old_centers[k * 3 + j]); d = __dadd_rn(d, __dmul_rn(u, u)); }
            max_shift = fmax(max_shift, d);
        }
        s.shift = max_shift;
    }
    __syncthreads();
    const double r = s.shift;
    __syncthreads();
    return r;
}
// Every sample to its nearest centre (the first among equals).  Barriers: 1.
__device__ __forceinline__ void km_assign(KmThread& t) {
    for (int i = t.gtid; i < t.N; i += KM_GSZ) {
        float md = 0.f; int kb = 0;
        for (int k = 0; k < t.K; k++) { float d = fsq3(t.data + 3 * i, &t.s->centers[3 * k]); if (k == 0 || md > d) { md = d; kb = k; } }
        t.labels[i] = kb;
    }
    km_grid_sync(t.G);
}
// The last iteration: the distance of every sample to its centre, summed by workgroup 0 in the reduction tree of a 1024-thread workgroup (strided
// partials, shfl_down tree per 64, then 16 sequential adds).  Barriers: 2 (the terms | the sum).
__device__ __forceinline__ double km_compactness(KmThread& t) {
    KmLds& s = *t.s;
    for (int i = t.gtid; i < t.N; i += KM_GSZ) t.dd[i] = (double)fsq3(t.data + 3 * i, &s.centers[3 * t.labels[i]]);
    km_grid_sync(t.G);
    if (t.bid == 0) {
        for (int v = t.tid; v < 1024; v += KMB_T) { double r = 0; for (int i = v; i < t.N; i += 1024) r += t.dd[i]; s.ptree[v] = r; }
        __syncthreads();
        for (int o = 32; o > 0; o >>= 1) {
            for (int q = t.tid; q < 16 * o; q += KMB_T) { const int w = q / o, l = q % o; s.ptree[w * 64 + l] += s.ptree[w * 64 + l + o]; }
            __syncthreads();
        }
        if (t.tid == 0) { double r = 0; for (int w = 0; w < 16; w++) r += s.ptree[w * 64]; t.G->compact = r; }
    }
    km_grid_sync(t.G);
    return *(volatile double*)&t.G->compact;
}

// The loop of cv::kmeans.  Workgroup blockIdx.x is workgroup bid of group grp; `attempts`, `groups`, K, maxCount and epsilon are the same for all.
__global__ __launch_bounds__(KMB_T) void k_kmeans_fit_mb(const u8* __restrict__ data, int N, int K, int attempts, int groups, int maxCount, double epsilon,
                                                          int32_t* __restrict__ dist_all, int32_t* __restrict__ labels_all,
                                                          double* __restrict__ dd_all, long long* __restrict__ parts_all, KmResult* __restrict__ res_all, KmGlobal* __restrict__ G_all) {
    __shared__ KmLds s;
    const int grp = blockIdx.x / KMB_B;
    KmThread t;
    t.tid = threadIdx.x; t.wave = t.tid >> 6; t.bid = blockIdx.x % KMB_B; t.gtid = t.bid * KMB_T + t.tid;
    t.N = N; t.K = K; t.chunk = (N + KM_GSZ - 1) / KM_GSZ; t.lo = min(N, t.gtid * t.chunk); t.hi = min(N, t.lo + t.chunk);
    t.data = data; t.dist = dist_all + (size_t)grp * N; t.labels = labels_all + (size_t)grp * N;
    t.dd = dd_all + (size_t)grp * N; t.parts = parts_all + (size_t)grp * KM_GSZ; t.G = G_all + grp;
    t.s = &s; t.pass = 0;
    KmResult* res = res_all + grp;
    unsigned long long rng = 0xffffffffULL;   // identical in every thread
    double best_compact = 1.79769313486231570815e+308; int best_attempt = -1;
    for (int a = 0; a < attempts; a++) {
        if (a % groups != grp) { for (int q = 0; q < 1 + 6 * (K - 1); q++) km_next(rng); continue; }      // another group's attempt: its draws
        double compactness = 0;
        for (int iter = 0;;) {
            double max_shift = 1.79769313486231570815e+308;
            __syncthreads();
            if (t.tid < K * 3) { float v = s.centers[t.tid]; s.centers[t.tid] = s.old_centers[t.tid]; s.old_centers[t.tid] = v; }
            __syncthreads();
            if (iter == 0) km_seed(t, rng);
            else { km_update(t, iter & 1); km_repair(t); max_shift = km_scale_shift(t); }
            ++iter;
            if (iter == max(maxCount, 2) || max_shift <= epsilon) { compactness = km_compactness(t); break; }
            km_assign(t);
        }
        if (compactness < best_compact) {
            best_compact = compactness; best_attempt = a;
            if (t.bid == 0 && t.tid < K * 3) res->cen[t.tid] = s.centers[t.tid];
        }
        __syncthreads();
    }
    if (t.bid == 0 && t.tid == 0) { res->compact = best_compact; res->attempt = best_attempt; res->status = 0; }
}

// ------------------------------------------------------------------------------------------------
// host entry points
// ------------------------------------------------------------------------------------------------
static int kmeans_fit_impl(orip_ctx* c, bool rgb, const int64_t* sample_idx, int64_t n_idx, int K, int attempts, int max_iter, double eps,
                           float* centers_out, double* compactness_out) {
    orip_enter(c);
    c->mask_bits = nullptr;
    if (!c->image.p) ORIP_FAIL(c, "no image set");
    if (K < 1 || K > ORIP_MAX_LAYERS) ORIP_FAIL(c, "K=%d out of range 1..%d", K, ORIP_MAX_LAYERS);
    ORIP_TRY(orip_contours_invalidate(c));       // (the sample indices of the upload path go to tmpC)
    const int64_t npx = (int64_t)c->H * c->W;
    const bool resident = !sample_idx && n_idx == -1;      // the set orip_kmeans_samples left in the context
    if (resident && (c->km_n == 0 || c->km_npx != npx))
        ORIP_FAIL(c, "no resident sample set for this image: the set holds %lld indices made for %lld pixels, the image has %lld pixels (orip_kmeans_samples)",
                  (long long)c->km_n, (long long)c->km_npx, (long long)npx);
    int64_t N = resident ? c->km_n : (sample_idx ? n_idx : npx);
    if (N < K || N > 0x7fffffff) ORIP_FAIL(c, "bad sample count %lld", (long long)N);
    HIPC(c, c->tmpB.ensure((size_t)N * 3 + 16));
    if (sample_idx) { HIPC(c, c->tmpC.ensure((size_t)N * 8)); HIPC(c, hipMemcpyAsync(c->tmpC.p, sample_idx, (size_t)N * 8, hipMemcpyHostToDevice, LN(c).stream)); }
    const int64_t* d_idx = resident ? c->km_idx.as<int64_t>() : (sample_idx ? c->tmpC.as<int64_t>() : nullptr);
    if (rgb) orip_raster02_gather(c, true, d_idx, N, c->tmpB.as<u8>());
    else { ProfScope ps(c, "k_lab_gather"); orip_raster02_gather(c, false, d_idx, N, c->tmpB.as<u8>()); }
    HIPC(c, c->tmpD.ensure((size_t)N * 4 * 4 + 256));     // (later stages find tmpD at least this large)
    attempts = std::max(attempts, 1);
    double epsilon = std::max(eps, 0.0); epsilon *= epsilon;
    int maxCount = std::min(std::max(max_iter, 2), 100);
    if (K == 1) { attempts = 1; maxCount = 2; }
    const int groups = std::min(attempts, (int)KM_GROUPS);
    const size_t NG = (size_t)N * groups;
    int32_t *dist, *labels; double* dd; long long* parts; KmGlobal* G; KmResult* res;
    Carve LD; LD.each(NG, dist, labels); HIPC(c, LD.commit(c->tmpD, 256));
    Carve LA; LA.take(dd, NG); LA.take(parts, (size_t)KM_GSZ * groups); LA.take(G, groups); LA.take(res, groups); HIPC(c, LA.commit(c->tmpA, 256));
    HIPC(c, hipMemsetAsync(G, 0, sizeof(KmGlobal) * groups, LN(c).stream));
    HIPC(c, hipMemsetAsync(res, 0xff, sizeof(KmResult) * groups, LN(c).stream));
    {
        ProfScope ps(c, "k_kmeans_fit");
        hipLaunchKernelGGL(k_kmeans_fit_mb, dim3(KMB_B * groups), dim3(KMB_T), 0, LN(c).stream, c->tmpB.as<u8>(), (int)N, K, attempts, groups, maxCount, epsilon,
                           dist, labels, dd, parts, res, G);
    }
    HIPC(c, hipGetLastError());
    KmResult hr[KM_GROUPS];
    HIPC(c, hipMemcpyAsync(hr, res, sizeof(KmResult) * groups, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    int bg = -1;
    for (int g = 0; g < groups; g++) {
        if (hr[g].status != 0) ORIP_FAIL(c, "kmeans kernel did not complete (group %d, status %d)", g, hr[g].status);
        if (bg < 0 || hr[g].compact < hr[bg].compact || (hr[g].compact == hr[bg].compact && hr[g].attempt < hr[bg].attempt)) bg = g;
    }
    memcpy(centers_out, hr[bg].cen, sizeof(float) * K * 3);
    if (compactness_out) *compactness_out = hr[bg].compact;
    return 0;
}

// The subsample of 02:39-44 depends on the pixel count and a fixed seed alone: a resident chain uploads it once and every later fit of an image of that
// size gathers through the context's copy (the set's lifetime: orip_ctx.h).  Synchronised, so the caller's array is free on return.
extern "C" int orip_kmeans_samples(orip_ctx* c, const int64_t* sample_idx, int64_t n_idx) {
    orip_enter(c);
    c->km_n = 0; c->km_npx = 0;
    if (!sample_idx) return 0;
    if (!c->image.p) ORIP_FAIL(c, "no image set");
    const int64_t npx = (int64_t)c->H * c->W;
    if (n_idx < 1 || n_idx > 0x7fffffff) ORIP_FAIL(c, "bad sample count %lld", (long long)n_idx);
    for (int64_t i = 0; i < n_idx; i++)
        if (sample_idx[i] < 0 || sample_idx[i] >= npx) ORIP_FAIL(c, "sample %lld is pixel %lld of %lld", (long long)i, (long long)sample_idx[i], (long long)npx);
    HIPC(c, c->km_idx.ensure((size_t)n_idx * 8));
    HIPC(c, hipMemcpyAsync(c->km_idx.p, sample_idx, (size_t)n_idx * 8, hipMemcpyHostToDevice, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    c->km_n = n_idx; c->km_npx = npx;
    return 0;
}
extern "C" int orip_kmeans_samples_info(orip_ctx* c, int64_t* n_idx, int64_t* n_pixels) {
    orip_enter(c);
    if (n_idx) *n_idx = c->km_n;
    if (n_pixels) *n_pixels = c->km_npx;
    return 0;
}

extern "C" int orip_kmeans_fit(orip_ctx* c, const int64_t* sample_idx, int64_t n_idx, int K, int attempts, int max_iter, double eps,
                               float* centers_out, double* compactness_out) {
    return kmeans_fit_impl(c, false, sample_idx, n_idx, K, attempts, max_iter, eps, centers_out, compactness_out);
}
extern "C" int orip_kmeans_fit_rgb(orip_ctx* c, const int64_t* sample_idx, int64_t n_idx, int K, int attempts, int max_iter, double eps,
                                   float* centers_out, double* compactness_out) {
    return kmeans_fit_impl(c, true, sample_idx, n_idx, K, attempts, max_iter, eps, centers_out, compactness_out);
}
