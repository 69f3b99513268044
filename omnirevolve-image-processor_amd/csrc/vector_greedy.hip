// csrc/vector_greedy.hip -- the greedy nearest-neighbour order of stages 07, 08 and 10 (vec_common.h: vreorder): seed and coordinate-range flags, the
// brute-force kernel over a global-memory or an LDS store, the grid-pruned lone-wave kernel with its asm step, and the gather of the ordered list.
#include "vec_common.h"

namespace {
// ---- greedy nearest-neighbour ordering (07:55-79 / 08:223-248 / 10:69-97), one 1024-thread block per list ----
// rule07: closed contours are entered at their start only and the cursor returns to their start (07:60-62, 80-83).
struct NNEnds { int32_t sx, sy, ex, ey; uint8_t closed; };
__device__ __forceinline__ float nn_d2(int32_t ax, int32_t ay, int32_t bx, int32_t by) {
    float dx = __fsub_rn((float)ax, (float)bx), dy = __fsub_rn((float)ay, (float)by);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}
// The coordinate-range flags of a list's end points (k_argmax_feat writes them next to the seed).  Some coordinate beyond int16: no LDS store (signed
// shorts); beyond 15 bits: no grid kernel (its packed words keep bit 15 for flags).
enum : int { NN_BEYOND_I16 = 1, NN_BEYOND_15BIT = 2 };
// sel[0] = seed polyline, sel[1] = coordinate-range flags (both written on the device just before: the host does not wait for them).  The candidates
// are all enqueued and each decides from sel[1] whether it is the one that runs: (flags & skip_if) != 0 -> not this one; need_any != 0 &&
// (flags & need_any) == 0 -> not this one either.
#define ORIP_NN_GATE(sel, skip_if, need_any) const int fl_ = (sel)[1]; if ((fl_ & (skip_if)) != 0 || ((need_any) != 0 && (fl_ & (need_any)) == 0)) return; const int seed = (sel)[0];
// Reading direction and next cursor of the polyline a step takes, from the squared distances of its start (ds) and end (de) to the cursor.  cl: closed
// under rule07 -- entered at its start only, and the cursor returns to its start.  Otherwise it is read backwards exactly when its end is strictly nearer
// (07:67-70), and the cursor moves to the far end.  Returns true when the next cursor is the polyline's START.
__device__ __forceinline__ bool nn_direction(bool cl, float ds, float de, bool& flip) { flip = cl ? false : !(ds <= de); return cl || flip; }
// Where the brute-force kernel keeps its candidates.  A store is initialised from `ends` (init(i, seed) by the thread that owns i, in front of the first
// barrier), gives candidate i (load) and marks it used (mark_used, thread 0 between two barriers).
struct NNCand { int32_t sx, sy, ex, ey; bool cl, used; };      // cl: closed under rule07
// global memory: the NNEnds array as it is and a used byte per polyline.  Any n, any coordinates; loops strided by blockDim.x (launched with 256 or 1024 threads)
struct NNStoreGlobal {
    static constexpr int THREADS = 0;                                // 0: blockDim.x
    const NNEnds* ends; uint8_t* used; int rule07;
    __device__ __forceinline__ NNStoreGlobal(const NNEnds* e, int, int r07, uint8_t* u) : ends(e), used(u), rule07(r07) {}
    __device__ __forceinline__ void init(int i, int seed) { used[i] = (i == seed); }
    __device__ __forceinline__ NNCand load(int i) const {           // (the end points of unused polylines only)
        NNCand q; q.used = used[i] != 0; if (q.used) return q;
        const NNEnds e = ends[i]; q.sx = e.sx; q.sy = e.sy; q.ex = e.ex; q.ey = e.ey; q.cl = rule07 && e.closed;
        return q;
    }
    __device__ __forceinline__ void mark_used(int i) { used[i] = 1; }
};
// LDS: end points as int16 quads + a state byte per polyline (n <= 16000, coordinates within int16; 1024 threads), so a greedy step costs two barriers and a
// few LDS reads instead of global-memory round trips
struct NNStoreLds {
    static constexpr int THREADS = 1024;
    const NNEnds* ends; short4* P; uint8_t* stt; int rule07;         // P: (sx, sy, ex, ey); stt: bit0 used, bit1 closed under rule07
    __device__ __forceinline__ NNStoreLds(const NNEnds* e, int n, int r07, uint8_t*) : ends(e), rule07(r07) {
        extern __shared__ __align__(16) unsigned char smem[];
        P = reinterpret_cast<short4*>(smem); stt = smem + (size_t)n * sizeof(short4);
    }
    __device__ __forceinline__ void init(int i, int seed) {
        const NNEnds e = ends[i];
        P[i] = make_short4((short)e.sx, (short)e.sy, (short)e.ex, (short)e.ey);
        stt[i] = (uint8_t)((i == seed ? 1 : 0) | ((rule07 && e.closed) ? 2 : 0));
    }
    __device__ __forceinline__ NNCand load(int i) const {
        const uint8_t f = stt[i]; NNCand q; q.used = (f & 1) != 0; if (q.used) return q;
        const short4 e = P[i]; q.sx = e.x; q.sy = e.y; q.ex = e.z; q.ey = e.w; q.cl = (f & 2) != 0;
        return q;
    }
    __device__ __forceinline__ void mark_used(int i) { stt[i] |= 1; }
};
// The brute-force order: every step all threads scan the unused candidates for the smallest (squared distance pattern, index) and thread 0 takes it.
// `used`: the global store's flags (scratch of n bytes); the LDS store wants (size_t)n * 9 bytes of dynamic LDS instead.
template <class Store>
__global__ __launch_bounds__(1024) void k_greedy_nn(const NNEnds* __restrict__ ends, int n, const int* __restrict__ sel, int skip_if, int need_any, int rule07, uint8_t* __restrict__ used,
                                                     int32_t* __restrict__ order, uint8_t* __restrict__ flips) {
    ORIP_NN_GATE(sel, skip_if, need_any)
    __shared__ unsigned long long wbest[16];
    __shared__ int cxs, cys;
    Store st(ends, n, rule07, used);
    const int tid = threadIdx.x, nthreads = Store::THREADS ? Store::THREADS : (int)blockDim.x;
    for (int i = tid; i < n; i += nthreads) st.init(i, seed);
    if (tid == 0) {
        order[0] = seed; flips[0] = 0;
        NNEnds e = ends[seed];
        if (rule07 && e.closed) { cxs = e.sx; cys = e.sy; } else { cxs = e.ex; cys = e.ey; }
    }
    __syncthreads();
    for (int step = 1; step < n; step++) {
        const int cx = cxs, cy = cys;
        unsigned long long best = ~0ULL;
        for (int i = tid; i < n; i += nthreads) {
            const NNCand e = st.load(i);
            if (e.used) continue;
            float ds = nn_d2(e.sx, e.sy, cx, cy);
            float v = ds;
            if (!e.cl) { float de = nn_d2(e.ex, e.ey, cx, cy); if (!(ds <= de)) v = de; }
            unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)i;
            if (key < best) best = key;
        }
        for (int o = 32; o > 0; o >>= 1) { unsigned long long t = __shfl_down(best, o, 64); if (t < best) best = t; }
        if ((tid & 63) == 0) wbest[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
            unsigned long long b = wbest[0];
            for (int w = 1; w < (nthreads >> 6); w++) if (wbest[w] < b) b = wbest[w];
            int bi = (int)(b & 0xffffffffu);
            const NNCand e = st.load(bi);                          // (unused: it has just won)
            float ds = nn_d2(e.sx, e.sy, cx, cy), de = nn_d2(e.ex, e.ey, cx, cy);
            bool flip; const bool to_start = nn_direction(e.cl, ds, de, flip);
            st.mark_used(bi); order[step] = bi; flips[step] = flip ? 1 : 0;
            if (to_start) { cxs = e.sx; cys = e.sy; } else { cxs = e.ex; cys = e.ey; }
        }
        __syncthreads();
    }
}

// order/flip -> descriptors over a source list
__global__ __launch_bounds__(256) void k_desc_from_order(const int64_t* __restrict__ off, const int32_t* __restrict__ order, const uint8_t* __restrict__ flips,
                                                          int64_t n, int open_view, const PolyFeat* __restrict__ feat, GatherDesc* __restrict__ d) {
    int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    int i = order ? order[k] : (int)k;
    GatherDesc g; g.begin = off[i]; g.len = open_view ? feat[i].n : (off[i + 1] - off[i]); g.rev = flips ? flips[k] : 0; g.src = i;
    d[k] = g;
}

// argmax with first-max tie-break over a float / double field of PolyFeat (seed of the greedy orders); tiny: single block
// (one 256-thread block: a 1024-thread block waits for a CU with sixteen free wave slots -- half a millisecond next to the other layers' work, in front of the greedy chain)
__global__ __launch_bounds__(256) void k_argmax_feat(const PolyFeat* __restrict__ f, int n, int use_arc, int* __restrict__ out, const NNEnds* __restrict__ e = nullptr) {
    __shared__ double bv[256]; __shared__ int bi[256];
    __shared__ int bad_s;
    if (threadIdx.x == 0) bad_s = 0;
    __syncthreads();
    double v = -1.0; int idx = 0x7fffffff; int bad = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        double x = use_arc ? f[i].arc : (double)f[i].per; if (x > v) { v = x; idx = i; }
        if (e) {      // the coordinate-range flags of the greedy kernels in the same pass: out[1]
            const NNEnds q = e[i];
            auto outside = [&](int lo, int hi) { return q.sx < lo || q.sx > hi || q.sy < lo || q.sy > hi || q.ex < lo || q.ex > hi || q.ey < lo || q.ey > hi; };
            if (outside(-32768, 32767)) bad |= NN_BEYOND_I16;
            if (outside(-16384, 16383)) bad |= NN_BEYOND_15BIT;
        }
    }
    if (bad) atomicOr(&bad_s, bad);
    bv[threadIdx.x] = v; bi[threadIdx.x] = idx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            double o = bv[threadIdx.x + s]; int oi = bi[threadIdx.x + s];
            if (o > bv[threadIdx.x] || (o == bv[threadIdx.x] && oi < bi[threadIdx.x])) { bv[threadIdx.x] = o; bi[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { *out = bi[0]; if (e) out[1] = bad_s; }
}
template <class Src>
__global__ __launch_bounds__(256) void k_ends_from_feat(const PolyFeat* __restrict__ f, int64_t n, int rule07, Src src, NNEnds* __restrict__ e) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    NNEnds q; q.sx = f[i].sx; q.sy = f[i].sy; q.ex = f[i].ex; q.ey = f[i].ey; q.closed = f[i].closed;
    if (rule07 && f[i].closed) {   // _ends (07:12-17): a closed contour ends at its second-to-last point
        int64_t m = src.len(i);
        if (m > 1) { const int2 p = src.cur(i).at(m - 2); q.ex = p.x; q.ey = p.y; }
    }
    e[i] = q;
}

// ---- the common step of k_greedy_nn_fast as ONE asm statement that runs step after step (r03).
// The compiled step is ~260 instructions on its usual path and stalls a dozen times on scalar instructions that consume vector results (cell
// ranges read out lane by lane, the gap test, the winner's end points): 1 750 cycles.  The usual path is narrow -- the 3x3 window away from the
// first / last cell row, 1..128 candidates, a unique nearest one that passes the gap test (94 % of the steps of the bench image) -- and this
// loop takes exactly that path in ~100 instructions: the six range words are read out back to back (one stall), the gap threshold is
// computed while the LDS reads are in flight, validity / used flags are vector selects, every lane settles reading direction and next cursor
// of its own candidate, the winner lane itself writes the used flag (exec = the one-bit tie mask), the result leaves through v_writelane.
// Anything else (empty or crowded window, a tie, a failed gap test, the border rows) leaves the loop BEFORE the step has changed anything;
// the caller then takes that one step with the compiled code.  Same arithmetic as the compiled step (unfused float ops, the same integer test).
// Returns 0: step == n; 1: 64 results are in `ringv` (step is a multiple of 64); 2..7: the step at `step` is the caller's (the reason: see the exits).
__device__ __forceinline__ int nn_asm_steps(int& cx, int& cy, int& step, unsigned& ringv, int n, int sh, int G, unsigned lds_p, unsigned lds_cst, unsigned lds_eid,
                                            unsigned n_ent_m1, int rowoff, int isend, int lane, int& dbg_cnt) {
    int ev; int s_cnt = 0;
    int s_cx = __builtin_amdgcn_readfirstlane(cx), s_cy = __builtin_amdgcn_readfirstlane(cy), s_step = __builtin_amdgcn_readfirstlane(step);
    const int s_n = __builtin_amdgcn_readfirstlane(n), s_sh = __builtin_amdgcn_readfirstlane(sh), s_G = __builtin_amdgcn_readfirstlane(G), s_Gm1 = s_G - 1;
    const unsigned s_p = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_p), s_cst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_cst),
                   s_eid = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_eid), s_nem1 = (unsigned)__builtin_amdgcn_readfirstlane((int)n_ent_m1);
    // ordinal T inside the window -> byte address Q of its entry (clamped into the table): row 0 holds the ordinals [0, n0), row 1 [n0, n01), row 2 the rest
#define ORIP_NN_Q(T, Q, TMP1, TMP2)                                                                                    \
        "v_cmp_gt_u32_e64 s[94:95], s73, " T "\n\t"                 /* (a vector compare's SGPR result is read two instructions later at the earliest) */ \
        "v_cmp_gt_u32 vcc, s68, " T "\n\t"                                                                             \
        "v_add_u32 " Q ", s67, " T "\n\t"                                                                              \
        "v_add_u32 " TMP1 ", s75, " T "\n\t"                                                                           \
        "v_add_u32 " TMP2 ", s76, " T "\n\t"                                                                           \
        "v_cndmask_b32_e64 " TMP1 ", " TMP2 ", " TMP1 ", s[94:95]\n\t"                                                 \
        "v_cndmask_b32 " Q ", " TMP1 ", " Q ", vcc\n\t"                                                                \
        "v_min_u32 " Q ", %[nem1], " Q "\n\t"                                                                          \
        "v_lshl_add_u32 " Q ", " Q ", 1, %[eidb]\n\t"
    // entry word IDW (index << 1 | end) -> its end bit, the address PA of the polyline's end points, and their read into v[E0:E1] issued
#define ORIP_NN_FETCH(IDW, ENDBIT, PA, E0, E1)                                                                         \
        "v_lshrrev_b32 v50, 1, " IDW "\n\t"                                                                            \
        "v_lshl_add_u32 " PA ", v50, 3, %[pb]\n\t"                                                                     \
        "ds_read_b64 v[" E0 ":" E1 "], " PA "\n\t"                                                                     \
        "v_and_b32 " ENDBIT ", 1, " IDW "\n\t"
    // key K of the candidate (squared distance pattern of the entry's end point; ~0 when the polyline is used or the ordinal lies beyond the window)
#define ORIP_NN_KEY(ENDBIT, K, E0, E1, VALID)                                                                          \
        "v_cmp_eq_u32_e64 s[94:95], 0, " ENDBIT "\n\t"                                                                 \
        "v_and_b32 v54, 0x7fff7fff, v" E0 "\n\t"                                                                       \
        "v_and_b32 v55, 0x8000, v" E0 "\n\t"                                                                           \
        "v_cndmask_b32_e64 v50, v" E1 ", v54, s[94:95]\n\t"                                                            \
        "v_cvt_f32_u32_sdwa v56, v50 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n\t"                          \
        "v_cvt_f32_u32_sdwa v57, v50 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t"                          \
        "v_sub_f32 v56, v56, v40\n\t"                                                                                  \
        "v_sub_f32 v57, v57, v41\n\t"                                                                                  \
        "v_mul_f32 v56, v56, v56\n\t"                                                                                  \
        "v_mul_f32 v57, v57, v57\n\t"                                                                                  \
        "v_add_f32 " K ", v56, v57\n\t"                                                                                \
        "v_cmp_eq_u32 vcc, 0, v55\n\t"                                                                                 \
        "v_cndmask_b32 " K ", -1, " K ", vcc\n\t"                                                                      \
        "v_cndmask_b32_e64 " K ", -1, " K ", " VALID "\n\t"
    // (entry word, K) in v[IK0:IK1], end points v[E0:E1], address PA: better than the best so far (v[58:59], v[52:53], v51)?  Smaller key, then smaller entry word.
#define ORIP_NN_MERGE(IK0, IK1, E0, E1, PA)                                                                            \
        "v_cmp_lt_u64 vcc, v[" IK0 ":" IK1 "], v[58:59]\n\t"                                                           \
        "v_cndmask_b32 v58, v58, v" IK0 ", vcc\n\t"                                                                    \
        "v_cndmask_b32 v59, v59, v" IK1 ", vcc\n\t"                                                                    \
        "v_cndmask_b32 v52, v52, v" E0 ", vcc\n\t"                                                                     \
        "v_cndmask_b32 v53, v53, v" E1 ", vcc\n\t"                                                                     \
        "v_cndmask_b32 v51, v51, " PA ", vcc\n\t"
    // minimum of v47 over the wave into lane 63 (the compiler's sequence for the same reduction; a DPP source is read two instructions after it was written)
#define ORIP_NN_MIN6                                                                                                   \
        "s_nop 1\n\t"                                                                                                  \
        "v_min_u32_dpp v47, v47, v47 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"                                         \
        "s_nop 1\n\t"                                                                                                  \
        "v_min_u32_dpp v47, v47, v47 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"                                         \
        "s_nop 1\n\t"                                                                                                  \
        "v_min_u32_dpp v47, v47, v47 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"                                         \
        "s_nop 1\n\t"                                                                                                  \
        "v_min_u32_dpp v47, v47, v47 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"                                         \
        "s_nop 1\n\t"                                                                                                  \
        "v_min_u32_dpp v47, v47, v47 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"                                      \
        "s_nop 1\n\t"                                                                                                  \
        "v_min_u32_dpp v47, v47, v47 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"                                      \
        "s_nop 1\n\t"
    asm volatile(
        "s_mov_b32 s89, m0\n\t"
        "s_and_b32 m0, %[step], 63\n\t"
        "s_lshl_b32 s87, 1, %[sh]\n\t"                              // cell
        "s_add_i32 s88, s87, -1\n\t"                                // cell - 1
        "s_add_i32 s79, s87, 1\n\t"
        "s_mul_i32 s59, s79, s79\n\t"
        "s_lshr_b32 s80, s59, 18\n\t"
        "s_sub_i32 s59, s59, s80\n\t"
        "s_add_i32 s59, s59, -1\n\t"                              // the gap test's threshold for the smallest gap a 3x3 window can have (cell + 1)
        "s_mov_b32 s81, -1\n\t"                                     // cell the range words in s67 .. s76 belong to: none yet
        "s_mov_b32 s58, 0\n\t"                                      // 1: the lanes hold the candidates of that cell's window (v45, v49, v51, v[52:53], s[92:93])
        "v_cvt_f32_i32 v40, %[cx]\n\t"
        "v_cvt_f32_i32 v41, %[cy]\n\t"
        "L_step%=:\n\t"
        "s_lshr_b32 s60, %[cx], %[sh]\n\t"
        "s_lshr_b32 s61, %[cy], %[sh]\n\t"
        "s_lshl_b32 s79, s61, 16\n\t"
        "s_or_b32 s79, s79, s60\n\t"
        "s_cmp_eq_u32 s79, s81\n\t"
        "s_cbranch_scc1 L_samecell%=\n\t"
        // ---- another cell: the window's range words
        "s_mov_b32 s81, s79\n\t"
        "s_mov_b32 s58, 0\n\t"
        "s_sub_i32 s62, s60, 1\n\t"
        "s_max_i32 s62, s62, 0\n\t"                                 // x0
        "s_add_i32 s63, s60, 1\n\t"
        "s_min_i32 s63, s63, %[Gm1]\n\t"
        "s_add_i32 s63, s63, 1\n\t"                                 // x1 + 1
        "s_sub_i32 s64, s61, 1\n\t"
        "s_max_i32 s64, s64, 0\n\t"                                 // y0
        "s_add_i32 s65, s61, 1\n\t"
        "s_min_i32 s65, s65, %[Gm1]\n\t"
        "s_sub_i32 s65, s65, s64\n\t"                               // y1 - y0: 2, or 1 in the first / last cell row
        "s_sub_i32 s66, s63, s62\n\t"
        "v_add_u32 v42, s64, %[rowoff]\n\t"                         // lanes 0..5: row of the range word, ...
        "v_mul_u32_u24 v43, s66, %[isend]\n\t"
        "v_add_u32 v43, s62, v43\n\t"                               // ... its cell column (x0: start of the row's range, x1 + 1: its end)
        "v_mad_u32_u24 v42, v42, %[G], v43\n\t"
        "v_lshl_add_u32 v42, v42, 2, %[cstb]\n\t"
        "ds_read_b32 v44, v42\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_readlane_b32 s67, v44, 0\n\t"
        "v_readlane_b32 s68, v44, 1\n\t"
        "v_readlane_b32 s69, v44, 2\n\t"
        "v_readlane_b32 s70, v44, 3\n\t"
        "v_readlane_b32 s71, v44, 4\n\t"
        "v_readlane_b32 s72, v44, 5\n\t"
        "s_sub_i32 s68, s68, s67\n\t"                               // n0
        "s_sub_i32 s70, s70, s69\n\t"                               // n1
        "s_sub_i32 s72, s72, s71\n\t"                               // n2 ...
        "s_cmp_lt_u32 s65, 2\n\t"
        "s_cselect_b32 s72, 0, s72\n\t"                             // ... none when the third row lies outside the grid
        "s_add_i32 s73, s68, s70\n\t"                               // n01
        "s_add_i32 s74, s73, s72\n\t"                               // total
        "s_sub_i32 s75, s69, s68\n\t"                               // lo1 - n0
        "s_sub_i32 s76, s71, s73\n\t"                               // lo2 - n01
        "s_nop 1\n\t"
        "s_branch L_ranges%=\n\t"
        "L_samecell%=:\n\t"                                          // the lanes may still hold this window's candidates: then no LDS read at all
        "s_cmp_eq_u32 s58, 1\n\t"
        "s_cbranch_scc1 L_hit1%=\n\t"
        "s_cmp_eq_u32 s58, 2\n\t"
        "s_cbranch_scc1 L_hit2%=\n\t"
        "L_ranges%=:\n\t"
        "s_cmp_eq_u32 s74, 0\n\t"
        "s_cbranch_scc1 L_fb3%=\n\t"
        "s_cmp_gt_u32 s74, 64\n\t"
        "s_cbranch_scc1 L_many%=\n\t"
        // ---- up to 64 candidates: one per lane, kept in the lanes while the cursor stays in the cell
        ORIP_NN_Q("%[lane]", "v46", "v47", "v48")
        "ds_read_u16 v49, v46\n\t"
        "v_cmp_gt_u32_e64 s[92:93], s74, %[lane]\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        ORIP_NN_FETCH("v49", "v45", "v51", "52", "53")
        "s_mov_b32 s58, 1\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "L_key%=:\n\t"
        ORIP_NN_KEY("v45", "v59", "52", "53", "s[92:93]")
        "v_mov_b32 v58, v49\n\t"
        "s_branch L_best%=\n\t"
        // ---- 65 .. 128 candidates: two per lane (A: v66, v70, v65, v[68:69], s[92:93]; B: v76, v71, v73, v[74:75], s[96:97]), kept like the single ones
        "L_many%=:\n\t"
        "s_cmp_gt_u32 s74, 128\n\t"
        "s_cbranch_scc1 L_loop%=\n\t"
        "v_add_u32 v43, 64, %[lane]\n\t"
        ORIP_NN_Q("%[lane]", "v46", "v47", "v48")
        "ds_read_u16 v66, v46\n\t"
        ORIP_NN_Q("v43", "v72", "v47", "v48")
        "ds_read_u16 v76, v72\n\t"
        "v_cmp_gt_u32_e64 s[92:93], s74, %[lane]\n\t"
        "v_cmp_gt_u32_e64 s[96:97], s74, v43\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        ORIP_NN_FETCH("v66", "v70", "v65", "68", "69")
        ORIP_NN_FETCH("v76", "v71", "v73", "74", "75")
        "s_mov_b32 s58, 2\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "L_key2%=:\n\t"
        ORIP_NN_KEY("v70", "v67", "68", "69", "s[92:93]")
        ORIP_NN_KEY("v71", "v77", "74", "75", "s[96:97]")
        "v_mov_b32 v58, v66\n\t"
        "v_mov_b32 v59, v67\n\t"
        "v_mov_b32 v52, v68\n\t"
        "v_mov_b32 v53, v69\n\t"
        "v_mov_b32 v51, v65\n\t"
        ORIP_NN_MERGE("76", "77", "74", "75", "v73")
        "s_branch L_best%=\n\t"
        // ---- more than 128: 128 per turn, the two halves' LDS reads in flight together; nothing is kept
        "L_loop%=:\n\t"
        "s_add_i32 %[cnt], %[cnt], 0x100000\n\t"
        "s_mov_b32 s58, 0\n\t"
        "s_mov_b32 s98, 0\n\t"
        "v_mov_b32 v58, -1\n\t"
        "v_mov_b32 v59, -1\n\t"
        "v_mov_b32 v52, 0\n\t"
        "v_mov_b32 v53, 0\n\t"
        "v_mov_b32 v51, 0\n\t"
        "L_pair%=:\n\t"
        "v_add_u32 v42, s98, %[lane]\n\t"
        "v_add_u32 v43, 64, v42\n\t"
        ORIP_NN_Q("v42", "v46", "v47", "v48")
        "ds_read_u16 v66, v46\n\t"
        ORIP_NN_Q("v43", "v72", "v47", "v48")
        "ds_read_u16 v76, v72\n\t"
        "v_cmp_gt_u32_e64 s[92:93], s74, v42\n\t"
        "v_cmp_gt_u32_e64 s[96:97], s74, v43\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        ORIP_NN_FETCH("v66", "v70", "v65", "68", "69")
        ORIP_NN_FETCH("v76", "v71", "v73", "74", "75")
        "s_waitcnt lgkmcnt(0)\n\t"
        ORIP_NN_KEY("v70", "v67", "68", "69", "s[92:93]")
        ORIP_NN_KEY("v71", "v77", "74", "75", "s[96:97]")
        ORIP_NN_MERGE("66", "67", "68", "69", "v65")
        ORIP_NN_MERGE("76", "77", "74", "75", "v73")
        "s_add_i32 s98, s98, 128\n\t"
        "s_cmp_lt_u32 s98, s74\n\t"
        "s_cbranch_scc1 L_pair%=\n\t"
        "L_best%=:\n\t"
        // ---- every lane: the next cursor if its candidate wins; the wave: the smallest key.  The winner is read backwards exactly when its
        // END entry won: had the start been as near or nearer it would hold a key as small or smaller (the gap test says every entry nearer
        // than the gap was scanned), and on equal keys the smaller entry word -- the start -- is taken below.  So entry word == index << 1 | flip.
        "v_mov_b32 v47, v59\n\t"
        "v_and_b32 v54, 0x7fff7fff, v52\n\t"
        "v_and_b32 v64, 1, v58\n\t"
        "v_min_u32_dpp v47, v47, v47 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "v_cmp_ne_u32 vcc, 0, v64\n\t"
        "v_cmp_gt_i32_e64 s[90:91], 0, v52\n\t"                     // closed (bit 31)
        "v_min_u32_dpp v47, v47, v47 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32 v62, v53, v54, vcc\n\t"
        "v_or_b32 v60, 0x8000, v52\n\t"
        "v_min_u32_dpp v47, v47, v47 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_e64 v62, v62, v54, s[90:91]\n\t"             // next cursor: the start when closed or read backwards, else the end
        "s_nop 0\n\t"
        "v_min_u32_dpp v47, v47, v47 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_u32_dpp v47, v47, v47 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_u32_dpp v47, v47, v47 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_readlane_b32 s77, v47, 63\n\t"
        "s_cmp_eq_u32 s77, -1\n\t"
        "s_cbranch_scc1 L_fb5%=\n\t"
        "v_cvt_u32_f32 v48, s77\n\t"
        "v_add_u32 v48, 1, v48\n\t"
        "v_cmp_ge_u32 vcc, s59, v48\n\t"
        "s_and_b64 s[94:95], vcc, exec\n\t"
        "s_cbranch_scc0 L_gap%=\n\t"
        "L_gapok%=:\n\t"
        "v_cmp_eq_u32_e64 s[82:83], s77, v59\n\t"
        "s_bcnt1_i32_b64 s79, s[82:83]\n\t"
        "s_cmp_eq_u32 s79, 1\n\t"
        "s_cbranch_scc1 L_win%=\n\t"
        // several lanes at the smallest distance: the smallest entry word among them (07:67 -- the first polyline in list order, its start first)
        "v_cndmask_b32_e64 v47, -1, v58, s[82:83]\n\t"
        ORIP_NN_MIN6
        "v_readlane_b32 s79, v47, 63\n\t"
        "s_nop 1\n\t"
        "v_cmp_eq_u32_e64 s[94:95], s79, v58\n\t"
        "s_and_b64 s[82:83], s[82:83], s[94:95]\n\t"
        "L_win%=:\n\t"
        "s_ff1_i32_b64 s84, s[82:83]\n\t"
        "v_readlane_b32 s85, v58, s84\n\t"
        "v_readlane_b32 s86, v62, s84\n\t"
        "s_mov_b64 s[90:91], exec\n\t"
        "s_mov_b64 exec, s[82:83]\n\t"
        "ds_write_b32 v51, v60\n\t"                                 // the used flag, by the winning lane
        "s_mov_b64 exec, s[90:91]\n\t"
        "v_writelane_b32 %[ringv], s85, m0\n\t"
        // the lanes' copies of the winner's end points (its other entry may sit in this window too) take the flag as well
        "s_lshr_b32 s79, s85, 1\n\t"
        "s_cmp_eq_u32 s58, 2\n\t"
        "s_cbranch_scc1 L_upd2%=\n\t"
        "v_lshrrev_b32 v50, 1, v49\n\t"
        "v_or_b32 v55, 0x8000, v52\n\t"
        "v_cmp_eq_u32 vcc, s79, v50\n\t"
        "v_cndmask_b32 v52, v52, v55, vcc\n\t"
        "s_branch L_next%=\n\t"
        "L_upd2%=:\n\t"
        "v_lshrrev_b32 v50, 1, v66\n\t"
        "v_or_b32 v55, 0x8000, v68\n\t"
        "v_cmp_eq_u32 vcc, s79, v50\n\t"
        "v_cndmask_b32 v68, v68, v55, vcc\n\t"
        "v_lshrrev_b32 v50, 1, v76\n\t"
        "v_or_b32 v55, 0x8000, v74\n\t"
        "v_cmp_eq_u32 vcc, s79, v50\n\t"
        "v_cndmask_b32 v74, v74, v55, vcc\n\t"
        "L_next%=:\n\t"
        "s_and_b32 %[cx], s86, 0xffff\n\t"
        "s_lshr_b32 %[cy], s86, 16\n\t"
        "v_cvt_f32_i32 v40, %[cx]\n\t"
        "v_cvt_f32_i32 v41, %[cy]\n\t"
        "s_add_i32 %[step], %[step], 1\n\t"
        "s_add_i32 m0, m0, 1\n\t"
        "s_cmp_eq_u32 m0, 64\n\t"
        "s_cbranch_scc1 L_flush%=\n\t"
        "s_cmp_ge_u32 %[step], %[n]\n\t"
        "s_cbranch_scc1 L_done%=\n\t"
        "s_branch L_step%=\n\t"
        // ---- the nearest candidate is farther than cell + 1: the exact gap = cell + min over x and y of min(l + 1, cell - l), l = cursor inside its cell
        "L_gap%=:\n\t"
        "s_and_b32 s79, %[cx], s88\n\t"
        "s_sub_i32 s80, s87, s79\n\t"
        "s_add_i32 s79, s79, 1\n\t"
        "s_min_i32 s79, s79, s80\n\t"
        "s_and_b32 s80, %[cy], s88\n\t"
        "s_sub_i32 s78, s87, s80\n\t"
        "s_add_i32 s80, s80, 1\n\t"
        "s_min_i32 s80, s80, s78\n\t"
        "s_min_i32 s79, s79, s80\n\t"
        "s_add_i32 s79, s79, s87\n\t"
        "s_mul_i32 s78, s79, s79\n\t"
        "s_lshr_b32 s80, s78, 18\n\t"
        "s_sub_i32 s78, s78, s80\n\t"
        "s_add_i32 s78, s78, -1\n\t"
        "v_cmp_ge_u32 vcc, s78, v48\n\t"
        "s_and_b64 s[94:95], vcc, exec\n\t"
        "s_cbranch_scc1 L_gapok%=\n\t"
        "s_mov_b32 %[ev], 6\n\t"                                       // 6: the gap test wants a wider window
        "s_branch L_out%=\n\t"
        "L_hit1%=:\n\t"
        "s_add_i32 %[cnt], %[cnt], 1\n\t"
        "s_branch L_key%=\n\t"
        "L_hit2%=:\n\t"
        "s_add_i32 %[cnt], %[cnt], 0x400\n\t"
        "s_branch L_key2%=\n\t"
        "L_fb3%=:\n\t"                                                 // 3: empty window
        "s_mov_b32 %[ev], 3\n\t"
        "s_branch L_out%=\n\t"
        "L_fb5%=:\n\t"                                                 // 5: every candidate used
        "s_mov_b32 %[ev], 5\n\t"
        "s_branch L_out%=\n\t"
        "L_flush%=:\n\t"
        "s_mov_b32 %[ev], 1\n\t"
        "s_branch L_out%=\n\t"
        "L_done%=:\n\t"
        "s_mov_b32 %[ev], 0\n\t"
        "L_out%=:\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "s_mov_b32 m0, s89\n\t"
        : [ev] "=&s"(ev), [cx] "+s"(s_cx), [cy] "+s"(s_cy), [step] "+s"(s_step), [ringv] "+v"(ringv), [cnt] "+s"(s_cnt)
        : [n] "s"(s_n), [sh] "s"(s_sh), [G] "s"(s_G), [Gm1] "s"(s_Gm1), [cstb] "s"(s_cst), [eidb] "s"(s_eid), [pb] "s"(s_p), [nem1] "s"(s_nem1),
          [rowoff] "v"(rowoff), [isend] "v"(isend), [lane] "v"(lane)
        : "vcc", "scc", "memory",
          "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s80", "s81",
          "s82", "s83", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98",
          "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60",
          "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77");
#undef ORIP_NN_Q
#undef ORIP_NN_FETCH
#undef ORIP_NN_KEY
#undef ORIP_NN_MERGE
#undef ORIP_NN_MIN6
    cx = s_cx; cy = s_cy; step = s_step; dbg_cnt = s_cnt;
    return ev;
}

// Grid-pruned search (same selection rule, same tie-break, n <= 11000 or so and int16 coordinates): the entry points (start of every
// polyline, end of every polyline that may be entered reversed) are bucketed into a G x G grid held in LDS next to the end points.  A greedy
// step scans the (2r+1)^2 cells around the cursor, r = 1, 3, 7, ...; it is final as soon as the best squared distance is below the squared
// gap between the cursor and the nearest unscanned cell (every unscanned entry is at least that far, so it can neither win nor tie), or the
// window covers the grid.  The chain of steps is strictly serial and a step looks at a few dozen entries, so ONE wavefront runs it: no
// barriers, no cross-wave exchange, and no other wave competing for the SIMD.
// The step is written for the way a lone wave executes (one instruction per ~4.5 cycles, +16..20 cycles whenever the scalar unit consumes
// a value produced by a vector instruction, every exec-mask juggle of divergent control flow a handful of both): a straightforward step
// compiles to ~350 instructions with divergent loops around uniform values = 1.1 us per step.  Here
//   * everything that is the same in all lanes (cursor, window, cell ranges, winner) is kept in SGPRs explicitly (v_readfirstlane);
//   * the candidates of the 3x3 window are evaluated without branches: every lane maps its ordinal to an entry with selects, entries
//     beyond the end take the pattern 0xffffffff; a candidate is a 2-byte entry + one 8-byte LDS read (both end points packed);
//   * the minimum runs over the 32-bit float pattern of the squared distance (6 DPP steps); the index tie-break of the reference (first
//     polyline in list order wins) only runs when two lanes hold the same pattern; the winner's end points come out of the winning lane's
//     registers (v_readlane), not from another LDS round trip;
//   * "no unscanned cell can be nearer" is an integer test: floor(d2) + 1 <= gap^2 - gap^2 / 2^18 - 1 (the three float roundings of a
//     squared distance stay below 2^-22 relative): conservative, so at worst one more round is scanned, never a wrong winner;
//   * results leave through a VGPR (one lane per step, 64 at a time);
//   * a window taller than three rows (r >= 3: what the asm loop hands back) is one pass per 64 rows: the rows' bounds in the lanes, a wave scan
//     over their counts, and the candidates 64 per trip across the rows -- not a scalar round trip per row.
// Dynamic LDS: P (8 n bytes), cst (4 (G^2 + 2)), Eid (room for 2 n entries of 2 bytes), and behind it wtab, 129 words (NN_WTAB_BYTES) that map the
// ordinals of a wide round's trip to their rows; the host's 158 KB check covers the first three, wtab lies between it and the CU's 160 KB.
__global__ __launch_bounds__(64) void k_greedy_nn_fast(const NNEnds* __restrict__ ends, int n, const int* __restrict__ sel, int skip_if, int need_any, int rule07, int G,
                                                        int32_t* __restrict__ order, uint8_t* __restrict__ flips, int no_asm, unsigned long long* __restrict__ dbg) {
    ORIP_NN_GATE(sel, skip_if, need_any)
    extern __shared__ __align__(16) unsigned char smem[];
    uint2* P = reinterpret_cast<uint2*>(smem);                                     // .x = sx | sy << 16, .y = ex | ey << 16; bit 15 of sx: used, bit 15 of sy: closed (rule07)
    unsigned* cst = reinterpret_cast<unsigned*>(P + n);                            // cst[0] = 0, cst[c + 1] = end of cell c
    uint16_t* Eid = reinterpret_cast<uint16_t*>(cst + (G * G + 2));                // entries sorted by cell: idx << 1 | end
    unsigned* wtab = reinterpret_cast<unsigned*>(Eid + 2 * n);                     // behind room for 2 n entries: 128 slots + a spare one, the rows of a wide round's trip (NN_WTAB_BYTES)
    const unsigned long long t_k0 = dbg ? __builtin_amdgcn_s_memtime() : 0ull;
    const int lane = threadIdx.x;
#define NNU(x) __builtin_amdgcn_readfirstlane((int)(x))
    int mnx = 0x7fffffff, mny = 0x7fffffff, mxx = -0x7fffffff, mxy = -0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        NNEnds e = ends[i];
        mnx = min(mnx, min(e.sx, e.ex)); mxx = max(mxx, max(e.sx, e.ex)); mny = min(mny, min(e.sy, e.ey)); mxy = max(mxy, max(e.sy, e.ey));
    }
    for (int o = 32; o > 0; o >>= 1) { mnx = min(mnx, __shfl_xor(mnx, o, 64)); mny = min(mny, __shfl_xor(mny, o, 64)); mxx = max(mxx, __shfl_xor(mxx, o, 64)); mxy = max(mxy, __shfl_xor(mxy, o, 64)); }
    const int ox = mnx, oy = mny;
    for (int i = lane; i < n; i += 64) {
        NNEnds e = ends[i];
        P[i] = make_uint2((unsigned)((e.sx - ox) | (i == seed ? 0x8000 : 0)) | ((unsigned)((e.sy - oy) | ((rule07 && e.closed) ? 0x8000 : 0)) << 16),
                          (unsigned)(e.ex - ox) | ((unsigned)(e.ey - oy) << 16));
    }
    unsigned* cnt = cst + 1;                                                       // counts, then cell ends
    for (int i = lane; i <= G * G + 1; i += 64) cst[i] = 0;
    __syncthreads();
    int sh = 0; while (((max(mxx - mnx, mxy - mny)) >> sh) >= G) sh++;
    sh = NNU(sh);
    for (int i = lane; i < n; i += 64) {
        const uint2 e = P[i];
        atomicAdd(&cnt[(((e.x >> 16) & 0x7fff) >> sh) * G + ((e.x & 0x7fff) >> sh)], 1u);
        if (!(e.x & 0x80000000u)) atomicAdd(&cnt[((e.y >> 16) >> sh) * G + ((e.y & 0xffff) >> sh)], 1u);
    }
    __syncthreads();
    {
        const int per = (G * G + 63) / 64, c0 = lane * per, c1 = min(G * G, c0 + per);
        unsigned sm = 0;
        for (int cc = c0; cc < c1; cc++) sm += cnt[cc];
        unsigned inc = sm;
        for (int o = 1; o < 64; o <<= 1) { unsigned t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        unsigned run = inc - sm;
        for (int cc = c0; cc < c1; cc++) { unsigned v = cnt[cc]; cnt[cc] = run; run += v; }     // starts for now
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {         // scatter; cnt[c] ends up as the END of cell c, so start(c) = cst[c], end(c) = cst[c + 1]
        const uint2 e = P[i];
        Eid[atomicAdd(&cnt[(((e.x >> 16) & 0x7fff) >> sh) * G + ((e.x & 0x7fff) >> sh)], 1u)] = (uint16_t)(i << 1);
        if (!(e.x & 0x80000000u)) Eid[atomicAdd(&cnt[((e.y >> 16) >> sh) * G + ((e.y & 0xffff) >> sh)], 1u)] = (uint16_t)((i << 1) | 1);
    }
    __syncthreads();
    const unsigned n_ent = (unsigned)NNU(cst[G * G]);
    int cx, cy;
    { const uint2 e = P[seed]; const bool cl = (e.x & 0x80000000u) != 0; cx = NNU(cl ? (e.x & 0x7fff) : (e.y & 0xffff)); cy = NNU(cl ? ((e.x >> 16) & 0x7fff) : (e.y >> 16)); }
    unsigned ringv = lane == 0 ? (unsigned)(seed << 1) : 0u;                      // lane (step & 63): index << 1 | flip of that step
    const int Gm1 = G - 1;
    const bool use_asm = G >= 4 && !no_asm;
    const unsigned lds_p = (unsigned)(uintptr_t)P, lds_cst = (unsigned)(uintptr_t)cst, lds_eid = (unsigned)(uintptr_t)Eid;
    const int rowoff = lane < 6 ? (lane >> 1) : 0, isend = lane < 6 ? (lane & 1) : 0;
    int step = 1, r_first = 1;
    unsigned long long d_fb = 0, d_calls = 0, t_asm = 0, t_gen = 0;      // ORIP_NN_DBG2: steps taken by the compiled code, asm entries, cycles in either
    unsigned d_rounds = 0, d_cand = 0;                                   // ... its rounds and the candidates they hold (entries of the windows' cells)
    if (dbg && lane == 0) dbg[9] = (__builtin_amdgcn_s_memtime() - t_k0) << 32;     // ... cycles of the prologue (bounding box, P, the grid), above the count of word 9
    while (step < n) {
        if (use_asm) {
            const unsigned long long t_0 = dbg ? __builtin_amdgcn_s_memtime() : 0ull;
            int cnt = 0;
            const int ev = nn_asm_steps(cx, cy, step, ringv, n, sh, G, lds_p, lds_cst, lds_eid, n_ent - 1u, rowoff, isend, lane, cnt);
            if (dbg) { t_asm += __builtin_amdgcn_s_memtime() - t_0; d_calls++; if (lane == 0) { if (ev >= 2) dbg[2 + ev]++; dbg[4] += (unsigned)cnt & 0x3ffu; dbg[6] += ((unsigned)cnt >> 10) & 0x3ffu; dbg[9] += (unsigned)cnt >> 20; } }
            if (ev == 1) { order[step - 64 + lane] = (int32_t)(ringv >> 1); flips[step - 64 + lane] = (uint8_t)(ringv & 1u); continue; }
            if (ev == 0) break;
            r_first = 3;                          // the 3x3 window has just been found wanting (empty, all used, or the nearest lies beyond the gap): the next one
        }
        // ---- one step with the compiled code: whatever the loop above does not take
        const unsigned long long t_g0 = dbg ? __builtin_amdgcn_s_memtime() : 0ull;
        d_fb++;
        const int gx = cx >> sh, gy = cy >> sh;
        const float fx = (float)cx, fy = (float)cy;
        unsigned wi = 0, w0 = 0, w1 = 0;
        for (int r = r_first;; r = 2 * r + 1) {
            const int x0 = max(0, gx - r), x1 = min(Gm1, gx + r), y0 = max(0, gy - r), y1 = min(Gm1, gy + r);
            unsigned myk = ~0u, myi = 0x7fffffffu, my0 = 0, my1 = 0;
            d_rounds++;
            // entry `q` (clamped into the table) as a candidate; valid == false: counts as infinitely far
            struct Cand { unsigned k, i; uint2 e; };
            auto fetch = [&](unsigned q, bool valid) {
                const unsigned id = Eid[q < n_ent ? q : n_ent - 1u]; Cand c; c.i = id >> 1;
                c.e = P[c.i];
                const unsigned xy = (id & 1u) ? c.e.y : (c.e.x & 0x7fff7fffu);
                const float dx = __fsub_rn((float)(xy & 0xffffu), fx), dy = __fsub_rn((float)(xy >> 16), fy);
                const unsigned k = __float_as_uint(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
                c.k = (valid && !(c.e.x & 0x8000u)) ? k : ~0u;                       // used polylines (the previous one among them) do not count
                return c;
            };
            auto merge = [&](const Cand& c) {
                const unsigned long long key = ((unsigned long long)c.k << 32) | c.i, mine = ((unsigned long long)myk << 32) | myi;
                const bool better = key < mine;
                myk = better ? c.k : myk; myi = better ? c.i : myi; my0 = better ? c.e.x : my0; my1 = better ? c.e.y : my1;
            };
            auto consider = [&](unsigned q, bool valid) { merge(fetch(q, valid)); };
            // two candidates per lane, both fetched before either is compared: their LDS reads are in flight together
            auto consider2 = [&](unsigned qa, bool va, unsigned qb, bool vb) { const Cand a = fetch(qa, va), b = fetch(qb, vb); merge(a); merge(b); };
            if (y1 - y0 <= 2) {
                // lanes 0..5: start / end of the entry range of the (up to) three rows
                const int row = y0 + (lane >> 1);
                const int ci = row * G + ((lane & 1) ? x1 + 1 : x0);
                const unsigned bnd = (lane < 6 && row <= y1) ? cst[ci] : 0u;
                const unsigned lo0 = (unsigned)__builtin_amdgcn_readlane((int)bnd, 0), n0 = (unsigned)__builtin_amdgcn_readlane((int)bnd, 1) - lo0;
                const unsigned lo1 = (unsigned)__builtin_amdgcn_readlane((int)bnd, 2), n1 = (unsigned)__builtin_amdgcn_readlane((int)bnd, 3) - lo1;
                const unsigned lo2 = (unsigned)__builtin_amdgcn_readlane((int)bnd, 4), n2 = (unsigned)__builtin_amdgcn_readlane((int)bnd, 5) - lo2;
                const unsigned n01 = n0 + n1, total = n01 + n2;
                if (dbg) d_cand += total;
                for (unsigned t0 = 0; t0 < total; t0 += 64) {                        // uniform trip count, no exec masking
                    const unsigned t = t0 + lane;
                    unsigned q = lo0 + t;
                    q = t >= n0 ? lo1 + (t - n0) : q;
                    q = t >= n01 ? lo2 + (t - n01) : q;
                    consider(q, t < total);
                }
            } else {
                // a taller window, 64 rows per pass: lane L reads both bounds of row yc + L, a wave scan gives every row the ordinal of its first
                // candidate, and the candidates go 128 per trip (two per lane), whatever rows they lie in -- no scalar round trip per row.  A trip
                // finds its rows through wtab: every non-empty row that starts inside the trip writes (first ordinal << 16 | first entry) at the slot
                // of that ordinal, the row that holds the trip's first ordinal writes slot 0, every other lane the spare slot 128; a running maximum
                // over the slots (the words grow with the row) hands each ordinal the word of its row.  Ordinals and entries stay below 2^15.
                for (int yc = y0; yc <= y1; yc += 64) {
                    const int row = min(yc + lane, y1);
                    const unsigned lo = cst[row * G + x0], hi = cst[row * G + x1 + 1];
                    const unsigned cn = yc + lane <= y1 ? hi - lo : 0u;
                    const unsigned incl = wave_incl_scan_u32(cn), excl = incl - cn;
                    const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
                    const unsigned word = (excl << 16) | lo;
                    if (dbg) d_cand += total;
                    for (unsigned t0 = 0; t0 < total; t0 += 128) {                   // uniform trip count, no exec masking; two ordinals per lane, their LDS reads in flight together
                        // (lanes write slots that other lanes read: relaxed atomics with a wave-scope fence between them -- plain LDS writes and reads, in order)
                        __hip_atomic_store(&wtab[lane], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        __hip_atomic_store(&wtab[64 + lane], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        __hip_atomic_store(&wtab[(cn != 0u && excl < t0 + 128u && incl > t0) ? max(excl, t0) - t0 : 128u], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        const unsigned wa = wave_incl_scan_max_u32(__hip_atomic_load(&wtab[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
                        unsigned wb = wave_incl_scan_max_u32(__hip_atomic_load(&wtab[64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
                        wb = max(wb, (unsigned)__builtin_amdgcn_readlane((int)wa, 63));      // the row that reaches over from the first half
                        const unsigned ta = t0 + lane, tb = ta + 64u;
                        consider2((wa & 0xffffu) + (ta - (wa >> 16)), ta < total, (wb & 0xffffu) + (tb - (wb >> 16)), tb < total);
                    }
                }
            }
            // minimum distance pattern over the wave
            unsigned m = myk;
#define ORIP_DPP_MINU(ctrl, rmask) { const unsigned t_ = (unsigned)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)m, ctrl, rmask, 0xf, false); m = t_ < m ? t_ : m; }
            ORIP_DPP_MINU(0x111, 0xf) ORIP_DPP_MINU(0x112, 0xf) ORIP_DPP_MINU(0x114, 0xf) ORIP_DPP_MINU(0x118, 0xf) ORIP_DPP_MINU(0x142, 0xa) ORIP_DPP_MINU(0x143, 0xc)
#undef ORIP_DPP_MINU
            const unsigned mink = (unsigned)__builtin_amdgcn_readlane((int)m, 63);
            bool final_ = x0 == 0 && y0 == 0 && x1 == Gm1 && y1 == Gm1;            // everything scanned
            if (!final_ && mink != ~0u) {
                int gap;                                                             // distance to the nearest unscanned cell, over the open sides
                if (r == 1) {
                    // the 3x3 window (94 % of the rounds): its sides lie one cell beyond the cursor's cell, so the gap is a function of the cursor's
                    // position inside its cell.  A side on the border of the grid counts as open here -- a smaller gap is conservative.
                    const int cell = 1 << sh, lx = cx & (cell - 1), ly = cy & (cell - 1);
                    gap = cell + min(min(lx + 1, cell - lx), min(ly + 1, cell - ly));
                } else {
                    gap = 0x7fff;
                    if (x0 > 0) gap = min(gap, cx - (x0 << sh) + 1);
                    if (x1 < Gm1) gap = min(gap, ((x1 + 1) << sh) - cx);
                    if (y0 > 0) gap = min(gap, cy - (y0 << sh) + 1);
                    if (y1 < Gm1) gap = min(gap, ((y1 + 1) << sh) - cy);
                }
                const unsigned g2 = (unsigned)(gap * gap);                           // gap < 2^15: exact
                const unsigned bfl = (unsigned)NNU((unsigned)__uint_as_float(mink)); // floor of the best squared distance (< 2^31)
                final_ = bfl + 1u <= g2 - (g2 >> 18) - 1u && g2 > 1u;
            }
            if (final_) {
                unsigned long long tie = __ballot(myk == mink);
                if (tie & (tie - 1)) {                                               // several lanes hold this distance: the smallest index wins
                    unsigned ci2 = myk == mink ? myi : 0x7fffffffu;
                    for (int o = 32; o > 0; o >>= 1) { const unsigned t_ = (unsigned)__shfl_xor((int)ci2, o, 64); ci2 = t_ < ci2 ? t_ : ci2; }
                    tie = __ballot(myk == mink && myi == ci2);
                }
                // every lane settles the reading direction and the next cursor of ITS candidate (a dozen vector instructions); the winner's come
                // out with two v_readlane -- instead of three, followed by the same arithmetic on scalars that wait for them
                const unsigned sxy = my0 & 0x7fff7fffu;
                const float ds = nn_d2((int)(sxy & 0xffffu), (int)(sxy >> 16), cx, cy), de = nn_d2((int)(my1 & 0xffffu), (int)(my1 >> 16), cx, cy);
                const bool cl = (my0 & 0x80000000u) != 0;
                bool flip;
                const unsigned ncur = nn_direction(cl, ds, de, flip) ? sxy : my1;
                const unsigned pack = (myi << 1) | (flip ? 1u : 0u);
                const int win_lane = __ffsll((long long)tie) - 1;
                wi = (unsigned)__builtin_amdgcn_readlane((int)pack, win_lane);
                w1 = (unsigned)__builtin_amdgcn_readlane((int)ncur, win_lane);
                w0 = (unsigned)__builtin_amdgcn_readlane((int)my0, win_lane);
                break;
            }
        }
        P[wi >> 1].x = w0 | 0x8000u;                                 // the used flag, through the type the entries are read as (every lane writes the same word)
        ringv = lane == (step & 63) ? wi : ringv;
        if ((step & 63) == 63) { order[step - 63 + lane] = (int32_t)(ringv >> 1); flips[step - 63 + lane] = (uint8_t)(ringv & 1u); }
        cx = (int)(w1 & 0xffffu); cy = (int)(w1 >> 16);
        step++;
        if (dbg) t_gen += __builtin_amdgcn_s_memtime() - t_g0;
    }
    if (dbg && lane == 0) { dbg[0] = d_fb | ((unsigned long long)d_rounds << 32); dbg[1] = d_calls | ((unsigned long long)d_cand << 32); dbg[2] = t_asm; dbg[3] = t_gen; }
    { const int done = n & ~63; if (done + lane < n) { order[done + lane] = (int32_t)(ringv >> 1); flips[done + lane] = (uint8_t)(ringv & 1u); } }
#undef NNU
}
}  // namespace

// ORIP_NN_DBG2 (debug): waits for the grid kernel and prints its counters (dbg: LaneFlags::nn_dbg2, cleared again for the next list)
static int nn_dbg2_report(orip_ctx* c, unsigned long long* dbg, int kind, int64_t n, int G) {
    unsigned long long h[10];
    HIPC(c, hipStreamSynchronize(LN(c).stream)); HIPC(c, hipMemcpy(h, dbg, 80, hipMemcpyDeviceToHost));
    const unsigned long long lo32 = 0xffffffffull;      // words 0, 1 and 9 carry a second counter in their upper half
    fprintf(stderr, "[nn dbg2] kind %d n %lld G %d: %llu steps by the compiled code (empty %llu, all used %llu, gap %llu; asm steps from cached candidates: "
                    "one per lane %llu, two per lane %llu; with more than 128 candidates %llu), %llu asm entries, cycles asm %llu compiled %llu; "
                    "compiled rounds %llu with %llu candidates, prologue cycles %llu\n",
            kind, (long long)n, G, h[0] & lo32, h[5], h[7], h[8], h[4], h[6], h[9] & lo32, h[1] & lo32, h[2], h[3], h[0] >> 32, h[1] >> 32, h[9] >> 32);
    HIPC(c, hipMemsetAsync(dbg, 0, 80, LN(c).stream));
    return 0;
}
int vreorder(orip_ctx* c, DPolys& src, DPolys& dst, int kind, const orip_params08* prefetch08) {
    int64_t n = src.n;
    if (n == 0) { HIPC(c, dst.clear(LN(c).stream)); return 0; }
    if (n > 0x7fffffff) ORIP_FAIL(c, "too many polylines");
    PolyFeat* feat; NNEnds* ends; GatherDesc* desc; int32_t* order; uint8_t *flips, *used;
    { Carve L; L.each(n, feat, ends, desc, order, flips, used); HIPC(c, L.commit(LN(c).vtmp[VTL_FEAT], 256)); }
    const int what = kind == 7 ? VF_ARC_CLOSED : (kind == 8 ? VF_PER : VF_ARC_OPEN);
    if (kind == 7 && is_coded(src) && src.vident && !getenv("ORIP_ARC_POINTS")) {      // whole walks: the long contours' arc lengths from the walk records
        VSrc vs_; ORIP_TRY(vsrc_of(c, src, vs_));
        vfeatures_short(c, vs_, n, what, feat, nullptr);
        if (src.total > ORIP_LONG_POLY) { ProfScope ps(c, "k_walk_arcs"); vwalk_arcs(c, vs_, n, feat); }
        HIPC(c, hipGetLastError());
    } else ORIP_TRY(vfeatures(c, src, what, feat));
    ORIP_WITH_SRC(c, src, ps, { hipLaunchKernelGGL(k_ends_from_feat<decltype(ps)>, dim3(cdiv(n, 256)), dim3(256), 0, LN(c).stream, feat, n, kind == 7 ? 1 : 0, ps, ends); });
    LaneFlags* fl = LN(c).flags.as<LaneFlags>(); int* d_seed = fl->nn_seed;
    hipLaunchKernelGGL(k_argmax_feat, dim3(1), dim3(256), 0, LN(c).stream, feat, (int)n, kind == 8 ? 0 : 1, d_seed, ends);      // seed and coordinate-range flags in one pass
    const size_t lds = (size_t)n * 9 + 16;
    // grid side: as fine as LDS allows (cells are powers of two, so twice the side is four times fewer candidates per window),
    // but not many more cells than polylines
    int G = 8; while (G < 128 && (size_t)(G + 8) * (G + 8) <= 4 * (size_t)n && (size_t)n * 12 + (size_t)((G + 8) * (G + 8) + 1) * 4 + 64 <= 158 * 1024) G += 8;
    const size_t lds_grid = (size_t)n * 12 + (size_t)(G * G + 1) * 4 + 64;        // (+4 for k_greedy_nn_fast: inside the 64 spare bytes of the 158 KB check)
    constexpr size_t NN_WTAB_BYTES = 129 * 4;                                     // k_greedy_nn_fast's wtab, behind the 158 KB the check admits: the CU has 160 KB
    static std::once_flag attr_once;                // several layer threads may arrive here together
    static std::atomic<int> attr_err{0};
    std::call_once(attr_once, [] {
        orip_max_lds(k_greedy_nn<NNStoreLds>, 150 * 1024, attr_err);
        orip_max_lds(k_greedy_nn_fast, 158 * 1024 + 4 + (int)NN_WTAB_BYTES, attr_err);
    });
    if (attr_err.load()) ORIP_FAIL(c, "hipFuncSetAttribute(greedy kernels) failed: %s", hipGetErrorString((hipError_t)attr_err.load()));
    // Seed and coordinate-range flags stay on the device: every kernel that may have to run is enqueued and picks itself from the flags
    // (NN_BEYOND_I16 -> the global-memory instance; NN_BEYOND_15BIT -> no grid).  No host round trip in front of the chain.
    if (prefetch08) HIPC(c, hipEventRecord(LN(c).ev2, LN(c).stream));      // everything the prefetch's side-stream work reads (features, ends) is complete at this point of the stream
    const bool grid_ok = n >= 64 && n <= 16000 && lds_grid <= 158 * 1024 && !getenv("ORIP_NN_NOGRID");
    const bool lds_ok = n <= 16000;
    const int r07 = kind == 7 ? 1 : 0;
    {
        ProfScope ps(c, "k_greedy_nn");
        if (grid_ok) {
            unsigned long long* dbg2 = getenv("ORIP_NN_DBG2") ? fl->nn_dbg2 : nullptr;
            if (dbg2) HIPC(c, hipMemsetAsync(dbg2, 0, 80, LN(c).stream));
            hipLaunchKernelGGL(k_greedy_nn_fast, dim3(1), dim3(64), lds_grid + 4 + NN_WTAB_BYTES, LN(c).stream, ends, (int)n, d_seed, NN_BEYOND_I16 | NN_BEYOND_15BIT, 0, r07, G, order, flips, getenv("ORIP_NN_NOASM") ? 1 : 0, dbg2);
            if (dbg2) ORIP_TRY(nn_dbg2_report(c, dbg2, kind, n, G));
        }
        // Behind the grid kernel only ONE more launch, and a light one (256 threads, no dynamic LDS): a kernel that merely checks its flag and
        // returns still waits for a CU with room for its whole workgroup -- 0.5 ms for 1024 threads or 150 KB of LDS next to the other layers' work.
        // The grid kernel bows out for coordinates beyond 15 bits only (never on a canvas below 32768 px): the global-memory instance takes those.
        if (lds_ok && !grid_ok) hipLaunchKernelGGL(k_greedy_nn<NNStoreLds>, dim3(1), dim3(1024), lds, LN(c).stream, ends, (int)n, d_seed, NN_BEYOND_I16, 0, r07, (uint8_t*)nullptr, order, flips);
        const int need = grid_ok ? (NN_BEYOND_I16 | NN_BEYOND_15BIT) : (lds_ok ? NN_BEYOND_I16 : 0);
        hipLaunchKernelGGL(k_greedy_nn<NNStoreGlobal>, dim3(1), dim3(lds_ok ? 256 : 1024), 0, LN(c).stream, ends, (int)n, d_seed, 0, need, r07, used, order, flips);
    }
    if (prefetch08) ORIP_TRY(orip_prefetch08(c, *prefetch08, src, feat));
    hipLaunchKernelGGL(k_desc_from_order, dim3(cdiv(n, 256)), dim3(256), 0, LN(c).stream, src.off.as<int64_t>(), order, flips, n, 0, feat, desc);
    HIPC(c, hipGetLastError());
    return vgather_list(c, desc, n, src, dst, src.total);      // every polyline of the source, whole: the same number of points
}
