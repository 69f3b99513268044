// csrc/gcode_merge.hip -- --merge-paths of gcode2stream.py / svg2stream.py: step polylines that meet end to end become one stroke (orip_gcode_merge; the rule
// is stated in include/orip.h and has one answer for every input).  Ours: the reference's generators draw paths that are already whole.
//
// Path p has two ENDS, 2p (head, its first point) and 2p + 1 (tail), and two traversal STATES, 2p (forwards, head -> tail) and 2p + 1 (backwards).  State t
// enters its path through end t and leaves it through end t ^ 1, so with partner[e] = the end joined to end e (or -1)
//     succ[t] = partner[t ^ 1]            the state that follows t: the partner end's path, entered through that end
// and the mirror of a reading t0, t1, ..., tk is tk ^ 1, ..., t1 ^ 1, t0 ^ 1.  Every chain therefore appears twice; the reading that holds (lowest member,
// forwards) is the one that is written.
//
// 1. Ends -> nodes.  (group, x, y) needs 66 bits, so the table holds END INDICES: open addressing over a power of two of at least 4n slots, a slot claimed
//    by a 32-bit atomicCAS of the end index; an end that finds a slot taken compares the whole triple through the occupant's index, joins it or probes on.
//    The claiming end owns the node: cnt[owner] counts the arrivals, arr[2 owner + k] keeps arrival k < 2.  Which arrival is which does not matter, only
//    degree exactly 2 joins.
// 2. Links.  One thread per state works out partner[t ^ 1] by the four conditions (same node, degree 2, another path, tail to head unless REVERSE).
// 3. Chains, by pointer jumping over succ: R rounds with 2^R >= n, fixed on the host, ping-pong between two arrays of (next, low, count, points), no host
//    round trip.  low = the smallest state id from t on (the smallest path, with the direction it has in this reading), count = states from t on, points =
//    sum of (length - 1) from t on.  Pass 1: a state whose pointer is still alive after R rounds never reaches a free end, it is on a cycle, and its low
//    has gone all the way round.  The reading with low = 2m is cut in front of state 2m (the state whose successor is 2m loses it), its mirror behind
//    state 2m + 1: two open chains, mirrors of each other, the first of which starts at (m, forwards).  Pass 2 jumps again over the cut successors.  Then
//    for a state t of path p, with a = pass2[t] and b = pass2[t ^ 1] (the mirror reading from p on, i.e. everything in front of t):
//        lowest state of t's reading   low = a.low if its path is the smaller one, else b.low ^ 1;   t is written iff low is even
//        members in front of t         b.count - 1            points in front of t        b.points - (len_p - 1)
//        members, points of the chain  a.count + b.count - 1, a.points + b.points - (len_p - 1) + 1
//    Path m is the lowest member of its chain iff low(2m) == 2m; it then carries the chain's totals, everybody else zeros, and three exclusive scans over
//    the PATH INDEX give the chain's output ordinal, its first point and its first member slot.  Nothing is sorted.
// 4. Emit.  One thread per state writes member / rev / the offsets and where its path's points go; one thread per input point copies it there (a path's
//    points sit in consecutive lanes, forwards or backwards, so a long member's stores coalesce); the first point of every member but the first is dropped.
//
// Launches: ends, insert, links, R jumps, cut, R jumps, heads, three scans, place, emit: 2R + 7 kernels and the scans' own; one host sync at the end, for
// the four stats.  Every index that is computed from chain data is checked against its array before it is used; a miss sets MgCounters::bad and fails the call.
//
// Scratch, free between calls.  c->mg_tab (nodes): E int4[2n] = (x, y, group, 0) per end; slot int[T]; own int[2n]; cnt unsigned[2n]; arr int[4n]; grp int[n].
// c->mg_tmp (chains): succ0 int[2n]; JA, JB int4[2n]; cyc u8[2n]; head unsigned[3][n + 1] = (is lowest, chain points, chain members) and scan unsigned[3][n + 1]
// = their exclusive scans; place int2[n] = (first output point, 1 reversed | 2 first point dropped); MgCounters.
// Resident: the merged polylines (gc_publish; orip_ctx.h states the list's contract and this writer's gc_merged rule), member_off / member / rev in c->mg_res until the next merge.
#include "orip_ctx.h"
#include "gc_convert.h"
#include <rocprim/rocprim.hpp>

namespace {
struct MgCounters { unsigned cycles, bad; };

__device__ __forceinline__ unsigned mg_hash(const int4 e) {
    unsigned long long k = (((unsigned long long)(unsigned)e.x << 32) | (unsigned)e.y) * 0x9E3779B97F4A7C15ull + (unsigned long long)(unsigned)e.z * 0xC2B2AE3D27D4EB4Full;
    k ^= k >> 32; k *= 0xD6E8FEB86659FD93ull; k ^= k >> 32;
    return (unsigned)k;
}

// ------------------------------------------------------------------------------------------------ 1. ends -> nodes
__global__ __launch_bounds__(256) void k_mg_ends(const long long* __restrict__ off, const int2* __restrict__ pts, const int* __restrict__ grp, int n, int4* __restrict__ E) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int2 a = pts[off[p]], b = pts[off[p + 1] - 1];
    const int g = grp[p];
    E[2 * p] = make_int4(a.x, a.y, g, 0); E[2 * p + 1] = make_int4(b.x, b.y, g, 0);
}
// slot changes under the kernel; E does not.  At most 2n of the >= 4n slots are ever taken, so a probe always ends; the bound only states it
__global__ __launch_bounds__(256) void k_mg_insert(const int4* __restrict__ E, int m, unsigned mask, int* slot, int* __restrict__ own, unsigned* cnt, int* __restrict__ arr) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int4 me = E[e];
    unsigned h = mg_hash(me) & mask;
    int o = e;
    for (unsigned tries = 0; tries <= mask; tries++, h = (h + 1) & mask) {
        const int old = atomicCAS(&slot[h], -1, e);
        if (old == -1) break;                                                 // the node is new: this end owns it
        if ((unsigned)old >= (unsigned)m) continue;
        const int4 q = E[old];
        if (q.x == me.x && q.y == me.y && q.z == me.z) { o = old; break; }    // the whole triple, never a hash of it
    }
    const unsigned k = atomicAdd(&cnt[o], 1u);
    if (k < 2) arr[2 * o + k] = e;
    own[e] = o;
}

// ------------------------------------------------------------------------------------------------ 2. links
__device__ __forceinline__ int mg_partner(int e, int m, const int* __restrict__ own, const unsigned* __restrict__ cnt, const int* __restrict__ arr, int rev) {
    const int o = own[e];
    if ((unsigned)o >= (unsigned)m || cnt[o] != 2u) return -1;
    const int a = arr[2 * o], b = arr[2 * o + 1], q = a == e ? b : a;
    if ((unsigned)q >= (unsigned)m || (q >> 1) == (e >> 1)) return -1;        // both ends of one closed path
    if (!rev && !((q ^ e) & 1)) return -1;                                    // head to head or tail to tail
    return q;
}
__global__ __launch_bounds__(256) void k_mg_links(const long long* __restrict__ off, int m, const int* __restrict__ own, const unsigned* __restrict__ cnt, const int* __restrict__ arr,
                                                  int rev, int* __restrict__ succ0, int4* __restrict__ J) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const int p = t >> 1, s = mg_partner(t ^ 1, m, own, cnt, arr, rev);
    succ0[t] = s;
    J[t] = make_int4(s, t, 1, (int)(off[p + 1] - off[p] - 1));
}

// ------------------------------------------------------------------------------------------------ 3. chains
// (next, low, count, points) of t and of the state its pointer names, combined; count and points only mean something in pass 2 (on a cycle they wrap)
__global__ __launch_bounds__(256) void k_mg_jump(const int4* __restrict__ A, int4* __restrict__ B, int m) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    int4 a = A[t];
    if ((unsigned)a.x < (unsigned)m) {
        const int4 b = A[a.x];
        a.x = b.x; a.y = min(a.y, b.y); a.z = (int)((unsigned)a.z + (unsigned)b.z); a.w = (int)((unsigned)a.w + (unsigned)b.w);
    }
    B[t] = a;
}
__global__ __launch_bounds__(256) void k_mg_cut(const long long* __restrict__ off, int m, const int4* __restrict__ J1, const int* __restrict__ succ0, uint8_t* __restrict__ cyc,
                                                int4* __restrict__ J) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const int4 j = J1[t];
    const bool on_cycle = j.x >= 0;
    int s = succ0[t];
    if (on_cycle) {
        if (!(j.y & 1)) { if (s == j.y) s = -1; }                             // the reading with (m, forwards): cut in front of it
        else if (t == j.y) s = -1;                                            // its mirror: cut behind (m, backwards)
    }
    cyc[t] = on_cycle ? 1 : 0;
    const int p = t >> 1;
    J[t] = make_int4(s, t, 1, (int)(off[p + 1] - off[p] - 1));
}
// the lowest state of t's reading: from t on (a) and, through the mirror, in front of t (b)
__device__ __forceinline__ int mg_low(const int4 a, const int4 b) { return (a.y >> 1) <= (b.y >> 1) ? a.y : (b.y ^ 1); }

__global__ __launch_bounds__(256) void k_mg_heads(const long long* __restrict__ off, int n, const int4* __restrict__ J, const uint8_t* __restrict__ cyc, unsigned* __restrict__ head,
                                                  MgCounters* cn) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    unsigned is = 0, points = 0, members = 0;
    if (p < n) {
        const int4 a = J[2 * p], b = J[2 * p + 1];
        if (mg_low(a, b) == 2 * p) {
            const unsigned w = (unsigned)(off[p + 1] - off[p] - 1);
            is = 1; points = (unsigned)a.w + (unsigned)b.w - w + 1u; members = (unsigned)a.z + (unsigned)b.z - 1u;
            if (cyc[2 * p]) atomicAdd(&cn->cycles, 1u);
        }
    }
    head[p] = is; head[(size_t)(n + 1) + p] = points; head[2 * (size_t)(n + 1) + p] = members;
}

// ------------------------------------------------------------------------------------------------ 4. emit
__global__ __launch_bounds__(256) void k_mg_place(const long long* __restrict__ off, int n, long long total, const int4* __restrict__ J, const unsigned* __restrict__ scan,
                                                  int2* __restrict__ place, int* __restrict__ member, uint8_t* __restrict__ rev, long long* __restrict__ member_off,
                                                  long long* __restrict__ out_off, MgCounters* cn) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const unsigned* ord = scan; const unsigned* ptoff = scan + (size_t)(n + 1); const unsigned* memoff = scan + 2 * (size_t)(n + 1);
    if (t == 0) {
        if (ord[n] <= (unsigned)n) { out_off[ord[n]] = (long long)ptoff[n]; member_off[ord[n]] = (long long)memoff[n]; } else atomicOr(&cn->bad, 1u);
    }
    if (t >= 2 * n) return;
    const int p = t >> 1;
    const int4 a = J[t], b = J[t ^ 1];
    const int low = mg_low(a, b);
    if (low & 1) return;                                                      // the mirror reading writes this path
    const int lm = low >> 1;
    if ((unsigned)lm >= (unsigned)n) { atomicOr(&cn->bad, 1u); return; }
    const unsigned w = (unsigned)(off[p + 1] - off[p] - 1);
    const unsigned k = (unsigned)b.z - 1u, before = (unsigned)b.w - w;       // members and points in front of t
    const unsigned c = ord[lm], base = ptoff[lm], mo = memoff[lm];
    const unsigned long long dst = (unsigned long long)base + (k ? 1u + before : 0u);
    if ((unsigned long long)mo + k >= (unsigned long long)n || c >= (unsigned)n || dst + w + (k ? 0u : 1u) > (unsigned long long)total) { atomicOr(&cn->bad, 1u); place[p] = make_int2(-1, 0); return; }
    member[mo + k] = p; rev[mo + k] = (uint8_t)(t & 1);
    place[p] = make_int2((int)dst, (t & 1) | (k ? 2 : 0));
    if (k == 0) { out_off[c] = (long long)base; member_off[c] = (long long)mo; }
}
__global__ __launch_bounds__(256) void k_mg_emit(const long long* __restrict__ off, const int2* __restrict__ pts, int n, long long total, const int2* __restrict__ place,
                                                 int2* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int p = (int)gc_path_of(off, n, i);                                    // every path has points, so this is the path of point i
    const int2 pl = place[p];
    if (pl.x < 0) return;
    long long q = i - off[p];
    if (pl.y & 1) q = off[p + 1] - off[p] - 1 - q;
    if (pl.y & 2) { if (q == 0) return; q--; }                                // equals the point in front of it
    if (pl.x + q < total) out[pl.x + q] = pts[i];
}
}  // namespace

// include/orip.h states the rule; the merged polylines become the resident step polylines
extern "C" int orip_gcode_merge(orip_ctx* c, const int64_t* off, const int32_t* pts, const int32_t* group, int64_t n, int32_t n_groups, int32_t flags, int64_t* stats) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (!stats) ORIP_FAIL(c, "bad arguments");
    if (flags & ~ORIP_MERGE_REVERSE) ORIP_FAIL(c, "unknown flags %d", flags);
    int64_t total;
    ORIP_TRY(gc_steps_check(c, __func__, off, pts, n, false, total));
    ORIP_TRY(gc_check_groups(c, __func__, group, n, n_groups, nullptr));
    hipStream_t s = LN(c).stream;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) {                                                             // nothing to launch; the explicit form leaves the empty list resident
        if (off) ORIP_TRY(gc_publish_empty(c, __func__));
        c->gc_merged = true; c->mg_n = 0; c->mg_paths = 0;
        return 0;
    }
    const int N = (int)n, M = 2 * N;
    unsigned T = 4; while ((int64_t)T < 4 * n) T <<= 1;
    int R = 0; while (((int64_t)1 << R) < n) R++;                             // rounds of each jumping pass
    int4 *E, *JA, *JB; int *slot, *own, *arr, *grp, *succ0; unsigned *cnt, *head, *scan; uint8_t* cyc; int2* place; MgCounters* cn;
    { Carve L; L.take(E, (size_t)M); L.take(slot, (size_t)T); L.take(own, (size_t)M); L.take(cnt, (size_t)M); L.take(arr, (size_t)2 * M); L.take(grp, (size_t)N);
      HIPC(c, L.commit(c->mg_tab, 64)); }
    { Carve L; L.take(succ0, (size_t)M); L.take(JA, (size_t)M); L.take(JB, (size_t)M); L.take(cyc, (size_t)M); L.take(head, 3 * ((size_t)N + 1)); L.take(scan, 3 * ((size_t)N + 1));
      L.take(place, (size_t)N); L.take(cn, 1); HIPC(c, L.commit(c->mg_tmp, 64)); }
    HIPC(c, c->mg_off.ensure(((size_t)N + 1) * 8 + 64)); HIPC(c, c->mg_pts.ensure((size_t)total * 8 + 64));       // the output is never larger than the input
    long long* r_moff; int* r_member; uint8_t* r_rev;
    { Carve L; L.take(r_moff, (size_t)N + 1); L.take(r_member, (size_t)N); L.take(r_rev, (size_t)N); HIPC(c, L.commit(c->mg_res, 64)); }
    c->mg_n = -1;
    if (off) ORIP_TRY(gc_steps_upload(c, __func__, off, pts, n, total));      // checked above: from here on the input is the resident list
    c->gc_merged = true;                                                      // the sources no longer name these polylines
    if (group) HIPC(c, hipMemcpyAsync(grp, group, (size_t)N * 4, hipMemcpyHostToDevice, s));
    else HIPC(c, hipMemsetAsync(grp, 0, (size_t)N * 4, s));
    HIPC(c, hipMemsetAsync(slot, 0xFF, (size_t)T * 4, s));
    HIPC(c, hipMemsetAsync(cnt, 0, (size_t)M * 4, s));
    HIPC(c, hipMemsetAsync(cn, 0, sizeof(MgCounters), s));
    const long long* d_off = c->gc_off.as<long long>(); const int2* d_pts = c->gc_pts.as<int2>();
    const dim3 gp(cdiv(N, 256)), gs(cdiv(M, 256)), b(256);
    hipLaunchKernelGGL(k_mg_ends, gp, b, 0, s, d_off, d_pts, grp, N, E);
    { ProfScope ps(c, "k_mg_insert");
      hipLaunchKernelGGL(k_mg_insert, gs, b, 0, s, E, M, T - 1, slot, own, cnt, arr); }
    hipLaunchKernelGGL(k_mg_links, gs, b, 0, s, d_off, M, own, cnt, arr, flags & ORIP_MERGE_REVERSE ? 1 : 0, succ0, JA);
    int4 *src = JA, *dst = JB;
    { ProfScope ps(c, "k_mg_jump");
      for (int r = 0; r < R; r++) { hipLaunchKernelGGL(k_mg_jump, gs, b, 0, s, src, dst, M); std::swap(src, dst); } }
    hipLaunchKernelGGL(k_mg_cut, gs, b, 0, s, d_off, M, src, succ0, cyc, dst);
    std::swap(src, dst);
    { ProfScope ps(c, "k_mg_jump");
      for (int r = 0; r < R; r++) { hipLaunchKernelGGL(k_mg_jump, gs, b, 0, s, src, dst, M); std::swap(src, dst); } }
    hipLaunchKernelGGL(k_mg_heads, dim3(cdiv((int64_t)N + 1, 256)), b, 0, s, d_off, N, src, cyc, head, cn);
    for (int k = 0; k < 3; k++)
        HIPC(c, orip_with_tmp(c, [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, head + k * ((size_t)N + 1), scan + k * ((size_t)N + 1), 0u, (size_t)N + 1, rocprim::plus<unsigned>(), s); }));
    hipLaunchKernelGGL(k_mg_place, gs, b, 0, s, d_off, N, (long long)total, src, scan, place, r_member, r_rev, r_moff, c->mg_off.as<long long>(), cn);
    { ProfScope ps(c, "k_mg_emit");
      hipLaunchKernelGGL(k_mg_emit, dim3(cdiv(total, 256)), b, 0, s, d_off, d_pts, N, (long long)total, place, c->mg_pts.as<int2>()); }
    HIPC(c, hipGetLastError());
    struct { unsigned paths, points; MgCounters cn; } h = {0, 0, {0, 0}};
    HIPC(c, hipMemcpyAsync(&h.paths, scan + N, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.points, scan + ((size_t)N + 1) + N, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(&h.cn, cn, sizeof(MgCounters), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));                                         // the one sync
    if (h.cn.bad || h.paths < 1 || h.paths > (unsigned)N || (int64_t)h.points > total) { gc_drop(c); ORIP_FAIL(c, "the chains do not add up (internal error)"); }
    gc_publish(c, c->mg_off, c->mg_pts, h.paths, h.points);
    c->mg_n = n; c->mg_paths = h.paths;
    stats[0] = h.paths; stats[1] = h.points; stats[2] = n - (int64_t)h.paths; stats[3] = h.cn.cycles;
    return 0;
}

extern "C" int orip_gcode_merge_fetch(orip_ctx* c, int64_t* member_off, int32_t* member, uint8_t* rev) {
    orip_enter(c);
    ORIP_LANE(c, ORIP_LANE_CROSS);
    if (c->mg_n < 0) ORIP_FAIL(c, "no merge: orip_gcode_merge has not succeeded since the last failure");
    if (!member_off || (c->mg_n > 0 && (!member || !rev))) ORIP_FAIL(c, "bad arguments");
    if (c->mg_n == 0) { member_off[0] = 0; return 0; }
    hipStream_t s = LN(c).stream;
    const size_t n = (size_t)c->mg_n;
    long long* r_moff; int* r_member; uint8_t* r_rev;                         // the layout orip_gcode_merge carved; the buffer already holds it, so nothing grows
    { Carve L; L.take(r_moff, n + 1); L.take(r_member, n); L.take(r_rev, n); HIPC(c, L.commit(c->mg_res, 64)); }
    HIPC(c, hipMemcpyAsync(member_off, r_moff, (size_t)(c->mg_paths + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(member, r_member, n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(rev, r_rev, n, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    return 0;
}
