// csrc/orip_ctx.h -- device context of liborip.so (gfx950 only).
#pragma once
// Environment switches that force a path, and the input that takes the same path without them.  The rule: a switch may only force a path that
// some input reaches anyway (the tests then check it against the default one); a path that no input reaches is deleted, not kept behind a switch.
//   ORIP_MORPH_BYTES       byte-plane morphology                      non-binary explicit masks
//   ORIP_PACK_BYTES        any-width bit-plane packing / unpacking    W % 64 != 0          (bitplane.h: k_pack_bits, k_bits_to_bytes)
//   ORIP_NMS_BYTES         byte-plane blur + NMS                      gauss_k != 3, or H / W below 8
//   ORIP_NN_NOGRID         greedy order without the grid kernel       list sizes beyond the LDS / grid limits
//   ORIP_PLOT_1WG          plot order without the LDS kernel          list sizes beyond the LDS limit
//   ORIP_TAPS_1WG          sequential taps without the LDS kernel     list sizes beyond the LDS limit
//   ORIP_HASH_SORT         stage-08 near test through sorted buckets  its size condition
//   ORIP_TAIL_SEQ          sequential tail replay of every polyline   its redo condition
//   ORIP_CAPPREV_SCAN      previous in-canvas sample by a scan        a polyline leaves the canvas
//   ORIP_ARC_POINTS        stage-07 arc lengths from the points       explicit lists from set_polys
//   ORIP_NO_PREFETCH08     no stage-08 prefetch under stage 07        explicit lists from set_polys
//   ORIP_NN_NOASM          compiled greedy step                       the compiled step is the asm loop's fallback
//   ORIP_NO_CHAINS         per-pixel stepping of the walker           chains shorter than ORIP_CHAIN_MIN
//   ORIP_TRACE_LATE        traces started by orip_contours_layer      a lane held by another thread
//   ORIP_PAINT_SEPARABLE   separable line painting in stage 10        its radius and size conditions
// Debug and test hooks, which change no result: ORIP_CAPS_TINY, ORIP_CAPSSET_TINY, ORIP_CAPS_RANGE, ORIP_COMP_CAPS, ORIP_COMP_DBG, ORIP_TIME08, ORIP_TIME10, ORIP_WALK_DBG, ORIP_NN_DBG2, ORIP_TAIL_DBG,
// ORIP_ALLOC_DBG, ORIP_TRACE_LOG_F, ORIP_SERIAL_LAYERS.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <mutex>
#include <atomic>
#include "../../include/orip.h"

typedef uint8_t u8;

// `who` names the entry point in the message: a helper that checks arguments for several entry points passes its caller's __func__ on
#define ORIP_FAIL_AS(ctx, who, ...)                                      \
    do {                                                                 \
        char _b[512];                                                    \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                           \
        { std::lock_guard<std::mutex> _g((ctx)->mu); (ctx)->err = std::string(who) + ": " + _b; } \
        return -1;                                                       \
    } while (0)
#define ORIP_FAIL(ctx, ...) ORIP_FAIL_AS(ctx, __func__, __VA_ARGS__)

#define HIPC_AS(ctx, who, call)                                                                \
    do {                                                                                       \
        hipError_t _e = (call);                                                                \
        if (_e != hipSuccess) ORIP_FAIL_AS(ctx, who, "%s -> %s", #call, hipGetErrorString(_e)); \
    } while (0)
#define HIPC(ctx, call) HIPC_AS(ctx, __func__, call)

#define ORIP_TRY(expr) do { int _r = (expr); if (_r != 0) return _r; } while (0)

extern int orip_alloc_dbg;      // ORIP_ALLOC_DBG: log every (re)allocation -- in steady state there must be none (hipFree waits for the whole device)
// Growable device buffer; contents are NOT preserved across growth unless keep=true.
struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes, hipStream_t s = 0, bool keep = false) {
        if (bytes <= cap) return hipSuccess;
        if (orip_alloc_dbg) fprintf(stderr, "[alloc] %p: %zu -> %zu bytes%s\n", (void*)this, cap, bytes, p ? " (hipFree: device-wide wait)" : "");
        size_t ncap = bytes + bytes / 4 + 256;
        void* np_ = nullptr;
        hipError_t e = hipMalloc(&np_, ncap);
        if (e != hipSuccess) return e;
        if (keep && p && cap) {
            e = hipMemcpyAsync(np_, p, cap, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { hipFree(np_); return e; }
        }
        if (p) hipFree(p);
        p = np_; cap = ncap;
        return hipSuccess;
    }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};
#include "gc_cut.h"             // GcCut, the result record of a cutting pass, made of DBufs; and what the three passes share
// Device polyline list: off int64[n+1], pts int32[2*total].
// A list can also be WALK-CODED (virt): its points are not stored but generated from the walk records stage 04 leaves for the layer
// (WalkStore below: own points, bounce tails as (log range, cycle) pieces) through a view per polyline (walk, first point, length,
// reversed) and an optional stage-05 scale -- see vsrc.h.  The walker re-walks the same pixels up to 4 * fg times, so
// the explicit form of a heavy layer is 2.8e8 points (2.25 GB) for ~1e6 distinct ones; stages 05 / 07 / 08 read the coded form and the
// explicit form only exists where somebody asks for it (orip_get_polys, a consumer that is not view-aware: orip_polys_materialize).
struct DPolys {
    DBuf off, pts;
    int64_t n = 0, total = 0;
    bool virt = false;          // walk-coded: `off` is valid, `pts` only when pts_ok
    bool pts_ok = true;
    DBuf vview;                 // VView[n]; unused when vident (polyline i = walk i, whole, forward)
    bool vident = true;
    int vlayer = 0;             // whose WalkStore
    uint64_t vepoch = 0;        // WalkStore::epoch the list was built on: a later trace of the layer makes it stale
    uint64_t vsepoch = 0;       // scaled lists: WalkStore::sepoch of the scaled tables they read
    uint64_t pf_tag = 0;        // != 0: the list is a permutation-with-flips of the list LaneRes::pf08 (same tag) was computed on
    bool scaled = false;        // reads the scaled tables of the WalkStore
    void set_explicit() { virt = false; pts_ok = true; pf_tag = 0; }
    hipError_t clear(hipStream_t s) {      // the empty explicit list: no polylines, off[0] = 0
        n = 0; total = 0; set_explicit();
        const hipError_t e = off.ensure(64);
        return e == hipSuccess ? hipMemsetAsync(off.p, 0, 8, s) : e;
    }
};
static inline bool is_coded(const DPolys& P) { return P.virt && !P.pts_ok; }      // walk-coded and not expanded: the points come from the walk records
// What stage 04 leaves per layer (raster04.hip: trace_finish) and every walk-coded list of the layer reads
struct WalkStore {
    DBuf log;                   // the trace's state log (walker.h: 4 words per entry)
    DBuf walk, piece, own;      // VWalk[n], VPiece[...], int2 own points (start + own steps of every kept walk)
    DBuf lxy;                   // int2 pixel of every log entry in use (same index as the log)
    DBuf ent_idx, cnt;          // the indices of those entries, in any order; cnt[0] = how many (device side: nobody on the host needs it)
    DBuf own_s, lxy_s;          // the same two tables after _scale_one (05:82-96) with (sx, sy, dx, dy): what a scaled list reads
    float sx = 1.f, sy = 1.f, dx = 0.f, dy = 0.f;
    int64_t n = 0, n_own = 0, ent_cap = 0;
    int W = 0;
    uint64_t epoch = 0;         // bumped by every trace of the layer
    uint64_t sepoch = 0;        // bumped whenever own_s / lxy_s are rewritten
};
struct DTaps {
    DBuf xy;  // int32[2*n]
    int64_t n = 0;
};

struct ProfEntry { double ms = 0; int64_t launches = 0; };

// One device scratch layout, stated once: take() registers typed arrays in order, commit() sizes the buffer (the arrays, their alignment padding and
// `tail` bytes of slack that wide loads past the last element may touch) and assigns every pointer.  An array starts at a multiple of max(16, alignof(T),
// align); arrays that a kernel or one read-back addresses from a common base are ONE take.  No heap; at most CAP arrays.
struct Carve { enum { CAP = 16 };
    struct { void* pp; size_t off; } slot[CAP]; int n = 0; size_t total = 0;
    template <class T> void take(T*& ptr, size_t count, size_t align = 16) {
        if (alignof(T) > align) align = alignof(T);
        total = (total + align - 1) / align * align;
        if (n < CAP) { slot[n].pp = &ptr; slot[n].off = total; }
        n++; total += count * sizeof(T);
    }
    template <class... T> void each(size_t count, T*&... ptrs) { (take(ptrs, count), ...); }      // several arrays of one length
    hipError_t commit(DBuf& buf, size_t tail_bytes) {
        const hipError_t e = n > CAP ? hipErrorInvalidValue : buf.ensure(total + tail_bytes);
        for (int i = 0; e == hipSuccess && i < n; i++) { void* a = (char*)buf.p + slot[i].off; memcpy(slot[i].pp, &a, sizeof a); }
        return e;
    }
};

// Every word of LaneRes::flags: small device-side results (counts, change / overflow flags) that the host reads back or a later kernel of the same call
// consumes.  Each use has its own member, so two uses never share bytes; nothing aliases on purpose.  orip_create allocates and zeroes the buffer of every
// lane (all lanes exist from then on), but NO use relies on that zero: each word below is cleared, copied or written whole by its own call before it is read.
struct LaneFlags {
    // lane 0: raster stages
    int not_binary;                                         // 02 orip_morph_open_close: some byte of an explicit mask is neither 0 nor 255
    uint8_t palette[ORIP_MAX_LAYERS * 3];                   // 02 orip_assign_palette: the K RGB triples
    alignas(8) unsigned long long palette_counts[ORIP_MAX_LAYERS];   // 02 orip_assign_palette: pixels per label
    alignas(8) unsigned long long label_counts[ORIP_MAX_LAYERS];     // 02 orip_extract_layers: pixels per label
    int thin_changed[2];                                    // 04 prepare: per thinning iteration of a batch, something was deleted
    unsigned chain_counts[2];                               // 04 prepare (side stream): {chain ends, cpix entries}
    // layer lanes
    int trace_overflow;                                     // 04 trace: a log ran full (set by k_trace, read by trace_finish -- possibly in a later call)
    int nn_seed[2];                                         // vreorder (07 / 08 / 10 on its lane): seed polyline, coordinate-range flags
    alignas(8) unsigned long long nn_dbg2[10];              // vreorder: ORIP_NN_DBG2 counters of the grid greedy
    // The next four are cleared by k_caps_init, the first kernel of every growth round of 08-A4, on the lane's main stream; every writer and reader below is on
    // that stream, behind it, in the same call (the side stream's k_tail_replay takes no flag), and the read-back of the call before lies in front of it.
    int caps_overflow;                                      // 08-A4: the capsule table ran full.  Set by k_caps_insert right behind the clear, read back by the host, cleared
                                                            //        again by the next round's k_caps_init: exactly when a larger table starts from empty
    unsigned caps_distinct;                                 // 08-A4: distinct capsules.  Added to by k_caps_stamp_bits, which runs once, behind the last round; read back at the
                                                            //        end of orip_dedup_layer -> caps_hint (nothing of 08-A5, 08-B or the reorder in between writes it)
    unsigned accept_survivors;                              // 08-A5: samples the cheap test leaves for the near test.  Added to by k_accept_pre, read by k_accept_brute / k_accept
    alignas(8) unsigned long long accept_work;              // 08-A5: candidate pairs of the direct near test.  Added to by k_accept_pre, read back by the host behind it
    int zs_changed[12];                                     // 08-B: per thinning iteration of a batch, something was deleted
    unsigned comp_counts[3];                                // 08-B: work-list cursors of the three component classes
    int taps_kept;                                          // 10 (ORIP_LANE_CROSS): sequential taps accepted
    int plot_ops;                                           // 12: ops written
    // (last, so that the words above keep their offsets: a fill of a word range costs one dispatch more when the range leaves its 16-byte alignment)
    alignas(8) unsigned long long tail_dbg[4];              // 08-A3: ORIP_TAIL_DBG counters of k_tail_replay (side stream; cleared in front of it, written only with the variable set)
};
static_assert(sizeof(LaneFlags) <= 4096, "LaneRes::flags is 4096 bytes, allocated and zeroed by orip_create");

// Per-lane resources.  Lane 0 serves the raster stages and the cross-layer stage 10; lane l+1 serves the per-layer vector
// stages (05, 07, 08, 12) of layer l, so that different layers can be driven concurrently from different host threads,
// each on its own HIP stream with its own scratch (the serial kernels of one layer then overlap with those of the others).
// Lifetimes.  A buffer is FREE BETWEEN ENTRY POINTS (any call on the lane may resize and overwrite it) unless this table names it; a named vtmp slot is only
// ever indexed by its constant on that lane.
//   lane 0  vtmp[VT0_MEMO]       memo planes of the walker     orip_contours_reserve or orip_contours_prepare (sized there) -> last trace of the prepare.  Never
//           cleared as a whole: a word is meaningful only at a skeleton pixel of the current prepare, where trace_launch has zeroed it in front of the
//           layer's k_trace; anything elsewhere is stale and never read (WalkArgs::memo)
//   lane 0  vtmp[VT0_EDGE_BITS]  bit planes of `edges`         orip_detect_edges (c->edge_bits) -> the next orip_contours_prepare, which thins in them
//           its second set (orip_edge_planes: b) then holds the degree-2 planes: k_bits_to_skel_state of that prepare -> lane 0's ev3, while the chain kernels
//           step on them on the side stream; only a prepare's thinning writes it again, behind ev3 (orip_detect_edges sizes it and writes the first set only)
//   lane 0  vtmp[VT0_KEYS, VT0_COMP_START, VT0_ORDER, VT0_LOG_USED, VT0_WINFO]  the stage-04 schedule (Prep04::A, Prep04::order: keys / lin of the skeleton, first
//           pixel of each component, largest-first component order, log entries used per component, two WalkInfo per pixel): orip_contours_prepare -> the last
//           orip_contours_layer of that prepare (every layer's k_trace / trace_finish reads them from its own lane); orip_contours_invalidate ends the lifetime
//   lane l+1 vtmp[VTL_STEPLOG], flags.trace_overflow  step log and overflow flag of the layer's trace: trace_launch (orip_contours_prepare, or
//           orip_contours_layer) -> trace_finish (orip_contours_layer).  Stage 08-B takes the same slot: it must not run on the lane in between
//   lane l+1 vtmp[VT_LEAVES], tmpF  perimeter leaves and sort scratch of Prefetch08: side-stream work of orip_sort_contours -> ev4 (split_small) or
//           orip_pf08_drain of the next call (the main stream of orip_sort_contours itself goes behind ev4 before it uses tmpF again)
//   lane l+1 pf08.*              own buffers of Prefetch08; src_off points into the SCALED list's offsets (c->polys), valid while pf08.tag matches the list's pf_tag
//   ORIP_LANE_CROSS canvas       forbidden raster of stage 10  orip_dedup_cross_begin (cleared there) -> the last orip_dedup_cross_layer* call of that pass
//   Everything else -- tp[], pixbits, tmpE, canvas on the other lanes, the other vtmp slots, the rest of flags -- is free between entry points.
//
// WITHIN ONE CALL on a layer lane or on ORIP_LANE_CROSS all twelve slots are in use, so they alias on purpose: a slot is free for its next role once the
// kernels that read its previous one have been enqueued on the lane's stream (one stream: order is enough; where the side stream reads, the table says so).
// A helper overwrites what it takes, so a caller must not hold those live across the call:
//   vscan_excl, vsort_pairs, orip_with_tmp   tmpF (vscan_excl only above 32768 items)
//   vgather, vgather_views, vgather_list     tmpE, tmpF (their scan), dst
//   vfeatures                                VT_LEAVES, tmpF (only when the list has more than ORIP_LONG_POLY points: the long polylines' leaves and length order)
//   vreorder                                 VTL_FEAT, flags.nn_seed / nn_dbg2; all of vfeatures and vgather_list; with prefetch08: all of orip_prefetch08
//   split_small (vector08a.hip)              VTL_SPLIT, VTL_SPLIT_FEAT; all of vfeatures, vscan_excl and vgather_list; waits for ev4 or drains the prefetch
//   orip_runs_to_polys                       VTL_RUN_STARTS (one word pair per tile of ORIP_RUN_TILE slots), VTL_TAIL_RUNS (20 bytes per run; at most one run
//                                            per slot, and stage 10 comes close: every second one); all of vscan_excl; dst.  READS the caller's flags and
//                                            point source (08-A: sflag, sx, sy of VTL_SAMPLES; 10: VTL_CUM) until its last kernel
//   orip_prefetch08 (side stream)            pf08.*, VT_LEAVES, tmpF (until ev4); READS the caller's features (stage 07's VTL_FEAT) until ev3
// and every stage holds live, across such calls:
//   04  (raster04.hip)    on the layer's lane: VTL_STEPLOG trace_launch -> trace_finish (between entry points, see above); inside trace_finish VTL_CAPS (walk sums per
//                         slot, to k_vwalk_fill) and then VTL_CELLS (kept walk slots); with ORIP_WALK_DBG (debug) also VT_LEAVES: per-component counters,
//                         trace_launch -> trace_finish.  Calls orip_with_tmp (tmpF) for its scans
//   07  (vector.hip)      nothing of its own: vreorder's VTL_FEAT is the feat07 the prefetch reads on the side stream until ev3.  Stage 08's A0 fills the same
//                         slot behind ev4 only; the two meet in practice behind several host round trips of split_small, but no event orders them
//   08-A (vector08a.hip)  VTL_FEAT A0 -> k_rank_counts (across split_small, vsort_pairs, vscan_excl); VTL_RANKS A1 -> A6; VTL_CUM A2 (k_samples reads it last);
//                         VTL_SAMPLES, VTL_CELLS, canvas, pixbits A2 -> A6, VTL_SAMPLES on through orip_runs_to_polys (its sx, sy and sflag are the input);
//                         VTL_RANKS also holds the redo marks of A3 (nk + 1 words behind RsInfo: 1 + the last unsure sample), which the side stream reads until ev3 (awaited by A5);
//                         VTL_TAIL_RUNS A2 -> A6: the block-local tail sums (8 MS bytes; k_samples -> k_tail_par), then the last-in scan and then the
//                         survivors in its first 4 MS bytes, and orip_runs_to_polys takes the slot once A6 is enqueued;
//                         VTL_CAPS A4; A7's split_small finds everything but tp[] free
//   08-B (vector08b.hip)  VTL_FEAT (features, parents, groups) groups -> paths; canvas (group ids, defined at this call's stamped pixels only: B08::gid) raster -> paths; VTL_STEPLOG (bit planes)
//                         raster -> paths; VTL_SPLIT_FEAT (labels) and VTL_RANKS (block counts) within components; VTL_CUM (sorted pixels), VTL_CAPS (component
//                         tables) components -> paths; VTL_SAMPLES (heads) within components; VTL_CELLS within paths.  Calls vfeatures (first, into
//                         VTL_FEAT), vscan_excl, vsort_pairs and, last, vgather
//   08 C  (vector08.hip)  vreorder of tp[2] or tp[3]: nothing else is live
//   10  (vector10.hip)    canvas (forbidden raster, across calls) and VTL_STEPLOG (seed / distance planes) for the whole call; VTL_RANKS, VTL_CUM cut ->
//                         orip_runs_to_polys (VTL_CUM is its input); VTL_SPLIT, VTL_SPLIT_FEAT tiny lines -> the compaction of the taps; VTL_SAMPLES (tap
//                         sequence) from there to the end, across vreorder
//   12  (vector.hip)      VTL_FEAT, taken after the deferred vreorder of the layer has finished with it; calls vfeatures
enum { VT0_KEYS = 0, VT0_HEADS = 1, VT0_COMP_START = 2, VT0_ORDER = 3, VT0_ORDER_SORT = 5, VT0_MEMO = 6, VT0_LOG_USED = 7, VT0_WINFO = 8, VT0_EDGE_BITS = 10,     // lane 0
       VT0_NMS_BITS = 11 };     // (VT0_HEADS, VT0_ORDER_SORT: component heads / sort buffers inside orip_contours_prepare; VT0_NMS_BITS: candidate and strong planes inside orip_detect_edges)
// Layer lanes and ORIP_LANE_CROSS.  A name is the slot's role in stage 08-A, or in the helper that owns it; the other roles of the same index, in call order:
enum { VTL_RANKS = 0,           // 08-A: perimeter sort, order, samples per rank, sample bases + any-out word, RsInfo, redo flags | 08-B: skeleton pixels per block | 10: steps per point, their bases
       VTL_CUM = 1,             // 08-A: cumulative lengths and their offsets | 08-B: skeleton pixels sorted by label | 10: cut steps (points, flags)
       VTL_SPLIT = 2,           // split_small: tap / keep flags, their scans, tap centres, descriptors | 10: the same for _tiny_and_taps
       VTL_SAMPLES = 3,         // 08-A: the per-sample arrays (SampleArrs, npop, capprev, sflag) | 08-B: component heads and their scan | 10: tap sequence, accepted taps
       VTL_CAPS = 4,            // 08-A: capsule table | 08-B: component tables | 04 trace_finish: walk sums per slot
       VTL_CELLS = 5,           // 08-A: cell keys / values (bucket sort), sample hints | 08-B: per-component path scratch | 04 trace_finish: kept walk slots
       VTL_FEAT = 6,            // features: 08-A kept polylines | 08-B lines, parents, groups | vreorder (07, 08 C, 10, 12): features, ends, order | 12: features, alive flags
       VTL_RUN_STARTS = 7,      // orip_runs_to_polys: accepted slots and run starts per tile, scanned in place
       VTL_TAIL_RUNS = 8,       // 08-A: block-local tail sums -> last-in scan -> survivors, THEN orip_runs_to_polys: per run its first slot, rank and keep / length key, per kept run its first slot
       VTL_STEPLOG = 9,         // 04: step log of the layer's trace (between entry points, see above) | 08-B: thinning bit planes | 10: seed, distance, occupancy planes
       VTL_SPLIT_FEAT = 10,     // split_small: features of its source list | 08-B: union-find labels of the padded raster | 10: features of the cut lines
       VT_LEAVES = 11,          // wherever vfeatures runs: its perimeter leaves and length order, and those of the stage-08 prefetch (between entry points, see above) | 04 with ORIP_WALK_DBG: per-component debug counters of the trace
       VT_SLOTS = 12 };
struct LaneRes {
    hipStream_t stream = 0;
    hipStream_t stream2 = 0;              // side stream of the lane (work that may overlap the main chain), fenced with ev2 / ev3
    hipEvent_t ev2 = nullptr, ev3 = nullptr, ev4 = nullptr;   // (ev4 / ev3: features / everything of stage 08's prefetch)
    DBuf vtmp[VT_SLOTS], tmpE, tmpF, flags, canvas;             // flags: one LaneFlags
    DBuf pixbits;                         // stage 08-A: one bit per canvas pixel that is the rounded position of a sample
    unsigned caps_hint = 0;               // distinct capsules of the lane's last stage-08-A run (sizes the next run's table)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DPolys tp[6];   // persistent temporaries of the vector stages (no hipFree in steady state: hipFree synchronises the device)
    // stage 08's order-independent front, computed on the side stream while stage 07's greedy chain runs (vector08a.hip: orip_prefetch08)
    struct Prefetch08 {
        bool pending = false;          // side-stream work the lane's main stream has not waited for yet (orip_pf08_drain)
        bool valid = false; uint64_t tag = 0; int64_t n = 0; int64_t tot_f = 0; double step = 0;
        const int64_t* src_off = nullptr;   // offsets of the list it was computed on (device): both readings of polyline i keep their cumulative lengths at src_off[i]
        DBuf seg;                      // float32 length of every segment of the list (k_seglen -> both readings, perimeter sums)
        DBuf feat, info, cum, ord;     // PolyFeat[n] + reversed perimeters float[n]; RsInfo[2n]: forward at i, reversed at n + i; cum: forward readings, then (tot_f on) reversed
    } pf08;
};
extern thread_local int orip_tls_lane;
#define LN(c) ((c)->ln[orip_tls_lane])
// Hardware queues.  HIP multiplexes its streams onto GPU_MAX_HW_QUEUES hardware queues (4 when nothing is set) and kernels of different streams that
// share a queue run one after the other; the layer schedule is full of lone-wave kernels that hold a queue for milliseconds (k_trace, k_greedy_nn_fast),
// so it needs its active streams on separate queues.  The first orip_create of the process leaves at least ORIP_HW_QUEUES_WANTED in the variable
// (orip_api.hip: orip_queue_decision); it never writes more than ORIP_HW_QUEUES_MAX.  16 against 20: DESIGN 8.
enum { ORIP_HW_QUEUES_WANTED = 16, ORIP_HW_QUEUES_MAX = 32 };
// HIP's current device is per host thread: every entry point selects the context's GPU for the calling thread (the layer pipelines
// call in from pool threads, which would otherwise allocate and launch on device 0 of a multi-GPU node)
struct orip_ctx;
void orip_enter(orip_ctx* c);
#define ORIP_LANE_CROSS (ORIP_MAX_LAYERS + 1)
void orip_contours_free(orip_ctx* c);
// stage 04's schedule (orip_contours_prepare) no longer describes the resident state: waits for traces still in flight, then later orip_contours_layer
// calls fail until the next prepare (raster04.hip)
int orip_contours_invalidate(orip_ctx* c);
// A lane (stream + scratch that grows with hipFree / hipMalloc) serves ONE call at a time: two host threads on one lane would free
// buffers under each other's kernels (the r01 memory access fault of the sharded path: a stage-12 call addressed by the GLOBAL layer id
// landed on the lane of another layer's running 04->08 pipeline).  LaneGuard claims the lane for the calling thread and the entry
// points fail loudly when it is taken; nested claims of the lane the thread already holds are free.
struct LaneGuard {
    orip_ctx* c; int prev, lane; bool ok, owner;
    LaneGuard(orip_ctx* ctx, int lane_id);
    ~LaneGuard();
};
#define ORIP_LANE_NODRAIN_AS(ctx, who, lane_id)                                                                              \
    LaneGuard _lane_guard((ctx), (lane_id));                                                                                 \
    if (!_lane_guard.ok) ORIP_FAIL_AS(ctx, who, "lane %d is busy: another call is using this layer's stream and scratch", (int)(lane_id))
#define ORIP_LANE_NODRAIN(ctx, lane_id) ORIP_LANE_NODRAIN_AS(ctx, __func__, lane_id)
// Stage 08's prefetch (vector08a.hip: orip_prefetch08) may still be running on the lane's side stream when stage 07 returns: stage 08 waits for its parts where it
// consumes them; every other call that claims the lane puts its main stream behind the whole of it first (it reads the scaled list and the lane's scratch).
#define ORIP_LANE_AS(ctx, who, lane_id)                                                                                      \
    ORIP_LANE_NODRAIN_AS(ctx, who, lane_id);                                                                                 \
    HIPC_AS(ctx, who, orip_pf08_drain(ctx))
#define ORIP_LANE(ctx, lane_id) ORIP_LANE_AS(ctx, __func__, lane_id)

struct orip_ctx {
    int device = 0;
    LaneRes ln[ORIP_MAX_LAYERS + 2];      // 0: raster stages; l + 1: layer l; ORIP_LANE_CROSS: stage 10
    std::atomic<int> lane_owner[ORIP_MAX_LAYERS + 2];   // 1 while a call holds the lane (LaneGuard); lane 0 is not claimed
    orip_params10 p10{}; bool p10_ready = false;   // stage 10 between orip_dedup_cross_begin and the per-layer calls
    size_t hw_cross_off = 0, hw_cross_pts = 0;      // largest kept-line list of stage 10 so far: the buffers it swaps with the layers' LINES_CROSS slots never have to grow again
    bool cross_unordered[ORIP_MAX_LAYERS] = {false};   // LINES_CROSS of the layer still waits for its travel reorder (orip_dedup_cross_layer_deferred)
    void* prep04 = nullptr;               // stage-04 state between orip_contours_prepare and orip_contours_layer (raster04.hip)
    std::mutex mu;
    std::string err;
    // image / raster state
    int H = 0, W = 0, K = 0;
    DBuf image;     // u8 [H,W,3] BGR
    DBuf labels;    // u8 [H,W]
    DBuf masks;     // u8 [K,H,W]
    DBuf edges;     // u8 [K,H,W]
    DBuf skel;      // u8 [K,H,W]
    DBuf tmpA, tmpB, tmpC, tmpD;   // raster scratch
    DBuf cref, cpix;               // forced stretches of the skeletons (walker.h: ST_CHAIN): position plane and chain pixel lists
    DBuf lab_tabs;  // u16 gamma[256] + u16 cbrt[3072] + i32 coeffs[9]
    bool tabs_ready = false;
    // The resident k-means sample set (orip_kmeans_samples): km_idx int64[km_n], pixel indices into an image of km_npx pixels; km_n == 0: none.  The buffer
    // serves nothing else, so no stage overwrites it.  Lifetime: orip_kmeans_samples -> the next orip_kmeans_samples, or the first image of another pixel
    // count (orip_set_image, orip_resize_area as_image), or orip_destroy; an image of the same pixel count keeps it (the set depends on the count alone).
    DBuf km_idx; int64_t km_n = 0, km_npx = 0;
    void km_drop_unless(int64_t npx) { if (km_npx != npx) { km_n = 0; km_npx = 0; } }
    const void* edge_bits = nullptr;   // bit planes of `edges` left in lane 0's scratch by stage 03 (nullptr: not available); consumed by stage 04
    const void* morphed_bits = nullptr; // bit planes of the opened / closed masks left in tmpA for stage 03's NMS kernel (nullptr: byte planes in tmpB)
    const void* mask_bits = nullptr;   // bit planes of `masks` left in tmpA by stage 02 (nullptr: not available); consumed by stage 03
    // vector state
    DPolys polys[ORIP_SLOT_COUNT][ORIP_MAX_LAYERS];
    WalkStore wstore[ORIP_MAX_LAYERS];
    DTaps taps[2][ORIP_MAX_LAYERS];
    DBuf ops[ORIP_MAX_LAYERS];
    int64_t n_ops[ORIP_MAX_LAYERS] = {0};
    // multi-GPU exchange (comm.hip): RCCL communicator of this process, device row for the list sizes
    void* comm = nullptr; int comm_rank = 0, comm_world = 1;
    DBuf comm_sizes;
    // 13_build_stream: moves and their direction codes (stream.hip), resident between orip_stream_codes and the fetch
    DBuf stream_segs, stream_off, stream_codes; int64_t stream_n = 0, stream_total = 0;
    // 14_preview_stream: stream bytes, tile products / prefixes / totals / counters, key plane, RGB image (stream_preview.hip), resident until the fetch
    DBuf sp_data, sp_agg, sp_keys, sp_rgb; int sp_rw = 0, sp_rh = 0; bool sp_ready = false;
    // gcode2stream (gcode.hip): gc_tmp = scratch of the conversions; the piece table and the packed bytes between orip_stream_pack and its fetch (stream.hip).
    // THE RESIDENT STEP POLYLINES: gc_off int64[gc_n + 1], gc_pts int2[gc_total], valid while gc_ready; gc_src int32[gc_n] = the input path every polyline
    // came from, which names them while !gc_merged (a field of the merge's line below).  This block is the one statement of their contract; the helpers that
    // keep it are declared in gc_convert.h and defined in gcode.hip, and no other code writes these fields.
    //   Readers (fail while !gc_ready, or when the n they are given is not gc_n): orip_gcode_steps_fetch, orip_gcode_steps_source_fetch (also fails while
    //   gc_merged), and for NULL input orip_gcode_order, orip_gcode_order_pens, orip_gcode_improve, orip_gcode_merge, orip_gcode_simplify, orip_gcode_dedup, orip_gcode_occlude, orip_gcode_dash, orip_gcode_hatch_link; orip_svg_occlude and orip_svg_hatch_link always.
    //   orip_gcode_seam is a reader in both forms: NULL input reads the list, an explicit input goes to sm_in and does not become the list; it never writes these fields.
    //   orip_gcode_order_rings likewise: NULL input reads the list, an explicit input goes to ro_in.
    //   Writers, and what each leaves:
    //     orip_gcode_to_steps       drops the list on entry (gc_drop), before it looks at its arguments: after ANY failure there is no list.  Success: its
    //                               polylines and their sources, gc_merged cleared; no points to convert (n == 0 included): the empty list (gc_publish_empty).
    //     orip_gcode_to_steps_clip  checks first: an argument error leaves the list as it was.  Then as orip_gcode_to_steps: dropped, and a device-found
    //                               error (a coordinate not finite or out of range, counts that do not add up) leaves no list.
    //     orip_gcode_merge          checks first: an argument error leaves the list as it was.  The explicit form then uploads its input as the list
    //                               (gc_steps_upload; n == 0: the empty list); the resident form works on the list.  gc_merged is SET in every case that passes
    //                               the checks, n == 0 in either form included.  Success: the merged polylines (gc_publish swaps mg_off / mg_pts in).
    //                               A device-found error (chains that do not add up) leaves no list.
    //     orip_gcode_simplify       as the merge, with sp_off / sp_pts, but strokes keep their number and order, so gc_merged is left as it is -- except that
    //                               an explicit input of another count than the resident one (or with no list resident) cannot be the polylines the sources
    //                               name: then, n == 0 included, gc_merged is set.  An explicit input of the resident count is taken for the polylines a fetch gave out.
    //     THE CUTTING PASSES: orip_gcode_dedup (record dd), orip_gcode_occlude and orip_svg_occlude (oc), orip_gcode_dash (ds); gc_cut.h holds their
    //                               frame.  As the simplify, with the record's off / pts and the same rule for an explicit input and gc_merged: every check
    //                               of the arguments first (an argument error leaves the list as it was); n == 0 leaves the empty list (explicit form) or the
    //                               resident one, which is empty.  But strokes are cut and vanish, so while !gc_merged the sources are gathered through
    //                               origin and swapped in with the list (gc_cut_publish, the record's src): gc_src keeps naming the input path of every
    //                               stroke, with repeats as after the clip.  A device-found error (a repeated point in the resident list, 2^30 output
    //                               points or more, counts that do not add up; below, what a pass adds) leaves no list.  Particular to a pass:
    //       the occlusion           two entry points, explicit rings in steps or the resident fitted paths, behind their own checks of the strokes and one
    //                               body; it sizes its events and then its output by read-backs of their own, and a ring coordinate that is not finite or
    //                               out of range is a device-found error of the first.
    //       the dash                sizes its raw arrays by a read-back; when every stroke lies in a gap it launches nothing more and leaves the list of
    //                               no polylines; a dashed stroke of 2^62 units or more is a device-found error.
    //     orip_gcode_hatch_link, orip_svg_hatch_link (--hatch-connect, gcode_link.hip; record hl, the cutting passes' frame with origin = the first member
    //                               of every output stroke): every check of the arguments first (an argument error leaves the list as it was); n == 0
    //                               leaves the empty list (explicit form) or the resident one; the intake's rule for an explicit input and gc_merged.
    //                               Strokes are joined, so while !gc_merged the sources are gathered through the first member and swapped in with the
    //                               list (gc_cut_publish).  A device-found error (a ring coordinate not finite or out of range, 2^30 pairs in reach or
    //                               more, counts that do not add up) leaves no list.
    //   A failed HIP call inside a writer leaves what had been written up to it; gc_ready is false across an upload, so a list is never half there.
    DBuf gc_tmp, gc_off, gc_pts, gc_src, pk_tab, pk_out; int64_t gc_n = 0, gc_total = 0, pk_bytes = -1; bool gc_ready = false;
    // orip_gcode_order and orip_gcode_order_pens (gcode_order.hip: gc_grids), free between calls.  With n paths in G groups, m = n or 2n candidates (both ends
    // under ORIP_ORDER_REVERSE) and ncell cells over all groups' grids:
    //   gc_ends = se int4[n] (first x, y, last x, y), grp int[n], order int[n], rev u8[n], box int[4G], OpGroup[G]; grp and rev only for the grouped order
    //   gc_grid = cnt unsigned[ncell + 1], start unsigned[ncell + 1], fill unsigned[ncell], hdr int2[ncell] = (first entry, live entries) per cell,
    //             ent int4[m] = (x, y, id, 0), slot int[m] = where candidate id sits (under ORIP_ORDER_REVERSE only)
    DBuf gc_ends, gc_grid;
    // --merge-paths (gcode_merge.hip): mg_tab / mg_tmp = scratch of the node table and of the chains, free between calls (the unit states their layout);
    // mg_off / mg_pts = the output, swapped with gc_off / gc_pts when a merge succeeds; mg_res = member_off int64[mg_paths + 1], member int32[mg_n],
    // rev u8[mg_n] of the last merge of mg_n paths (-1: none) until the next one.  gc_merged: gc_src no longer names the resident step polylines (above)
    DBuf mg_tab, mg_tmp, mg_off, mg_pts, mg_res; int64_t mg_n = -1, mg_paths = 0; bool gc_merged = false;
    // --improve-order (gcode_improve.hip), free between calls: im_state = the ends, the given sequence and the two position-ordered copies of the state
    // (ab int4[2][n], id int[2][n]) a move is written between; im_rec = one record per block of the evaluation, the two status slots and the two travels
    // (the unit states the layout)
    DBuf im_state, im_rec;
    // --loop-start (gcode_seam.hip), free between calls: sm_state = per position of the sequence the ring size, where the stroke's points start, entry and
    // exit, the scanned flags, the runs, the levels, the large layers and the seams, and the counters; sm_in = off / pts of an explicit input; sm_f = the
    // cost-to-go of every ring vertex, int64 (the unit states the layout)
    DBuf sm_state, sm_in, sm_f;
    // --ring-entry (orip_gcode_order_rings, gcode_order.hip: 2c), free between calls.  With n strokes of `total` points in G groups, m candidates (every ring
    // vertex of a closed stroke; an open stroke's first point, and its last under ORIP_ORDER_REVERSE; m <= total + n) and ncell cells over all groups' grids:
    //   ro_in    = off int64[n + 1], pts int2[total] of an explicit input (the resident list is only read, and an explicit input does not become the list)
    //   ro_state = se int4[n] (first x, y, last x, y), grp int[n] (only when given), cnt int[n + 1] = candidates per stroke, cbase int[n + 1] = their
    //              exclusive scan (candidate c of stroke i has the id cbase[i] + c), order int[n], seam int[n], rev u8[n], box int[4G], gcand u64[G] =
    //              candidates per group, OpGroup[G], RoCounters, cd int4[total + n] = (x, y, stroke, group) by id
    //   ro_grid  = cnt unsigned[ncell + 1] = entries per cell and, under the chain, the LIVE entries of the cell, start unsigned[ncell + 1],
    //              fill unsigned[ncell], hdr int2[ncell] = (first entry, entries), which the chain never writes, ent int4[m] = (x, y, id, stroke) with
    //              id = -1 once the candidate has left, slot int2[m] = (entry, cell) of candidate id.  Entries never move.
    DBuf ro_in, ro_state, ro_grid;
    // --simplify-mm (gcode_simplify.hip): sp_tmp = the keep flags, their scan, the two span lists and the counts, free between calls (the unit states the
    // layout); sp_off / sp_pts = the output, swapped with gc_off / gc_pts when a call succeeds; sp_res = kept int64[sp_points], the input index of every
    // output point of the last call (-1: none) until the next one
    DBuf sp_tmp, sp_off, sp_pts, sp_res; int64_t sp_points = -1;
    // --dedup (gcode_dedup.hip): dd_tmp = the sort words, the sorted intervals, the per-segment records and the scans, free between calls (the unit states the
    // layout); dd = the result record (gc_cut.h: GcCut states what it holds and for how long, for all three cutting passes)
    DBuf dd_tmp; GcCut dd;
    // --occlude (gcode_occlude.hip): oc_tmp = the levels, the rings and their edges, the shapes' tables, the per-segment records and the scans; oc_ev = the
    // events, the hidden intervals and the pieces of the segments that meet a shape (the unit states both layouts), free between calls; oc = the result record
    DBuf oc_tmp, oc_ev; GcCut oc;
    // --dashes / --dash-mm (gcode_dash.hip): ds_tmp = the lengths and their scan, the patterns' tables, the per-segment counts and their scan, the list of
    // the segments a wave takes; ds_raw = the points and dashes before the repeated points and the collapsed dashes are taken out (the unit states both
    // layouts), free between calls; ds = the result record
    DBuf ds_tmp, ds_raw; GcCut ds;
    // --hatch-connect (gcode_link.hip): hl_tmp = the classes, the rings and their edges, the shapes' tables, the per-stroke flags and scans, the counters;
    // hl_ln = the lines' points, classes and strokes, the bucket keys of their STARTs unsorted and sorted, the pair counts and their scan, the bests, the
    // links and the two chain arrays; hl_pair = the pairs in reach and their eligibility (the unit states the three layouts), free between calls; hl = the
    // result record; hl_res = member_off int64[hl_paths + 1], member int32[hl_n] of the last call of hl_n strokes (-1: none) until the next one
    DBuf hl_tmp, hl_ln, hl_pair, hl_res; GcCut hl; int64_t hl_n = -1, hl_paths = 0;
    // --stipple-mm (gcode_stipple.hip), which reads the fitted paths and writes nothing of the resident step polylines: st_tmp = the rings and their edges,
    // the shapes' tables (first point, group, box, has an edge, the plan of its lattice slots), the chunks per shape and their scan, the counters; st_ch =
    // per chunk of 64 slots the dot mask, the dot count and its scan (the unit states both layouts), free between calls; st_out = THE DOT LIST, xy int2
    // [st_dots] and group int32[st_dots] of the last call (-1: none) until the next one that passes its argument checks
    DBuf st_tmp, st_ch, st_out; int64_t st_dots = -1;
    // fill_layers (fill.hip), which reads the resident masks and writes nothing of the raster chain or of the stroke passes.  With Z blocks of 64 samples
    // over the lines of both families and R runs: fl_tmp = mask u8[h w] (only of an explicit mask), on u64[Z + 1] = the ON bits, cs u64[Z + 1] = (run starts
    // << 32 | run ends) per block, sc u64[Z + 1] = its scan, FlCounters; fl_runs = a0 int[R], a1 int[R], row int[R] (the line, counted over both families),
    // keep u64[R + 1], kbase u64[R + 1] = its scan (the unit states both layouts), free between calls; fl_out = THE SEGMENT LIST, int4[fl_segs] = x0 y0 x1 y1
    // of the last call (-1: none) until the next one that passes its argument checks
    DBuf fl_tmp, fl_runs, fl_out; int64_t fl_segs = -1;
    // what the fill keeps for orip_fill_link (fill_link.hip), valid while fl_segs > 0: fl_rows = segrow int[fl_segs] = the row of every segment (a row is a line
    // of either family, the rows of the first family first) and rfirst unsigned[fl_nrows + 1] = the first segment of every row, rfirst[fl_nrows] = fl_segs;
    // fl_row1 = the first row of the second family (fl_nrows with one family): row q + 1 is "the next line" of row q unless it is fl_row1; fl_xmajor = the major
    // axis of either family.  The link pass, S = fl_segs, P pairs in reach: fk_tmp = mask u8[h w] (only of an explicit mask), cnt u64[S + 1] = pairs per END
    // and base u64[S + 1] = its scan, best u64[2 S] = least (d^2 << 32 | partner) per END and per START, link int[2 S] = next, prev, head int[2][S] = the two
    // arrays of the pointer jumping, len int[S] = members of the chain, at its head, cs u64[S + 1] = (points << 32 | 1) at a head and sc u64[S + 1] = its scan,
    // FkCounters; fk_pair = pairs uint2[P] (the unit states both layouts), free between calls; fk_out = THE LINK RESULT, off int64[fk_paths + 1], pts
    // int2[2 fk_segs] of the last orip_fill_link (fk_paths -1: none) until the next one that passes its argument checks or the next orip_fill_mask that does
    DBuf fl_rows; int64_t fl_nrows = 0, fl_row1 = 0; int fl_xmajor[2] = {0, 0};
    DBuf fk_tmp, fk_pair, fk_out; int64_t fk_paths = -1, fk_segs = 0;
    // fill stipple (fill_stipple.hip), which reads the resident masks and writes nothing of the raster chain, of the stroke passes, of the fill's segment
    // list or of the link result.  With Z blocks of 64 candidates over the lattice rows: fs_tmp = mask u8[h w] (only of an explicit mask), tone u8[h w] (only
    // with a tone image), dot u64[Z] = the verdicts, cnt u64[Z + 1] = dots per block, sc u64[Z + 1] = its scan, FsCounters (the unit states the layout), free
    // between calls; fs_out = THE DOT LIST, xy int2[fs_dots] of the last call (-1: none) until the next one that passes its argument checks
    DBuf fs_tmp, fs_out; int64_t fs_dots = -1;
    // svg2stream (svg.hip): scratch of the flattening and of the box, the resident paths (off int64[sv_n + 1], pts double2[sv_total]; raw units after
    // orip_svg_flatten, page mm after orip_svg_fit) until the next flatten; orip_gcode_to_steps reads them when it is called without pointers
    DBuf sv_tmp, sv_tmp2, sv_off, sv_pts; int64_t sv_n = 0, sv_total = 0; bool sv_ready = false, sv_box_ok = false; double sv_box[4] = {0, 0, 0, 0};
    // hatch fills (hatch_common.h: the frame; hatch.hip, hatch_angle.hip: the rules): sv_fitted = orip_svg_fit has run on the resident paths, sv_hatched =
    // orip_svg_hatch or orip_svg_hatch_angle has appended to them (both cleared by the next flatten).  Scratch, free between calls, carved by the frame for
    // either rule with that rule's records: ht_pts = the plan (HtPlan: the quantised points with their group and successor, the groups' boxes, the call's
    // counters, per group the lines' origin, count and first row, per edge the chunk counts and their scan); ht_rows = one direction's crossing counts and
    // offsets per row and the list of rows for the block sort; ht_x = its crossings, unsorted and sorted, with the pairs' flags and their scan
    DBuf ht_pts, ht_rows, ht_x; bool sv_fitted = false, sv_hatched = false;
    // resident after either hatch call: ht_grp int32[ht_nseg] = the caller's fill group of every appended hatch line (orip_svg_hatch_groups_fetch)
    DBuf ht_grp; int64_t ht_nseg = 0;
    // analyze_colors (analyze.hip): the 2^24-bin table of the image's colours, the kept colours in key order (keys u32[an_D], counts int64[an_D]) resident from
    // orip_colors_table until the next image or table; an_tmp = AnState + the compaction's block counts / offsets, an_km = the k-means inits, their segment
    // sums, mind2 int32[n_init, an_D] and labels u8[n_init, an_D] (free between calls)
    DBuf an_table, an_keys, an_counts, an_tmp, an_km; int64_t an_D = 0, an_kept = 0; bool an_ready = false;
    DBuf resize_src, resize_dst;                       // raster01.hip staging
    // profiling
    bool prof_on = false;
    std::map<std::string, ProfEntry> prof;
};

inline LaneGuard::LaneGuard(orip_ctx* ctx, int lane_id) : c(ctx), prev(orip_tls_lane), lane(lane_id), ok(true), owner(false) {
    if (prev != lane) { int expect = 0; ok = c->lane_owner[lane].compare_exchange_strong(expect, 1); owner = ok; }
    if (ok) orip_tls_lane = lane;
}
inline hipError_t orip_pf08_drain(orip_ctx* c) {           // the claimed lane's main stream goes on behind its pending prefetch
    LaneRes& l = LN(c);
    if (!l.pf08.pending) return hipSuccess;
    l.pf08.pending = false;
    return hipStreamWaitEvent(l.stream, l.ev3, 0);
}
inline LaneGuard::~LaneGuard() { if (ok) orip_tls_lane = prev; if (owner) c->lane_owner[lane].store(0); }
// lane 0's vtmp[VT0_EDGE_BITS]: two sets of bit planes, `nwords` words each.  Stage 03 leaves the edges in the first; stage 04 thins between the two.
static inline hipError_t orip_edge_planes(orip_ctx* c, size_t nwords, unsigned long long*& a, unsigned long long*& b) {
    Carve L; L.each(nwords, a, b); return L.commit(LN(c).vtmp[VT0_EDGE_BITS], 64);
}
// rocPRIM's query-then-run idiom, spelled once: run(tmp, bytes) is called with tmp == nullptr to learn the size, the lane's tmpF grows to it, then it runs
template <class F> static inline hipError_t orip_with_tmp(orip_ctx* c, F&& run) {
    size_t bytes = 0; hipError_t e = run((void*)nullptr, bytes);
    if (e == hipSuccess) e = LN(c).tmpF.ensure(bytes + 16);
    return e == hipSuccess ? run(LN(c).tmpF.p, bytes) : e;
}

// K bit planes of nw words each -> 0 / 255 byte planes, for rows that are multiples of 64 wide; enqueued on the calling lane's stream (raster02.hip)
void orip_bits_expand16(orip_ctx* c, const unsigned long long* bits, uint8_t* dst, size_t nw, int K);
// open (erode^n, dilate^n) then close (dilate^n, erode^n) of K planes, src -> dst, on bit planes when the input is binary; unpack == false leaves the
// result in c->morphed_bits only (raster02.hip; stage 03 opens and closes its masks with it)
int orip_morph_open_close(orip_ctx* c, const uint8_t* src, uint8_t* dst, int K, int shape, int k, int open_iters, int close_iters, bool labels_mode, bool unpack = true);
// Time one kernel launch with HIP events on ctx->stream when profiling is enabled (bench.py roofline leg).
struct ProfScope {
    orip_ctx* c; const char* name;
    bool armed = false;
    ProfScope(orip_ctx* ctx, const char* n) : c(ctx), name(n) { if (c->prof_on) armed = hipEventRecord(LN(c).ev0, LN(c).stream) == hipSuccess; }
    ~ProfScope() {
        if (!armed) return;
        float ms = 0;
        if (hipEventRecord(LN(c).ev1, LN(c).stream) != hipSuccess || hipEventSynchronize(LN(c).ev1) != hipSuccess ||
            hipEventElapsedTime(&ms, LN(c).ev0, LN(c).ev1) != hipSuccess) return;          // a failed timing is dropped, never recorded as 0 ms
        std::lock_guard<std::mutex> g(c->mu);
        auto& e = c->prof[name]; e.ms += ms; e.launches++;
    }
};

// raise a kernel's dynamic-LDS limit; the result is kept so that every caller (not only the one thread that ran the std::call_once) sees a failure
template <class F> static inline void orip_max_lds(F* kernel, int bytes, std::atomic<int>& err) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) err.store((int)e);
}
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// stage entry points implemented across the .hip files
int orip_raster02_lab_tables(orip_ctx* c);
// the Lab (02:35) or, rgb, the R, G, B bytes of the n pixels d_idx names in the resident image (a device list; nullptr: pixels 0 .. n - 1) -> dst, n
// triples in device memory; enqueued on the calling lane's stream (raster02.hip; the samples of kmeans02.hip)
void orip_raster02_gather(orip_ctx* c, bool rgb, const int64_t* d_idx, int64_t n, uint8_t* dst);
// the per-layer stages without the closing stream wait (orip_layer_front chains them on the layer's stream)
int orip_contours_layer_impl(orip_ctx* c, int layer, bool sync);
int orip_scale_vectors_impl(orip_ctx* c, int layer, float sx, float sy, float dx, float dy, bool sync);
int orip_sort_contours_impl(orip_ctx* c, int layer, bool sync, const orip_params08* prm_for_prefetch = nullptr);
// stage 08's order-independent front on the lane's side stream, called by stage 07 under its greedy chain with the features it has computed (vector08a.hip)
struct PolyFeat;
int orip_prefetch08(orip_ctx* c, const orip_params08& prm, DPolys& scaled, const PolyFeat* feat07);
// explicit points of a walk-coded list (no-op for explicit lists); on the calling lane's stream, not synchronised (vector_common.hip)
int orip_polys_materialize(orip_ctx* c, DPolys& P);
