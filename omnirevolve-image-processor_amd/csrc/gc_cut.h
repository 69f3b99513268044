// csrc/gc_cut.h -- the output frame of the CUTTING PASSES, stated once: --dedup (gcode_dedup.hip), --occlude (gcode_occlude.hip) and --dashes / --dash-mm
// (gcode_dash.hip).  Each takes the resident step polylines, cuts segments into pieces and compacts the pieces into new strokes: (off, pts), origin = the
// input stroke of every output stroke, and the sources gathered through origin.  What a pass keeps between calls is one GcCut; what its kernels write into
// is one GcCutOut; how a piece finds its place is below; the host side (defined in gcode.hip) is the intake, the hand-over and the origin fetch.
// orip_ctx.h states the contract these keep and includes this file behind DBuf: a unit includes orip_ctx.h, never this file on its own.
#pragma once

struct orip_ctx;

// One pass's result record.  off / pts: its output, swapped with gc_off / gc_pts when a call succeeds; src: the gathered sources, swapped with gc_src then;
// res: origin int32[paths] of the pass's last call (paths -1: none) until its next one.  A record per pass, not one shared: whatever other pass runs in
// between, the origin stays fetchable, and each pass keeps the capacity it grew.
struct GcCut {
    DBuf off, pts, src, res; int64_t paths = -1;
    void release() { off.release(); pts.release(); src.release(); res.release(); }
};

// where the kernels of a pass write: the record's buffers, the sources to gather from (NULL: they no longer name the strokes) and the two capacities
struct GcCutOut { int2* pts; long long* off; int* origin; int* src; const int* src_in; long long cap_pts, cap_paths; };

// The per-segment record of the compaction: the kept pieces, whether the first one starts at the segment's first vertex (FA) and the last one ends at its
// second (FB).  Bit 29 is the pass's own (the dedup: a wave took the segment; the occlusion: the segment is whole) and k_gc_cut_compact does not look at it.
constexpr unsigned GC_CUT_NP = (1u << 29) - 1, GC_CUT_OWN = 1u << 29, GC_CUT_FA = 1u << 30, GC_CUT_FB = 1u << 31;

// the closing offset, from the scan's last word tot = (points << 32) | strokes
__device__ __forceinline__ void gc_cut_close(const GcCutOut& o, unsigned long long tot) {
    if ((long long)(unsigned)tot <= o.cap_paths) o.off[(unsigned)tot] = (long long)(tot >> 32);
}
// stroke sid starts at point `at` and comes from input stroke `path`; the caller has checked sid and at
__device__ __forceinline__ void gc_cut_start(const GcCutOut& o, long long sid, long long at, int path) {
    o.off[sid] = at; o.origin[sid] = path;
    if (o.src_in) o.src[sid] = o.src_in[path];
}
// Piece t of the nk kept pieces of a segment, a -> b in drawing order, where the scan's word (pbase points, sbase strokes) says.  cont: the segment's first
// piece continues the stroke of the segment before it, so it adds its end point only and starts no stroke.  false: out of place, nothing written -- the
// caller sets its own BAD_PLACE bit.
__device__ __forceinline__ bool gc_cut_piece(const GcCutOut& o, long long pbase, long long sbase, bool cont, unsigned t, unsigned nk, int path, int2 a, int2 b) {
    long long at = pbase + (cont ? (t ? 2ll * t - 1 : 0) : 2ll * t);
    const bool starts = !(cont && t == 0);
    const long long sid = sbase + t - (cont ? 1 : 0);
    if (t >= nk || at < 0 || at + (starts ? 2 : 1) > o.cap_pts || (starts && (sid < 0 || sid >= o.cap_paths))) return false;
    if (starts) { o.pts[at] = a; gc_cut_start(o, sid, at, path); at++; }
    o.pts[at] = b;
    return true;
}

// cs[g] = (points << 32) | strokes started, cs[S] = 0, from rec[g] and sinfo[g].y = the segment's stroke: a piece starts a stroke unless it is its segment's
// first, starts at the segment's first vertex, and the segment before it in the stroke still reaches that vertex.  Grid: cdiv(S + 1, 256) blocks of 256.
__global__ __launch_bounds__(256) void k_gc_cut_compact(int64_t S, const unsigned* __restrict__ rec, const int2* __restrict__ sinfo, unsigned long long* __restrict__ cs);

// ---- host side, defined in gcode.hip; `who` is the entry point's __func__, as for the gc_* helpers of gc_convert.h.  Everything on the calling lane's stream
// the 64-bit exclusive scan that places points and numbers strokes: out[i] = in[0] + .. + in[i - 1], count words
hipError_t gc_scan_u64(orip_ctx* c, unsigned long long* in, unsigned long long* out, size_t count);
// the scan's last word, read back: how many strokes and points the pass leaves
static inline void gc_cut_totals(unsigned long long tot, int64_t& paths, int64_t& points) { paths = (int64_t)(tot & 0xFFFFFFFFu); points = (int64_t)(tot >> 32); }
// n == 0, nothing to launch: the explicit form leaves the empty list resident, with gc_merged under the intake's rule; the record holds no strokes
int gc_cut_empty(orip_ctx* c, const char* who, GcCut& r, bool explicit_in);
// The intake, behind every check of the arguments: the record holds no result from here to the publish; an explicit input (off != NULL) becomes the resident
// list, and when it is not of the resident count it cannot be the polylines the sources name, so gc_merged is set.  sources: gc_src names the input strokes
int gc_cut_intake(orip_ctx* c, const char* who, GcCut& r, const int64_t* off, const int32_t* pts, int64_t n, int64_t total, bool& sources);
// room for cap_paths strokes of cap_pts points in the record's four buffers, and the kernels' view of them
int gc_cut_ensure(orip_ctx* c, const char* who, GcCut& r, long long cap_paths, long long cap_pts);
GcCutOut gc_cut_out(orip_ctx* c, const GcCut& r, bool sources, long long cap_pts, long long cap_paths);
// the hand-over: the record's strokes become the resident list, with their gathered sources while the sources name strokes; origin stays in the record
void gc_cut_publish(orip_ctx* c, GcCut& r, bool sources, int64_t paths, int64_t points);
// a whole _fetch entry point: origin of the pass's last call; `pass` is the subject of "no result: <pass> has not succeeded since the last failure"
int gc_cut_fetch(orip_ctx* c, const char* who, const GcCut& r, const char* pass, int32_t* origin);
