// csrc/hatch_common.h -- what the two hatch fills share (hatch.hip: the reference's rule along X and Y; hatch_angle.hip: ours, exact, along any direction):
// the limits, the call's counters, floor division, the rows' classes for the sort, and the intake of a call (state, arguments, the fill groups renumbered).
// Both units run the same scaffolding -- group boxes, a scan of the line counts, edge chunks of HT_CHUNK lines, count / scan / fill through row cursors, a
// sort inside each row by its class, pair, scan, emit -- on their own crossing records.
#pragma once
#include "vec_common.h"
#include <vector>

namespace {
constexpr unsigned HT_WAVE_MAX = 64, HT_BLOCK_MAX = 2048;
constexpr int HT_CHUNK = 64;
constexpr int64_t HT_MAX_ROWS = 1ll << 26, HT_MAX_CROSSINGS = 1ll << 30, HT_MAX_POINTS = (1ll << 30) - 1;     // the last: what orip_gcode_to_steps accepts
constexpr double HT_MAX_SPM = 5000.0;

struct HtCounters { unsigned long long crossings; unsigned n_med, n_big; int err; int pad; };

__host__ __device__ __forceinline__ long long ht_floordiv(long long a, long long b) { const long long q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }     // b > 0

// rows for the block sort go on a list (in any order); rows beyond it are counted: a non-zero count calls the large sort.  rowcnt[R] = 0 closes the scan
__global__ __launch_bounds__(256) void k_ht_classify(unsigned* __restrict__ rowcnt, int64_t R, unsigned* __restrict__ medlist, HtCounters* __restrict__ cn) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > R) return;
    if (r == R) { rowcnt[r] = 0; return; }
    const unsigned n = rowcnt[r];
    if (n > HT_BLOCK_MAX) atomicAdd(&cn->n_big, 1u);
    else if (n > HT_WAVE_MAX) { const unsigned i = atomicAdd(&cn->n_med, 1u); if (i < R) medlist[i] = (unsigned)r; }
}

// The intake of either hatch call, behind `stats` being cleared: the state, the arguments both take, and the groups in use renumbered 0 .. G - 1 in
// ascending order of their number (gid[p]: the rank of subpath p's group or -1; gnum[rank]: the caller's number).
struct HtGroups { std::vector<int32_t> gid, gnum; int64_t G = 0; };
inline int ht_intake(orip_ctx* c, const char* who, const int32_t* fill_group, int64_t n_sub, double steps_per_mm, int32_t spacing, int32_t inset, int32_t flags, HtGroups& g) {
    if (!c->sv_ready || !c->sv_fitted) ORIP_FAIL_AS(c, who, "no fitted paths: orip_svg_flatten and orip_svg_fit come first");
    if (c->sv_hatched) ORIP_FAIL_AS(c, who, "the resident paths are hatched already: flatten again first");
    if (n_sub != c->sv_n) ORIP_FAIL_AS(c, who, "%lld fill groups given, %lld paths resident", (long long)n_sub, (long long)c->sv_n);
    if (!(steps_per_mm > 0.0) || !(steps_per_mm <= HT_MAX_SPM)) ORIP_FAIL_AS(c, who, "steps per mm %g: hatching needs a value in (0, 5000], so that four decimals of a mm name every step", steps_per_mm);
    if (spacing < 1) ORIP_FAIL_AS(c, who, "hatch spacing %d steps: at least 1", spacing);
    if (inset < 0) ORIP_FAIL_AS(c, who, "hatch inset %d steps: at least 0", inset);
    if (!(flags & (ORIP_HATCH_HORIZONTAL | ORIP_HATCH_VERTICAL)) || (flags & ~(ORIP_HATCH_SERPENTINE | ORIP_HATCH_HORIZONTAL | ORIP_HATCH_VERTICAL)))
        ORIP_FAIL_AS(c, who, "flags %d: ORIP_HATCH_HORIZONTAL, ORIP_HATCH_VERTICAL or both, and ORIP_HATCH_SERPENTINE", flags);
    g.gid.assign((size_t)n_sub, -1);
    std::vector<int32_t> rank((size_t)n_sub, 0);
    for (int64_t p = 0; p < n_sub; p++) {
        if (fill_group[p] < -1 || fill_group[p] >= n_sub) ORIP_FAIL_AS(c, who, "subpath %lld: fill group %d of %lld", (long long)p, fill_group[p], (long long)n_sub);
        if (fill_group[p] >= 0) rank[fill_group[p]] = 1;
    }
    g.G = 0;
    for (int64_t k = 0; k < n_sub; k++) { const int32_t used = rank[k]; rank[k] = (int32_t)g.G; g.G += used; }
    for (int64_t p = 0; p < n_sub; p++) if (fill_group[p] >= 0) g.gid[p] = rank[fill_group[p]];
    g.gnum.assign((size_t)g.G, 0);                                             // rank -> the caller's number
    for (int64_t p = 0; p < n_sub; p++) if (g.gid[p] >= 0) g.gnum[g.gid[p]] = fill_group[p];
    return 0;
}
}  // namespace
