// csrc/sv_place.h -- where the flatteners put their points (svg.hip: orip_svg_flatten; gcode_arc.hip: orip_gcode_flatten): segment s of a subpath emits cnt[s]
// points behind its first one, ex = the exclusive scan of cnt over all segments, and every subpath adds its own first point in front of its segments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
// off[p] = place of subpath p's first point: the pieces before its first segment, and one first point per subpath before it
__global__ __launch_bounds__(256) void k_svg_off(const long long* __restrict__ sub_off, int64_t P, const long long* __restrict__ ex, long long* __restrict__ off) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p <= P) off[p] = ex[sub_off[p]] + p;
}

// first[s] = place of the point i = 1 of segment s
__global__ __launch_bounds__(256) void k_svg_first(const long long* __restrict__ sub_off, int64_t P, int64_t S, const long long* __restrict__ ex, long long* __restrict__ first) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    int64_t lo = 0, hi = P;                                                  // last p with sub_off[p] <= s
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (sub_off[mid] <= s) lo = mid; else hi = mid; }
    first[s] = ex[s] + lo + 1;
}
}  // namespace
