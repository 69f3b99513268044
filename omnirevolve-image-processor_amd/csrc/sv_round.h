// csrc/sv_round.h -- the unfused double arithmetic and the 4-decimal rounding that svg.hip (the fit) and the hatch fills (hatch_common.h: the quantisation and the hatch lines' end points; hatch.hip: the crossings) share
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double sv_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double sv_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sv_sub(double a, double b) { return __dsub_rn(a, b); }
// float(f"{v:.4f}"): the integer k nearest to the EXACT v * 10^4, ties to even, divided by 10^4 in one correctly rounded division (svg.hip, 3.)
__device__ __forceinline__ double sv_round4(double v) {
    const double p = sv_mul(v, 1e4), e = __fma_rn(v, 1e4, -p);
    double k = rint(p);
    const double r = sv_sub(p, k);                                           // exact
    if (r == 0.5 && e > 0.0) k = sv_add(k, 1.0);
    else if (r == -0.5 && e < 0.0) k = sv_sub(k, 1.0);
    return __ddiv_rn(k, 1e4);
}
