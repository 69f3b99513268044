// tail_window.h -- the integer form of a window of k_tail_replay (vector08a.hip): float64 running sums with sequential rounding, without the sequential chain.
// Compiles with hipcc (device and host) and with g++ (tests/host/tail_window_harness.cpp), as walker.h does.
//
// While a running value p stays inside one binade [2^e, 2^(e+1)) it is a multiple of u = 2^(e-52), P = p / u an integer in [2^52, 2^53), and for any d
//     fl(p + d) = p + R(d),   R(d) = d rounded to a multiple of u,
// because the exact sum lies in a range where the doubles are exactly the multiples of u.  d / u = d * 2^(52-e) is exact (a power of two; a d that is subnormal,
// or a quotient of 2^53 or more, is an exception), so R(d) is an integer that does not depend on p -- unless d / u lies exactly half-way between two integers:
// then round-to-even looks at the parity of P.  Such a tie is no exception here: an operation is a pair of increments (for an even P, for an odd P), and
// two operations compose to such a pair again (tw_compose), so a window is an inclusive scan of pairs, six steps over a wave.  (Distances have ~5 more bits
// than u at the default tail length, so one operation in 32 is a tie: falling back on ties would take nearly every window.)
// What remains an exception: a partial sum S that is not strictly inside (2^52, 2^53) -- at 2^53 the sum leaves the binade, and a real sum just below 2^e
// rounds at u / 2 and may come out as 2^52 or below; an incoming value that is zero, subnormal, negative or not finite; a subnormal or huge operand.  The
// results are exact up to the first exception, which tw_window reports; the caller falls back to real additions from there (k_tail_replay: for the window).
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define TW_FN __host__ __device__ __forceinline__
#else
#define TW_FN inline
#endif

struct TwInc { long long ev, od; };      // the increment of P, in units of u, when P is even / odd

TW_FN unsigned long long tw_bits(double x) { unsigned long long b; __builtin_memcpy(&b, &x, 8); return b; }
TW_FN double tw_double(unsigned long long b) { double x; __builtin_memcpy(&x, &b, 8); return x; }
// the frame of an incoming value: false for zero, subnormals, negatives, infinities, NaN and exponents whose scale factor would not be a normal double
TW_FN bool tw_frame(double p, int& e, long long& P) {
    const unsigned long long b = tw_bits(p), ef = b >> 52;      // (the sign bit makes ef >= 2048)
    if (ef < 123u || ef > 1923u) return false;                  // |e| <= 900
    e = (int)ef - 1023; P = (long long)((b & 0xfffffffffffffull) | (1ull << 52));
    return true;
}
// one operation in the frame of exponent e; false: exception (subnormal, not finite, or 2^53 units and more)
TW_FN bool tw_inc(double d, int e, TwInc& f) {
    f.ev = f.od = 0;
    if (d == 0.0) return true;
    const unsigned long long ef = (tw_bits(d) >> 52) & 0x7ffu;
    if (ef == 0u || ef == 0x7ffu) return false;
    const double s = d * tw_double((unsigned long long)(52 - e + 1023) << 52);      // d / u: exact wherever it is a normal number, and below 1/2 otherwise
    if (!(fabs(s) < 9007199254740992.0)) return false;
    const double r = rint(s);                                   // to nearest, ties to even
    if (fabs(s - r) == 0.5) {                                   // (s - r is exact) half-way: P + floor(s) or the integer above it, whichever is even
        const long long m = (long long)floor(s), odd = m & 1;
        f.ev = m + odd; f.od = m + 1 - odd;
    } else f.ev = f.od = (long long)r;
    return true;
}
// f, then g
TW_FN TwInc tw_compose(TwInc f, TwInc g) {
    TwInc h;
    h.ev = f.ev + ((f.ev & 1) ? g.od : g.ev);
    h.od = f.od + ((f.od & 1) ? g.ev : g.od);
    return h;
}
TW_FN long long tw_apply(long long P, TwInc f) { return P + ((P & 1) ? f.od : f.ev); }
TW_FN bool tw_inside(long long S) { return S > (1ll << 52) && S < (1ll << 53); }
TW_FN double tw_value(long long S, int e) { return tw_double(((unsigned long long)(e + 1023) << 52) | ((unsigned long long)S & 0xfffffffffffffull)); }      // S inside

// The window on the host, lanes as a loop: out[i] = the running value after operation i.  Returns n, or the first lane x whose value is an exception
// (out[0 .. x) are final, x = 0 for an incoming value without a frame).
inline int tw_window(double p, const double* ops, int n, double* out) {
    int e; long long P;
    if (!tw_frame(p, e, P)) return 0;
    TwInc acc = {0, 0};
    for (int i = 0; i < n; i++) {
        TwInc f;
        if (!tw_inc(ops[i], e, f)) return i;
        acc = tw_compose(acc, f);
        const long long S = tw_apply(P, acc);
        if (!tw_inside(S)) return i;
        out[i] = tw_value(S, e);
    }
    return n;
}
