// tests/host/tail_window_harness.cpp -- csrc/tail_window.h against plain sequential double additions (TEST INFRASTRUCTURE; g++, CPU only).
// usage: tail_window_harness [random windows, default 3000000].  Exit status 0 and a line "ok ..." when everything holds.
// For every window: the lanes tw_window calls final equal the sequential sums bit for bit; the lane it stops at is an exception by the header's own
// definition, and for the crafted windows it is the lane the case is built to stop at.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdint>
#include "../../omnirevolve-image-processor_amd/csrc/tail_window.h"

static unsigned long long rs = 0x9e3779b97f4a7c15ull;
static unsigned long long rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static long long fails = 0;
static unsigned long long bits(double x) { unsigned long long b; memcpy(&b, &x, 8); return b; }

// returns the exception lane; checks the final lanes against the sequential sums
static int check(const char* what, double p, const double* ops, int n, int want_x = -1) {
    double out[64], seq[64]; volatile double acc = p;
    for (int i = 0; i < n; i++) { acc = acc + ops[i]; seq[i] = acc; }
    const int x = tw_window(p, ops, n, out);
    for (int i = 0; i < x; i++)
        if (bits(out[i]) != bits(seq[i])) { if (fails++ < 10) fprintf(stderr, "%s: lane %d of %d: %.17g, sequential %.17g (p %.17g)\n", what, i, n, out[i], seq[i], p); break; }
    if (want_x >= 0 && x != want_x) { if (fails++ < 10) fprintf(stderr, "%s: stops at lane %d, expected %d\n", what, x, want_x); }
    return x;
}

int main(int argc, char** argv) {
    const long long N = argc > 1 ? atoll(argv[1]) : 3000000;
    long long full = 0, lanes = 0, ties = 0;
    // ---- random windows: pushes and pops in turn, as the replay makes them, the value hovering in [64, 128), around 64.0 and around 128.0
    for (long long w = 0; w < N; w++) {
        const int kind = (int)(w % 4);
        const double centre = kind == 0 ? 120.0 : kind == 1 ? 96.0 : kind == 2 ? 64.0 : 128.0, T = centre;
        double p = centre + (uni() - 0.5) * (kind < 2 ? 8.0 : 1e-3 * (1 + (rnd() & 1023)));
        if (rnd() % 64 == 0) p = centre;
        const int n = 1 + (int)(rnd() % 64);
        double ops[64]; double v = p;
        for (int i = 0; i < n; i++) {
            double d = (rnd() % 8 == 0) ? (double)(1 + rnd() % 3) : 0.25 + 2.5 * uni();
            if (rnd() % 16 == 0) d = ldexp((double)(rnd() & 0xffff) + 0.5, -46 - (int)(rnd() % 2));      // half-way patterns at the ulp of [64, 128) and of [32, 64)
            if (rnd() % 512 == 0) d = 0.0;
            ops[i] = v > T ? -d : d; v += ops[i];
        }
        const int x = check("random", p, ops, n);
        full += x == n; lanes += x;
        int e; long long P;
        if (tw_frame(p, e, P)) for (int i = 0; i < x; i++) { TwInc f; tw_inc(ops[i], e, f); ties += f.ev != f.od; }
    }
    // ---- crafted windows
    const double u = ldexp(1.0, -46);                     // the ulp of [64, 128)
    { double ops[4] = {2.0 + 0.5 * u, 2.0 + 0.5 * u, -(1.0 + 1.5 * u), 0.5 * u};      // exact ties, from an even and from an odd P
      check("ties, even P", 100.0, ops, 4, 4); check("ties, odd P", 100.0 + u, ops, 4, 4);
      check("ties, odd P below", 100.0 - u, ops, 4, 4); }
    { double ops[3] = {20.0, 8.0, 1.0}; check("reaches 2^(e+1) exactly", 100.0, ops, 3, 1); }
    { double ops[2] = {28.0 - u, u}; check("one ulp below 2^(e+1), then onto it", 100.0, ops, 2, 1); }
    { double ops[2] = {-(6.0 - 0.75 * u), 1.0}; check("within half an ulp of 2^e from above", 70.0, ops, 2, 2); }       // 64 + 0.75 u: rounds to 64 + u, inside
    { double ops[2] = {-(6.0 + 0.25 * u), 1.0}; check("within half an ulp of 2^e from below", 70.0, ops, 2, 0); }       // 64 - 0.25 u: a double of the binade below
    { double ops[2] = {-(6.0 - 0.25 * u), 1.0}; check("a quarter ulp above 2^e", 70.0, ops, 2, 0); }                    // rounds to 2^e: the frame's edge, refused
    { double ops[2] = {-6.0, 1.0}; check("onto 2^e exactly", 70.0, ops, 2, 0); }
    { double ops[2] = {3.0, -1.0}; check("incoming 2^e, upwards", 64.0, ops, 2, 2); }
    { double ops[2] = {2.0, 2.0}; check("incoming 0.0", 0.0, ops, 2, 0); }
    { double ops[3] = {0.0, 2.0, -0.0}; check("a push of 0.0", 100.0, ops, 3, 3); }
    { double ops[1] = {1.5}; check("one operation", 100.0, ops, 1, 1); }
    { double ops[1] = {4.9406564584124654e-324}; check("a subnormal operand", 100.0, ops, 1, 0); check("a subnormal incoming value", 4.9406564584124654e-324, ops, 1, 0); }
    { double ops[64]; for (int i = 0; i < 64; i++) ops[i] = (i & 1) ? -(1.75 + i * 0.37 * u) : 1.75 + i * 0.61 * u; check("64 operations", 119.0, ops, 64, 64); }
    { double ops[1] = {1.0}; check("a negative incoming value", -100.0, ops, 1, 0); check("infinity", INFINITY, ops, 1, 0); }
    if (fails) { fprintf(stderr, "%lld failures\n", fails); return 1; }
    printf("ok: %lld random windows, %lld whole, %lld final lanes, %lld ties among them\n", N, full, lanes, ties);
    return full * 4 > N && ties > 0 ? 0 : 2;
}
