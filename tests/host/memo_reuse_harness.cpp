// tests/host/memo_reuse_harness.cpp -- TEST INFRASTRUCTURE, a stand-alone program.  Runs the product's serial walker (csrc/walker.h) over PAIRS of
// consecutive skeleton maps with ONE memo vector and ONE log buffer kept across the pair, as stage 04 keeps its memo planes and walk logs from step to
// step without clearing them as a whole (WalkArgs::memo).  Both are sized for the larger run of the pair, so a stale memo word always points inside the
// allocation.  Between the two runs
//   mode "clear"    zeroes the eight memo words of every skeleton pixel of the second map and nothing else: what k_clear_memo_layer does on the device;
//   mode "noclear"  zeroes nothing: the negative control, run on the CPU only.
// The contours of the second run of every pair go to the output file; tests/test_memo_reuse_host.py compares them with the oracle.  The preparation
// around the walker (components, state bytes, keys) is the plain host re-implementation of tests/host/walk_harness.cpp.
//
//   memo_reuse_harness <in> <out> clear|noclear
//   in : int32 n_maps, then per map int32 H, int32 W, H * W bytes; int32 n_pairs, then per pair int32 first, int32 second
//   out: per pair int32 rc (0 ok, 1 output too large, 2 log overflow), int64 n_paths, int64 n_pts, (n_paths + 1) int64 offsets, 2 * n_pts int32 x, y
#include <vector>
#include <algorithm>
#include <cstring>
#include <cstdint>
#include <cstdio>
#include <string>
#include "../../omnirevolve-image-processor_amd/csrc/walker.h"

namespace {
struct Map { int H = 0, W = 0; std::vector<uint8_t> px; };

// everything a run needs besides the memo and the log: components (root = minimum block-raster id), state bytes, the pixel list sorted by component
struct Prep {
    int H, W; unsigned M = 0, NC = 0;
    std::vector<uint8_t> st; std::vector<unsigned> keys, lin, cs;
    explicit Prep(const Map& m) : H(m.H), W(m.W) {
        const uint8_t* skel = m.px.data();
        const size_t N = (size_t)H * W;
        st.assign(N, 0);
        std::vector<int> root(N, -1);
        const int Wb = (W + 1) / 2;
        auto pid = [&](int y, int x) { return (((y >> 1) * Wb + (x >> 1)) << 2) | ((y & 1) << 1) | (x & 1); };
        std::vector<size_t> stack, members;
        for (size_t s = 0; s < N; s++) {
            if (!skel[s] || root[s] >= 0) continue;
            members.clear(); stack.push_back(s); root[s] = 0; int best = 1 << 30;
            while (!stack.empty()) {
                size_t i = stack.back(); stack.pop_back(); members.push_back(i);
                int y = (int)(i / W), x = (int)(i % W); best = std::min(best, pid(y, x));
                for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
                    int yy = y + dy, xx = x + dx; if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                    size_t j = (size_t)yy * W + xx; if (skel[j] && root[j] < 0) { root[j] = 0; stack.push_back(j); }
                }
            }
            for (size_t i : members) root[i] = best;
        }
        std::vector<std::pair<unsigned, unsigned>> kl;
        for (size_t i = 0; i < N; i++) if (skel[i]) {
            int y = (int)(i / W), x = (int)(i % W), deg = 0;
            for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) { if (!dy && !dx) continue; int yy = y + dy, xx = x + dx; if (yy >= 0 && yy < H && xx >= 0 && xx < W && skel[(size_t)yy * W + xx]) deg++; }
            st[i] = ST_FG | (deg == 1 ? ST_END : 0) | (deg >= 3 ? ST_JUN : 0);
            kl.push_back({(unsigned)root[i], (unsigned)i});
        }
        std::stable_sort(kl.begin(), kl.end(), [](auto& a, auto& b) { return a.first < b.first; });
        M = (unsigned)kl.size(); keys.resize(M); lin.resize(M);
        for (unsigned i = 0; i < M; i++) { keys[i] = kl[i].first; lin[i] = kl[i].second; if (i == 0 || keys[i] != keys[i - 1]) cs.push_back(i); }
        NC = (unsigned)cs.size(); cs.push_back(M);
    }
    size_t memo_words() const { return (size_t)H * W * 8; }
    size_t log_words(unsigned F) const { return ((size_t)F * M + 64 * (size_t)NC + 8) * 4; }
};

const unsigned F = 16;

struct Result { int rc = 0; std::vector<int64_t> off; std::vector<int32_t> pts; };

// one trace + write pass over the caller's memo and log (neither is touched here before the walker runs)
Result run(Prep& P, std::vector<unsigned>& memo, std::vector<unsigned>& logbuf) {
    Result R; R.off.assign(1, 0);
    const unsigned M = P.M, NC = P.NC;
    if (!M) return R;
    WalkArgs A; memset(&A, 0, sizeof(A));
    A.H = P.H; A.W = P.W; A.plane = (int64_t)P.H * P.W; A.st = P.st.data(); A.keys = P.keys.data(); A.lin = P.lin.data(); A.comp_start = P.cs.data(); A.nc = NC;
    A.total_fg[0] = M; A.comp_order = nullptr;
    std::vector<uint8_t> steplog((size_t)F * M + 256 * (size_t)NC + 8, 0);
    std::vector<WalkInfo> winfo((size_t)2 * M); memset(winfo.data(), 0, winfo.size() * sizeof(WalkInfo));
    int over = 0;
    A.memo = memo.data(); A.logbuf = logbuf.data(); A.steplog = steplog.data(); A.cap_factor = F; A.winfo = winfo.data(); A.overflow = &over;
    for (unsigned c = 0; c < NC; c++) trace_component(A, c);
    if (over) { R.rc = 2; return R; }
    const unsigned nslots = 2 * M;
    for (unsigned i = 0; i < nslots; i++) walk_close_tail(A, PlainReader(), i, winfo[i]);
    std::vector<unsigned long long> pts_off(nslots + 1, 0); std::vector<unsigned> path_off(nslots + 1, 0);
    for (unsigned i = 0; i < nslots; i++) { pts_off[i + 1] = pts_off[i] + winfo[i].len_kept; path_off[i + 1] = path_off[i] + (winfo[i].len_kept ? 1u : 0u); }
    const unsigned long long total = pts_off[nslots];
    if (total > 50000000ull) { R.rc = 1; return R; }
    R.off.assign((size_t)path_off[nslots] + 1, 0); R.pts.assign((size_t)total * 2 + 2, 0);
    A.pts_off = pts_off.data(); A.path_off = path_off.data(); A.pts[0] = R.pts.data(); A.off[0] = R.off.data();
    std::vector<unsigned> kept; std::vector<unsigned long long> kept_off;
    for (unsigned i = 0; i < nslots; i++) if (winfo[i].len_kept) { kept.push_back(i); kept_off.push_back(pts_off[i]); }
    const unsigned long long chunk = 1000;
    for (unsigned long long p0 = 0; p0 < total; p0 += chunk) write_chunk(A, 0, kept.data(), kept_off.data(), (unsigned)kept.size(), p0, std::min(total, p0 + chunk));
    R.pts.resize((size_t)total * 2);
    return R;
}

template <class T> bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> void wr(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s <in> <out> clear|noclear\n", argv[0]); return 64; }
    const bool clear = std::string(argv[3]) == "clear";
    FILE* in = fopen(argv[1], "rb"); if (!in) { perror(argv[1]); return 65; }
    int32_t n_maps = 0; if (!rd(in, &n_maps, 1) || n_maps < 1 || n_maps > 4096) return 66;
    std::vector<Map> maps((size_t)n_maps);
    for (Map& m : maps) {
        int32_t hw[2]; if (!rd(in, hw, 2) || hw[0] < 1 || hw[1] < 1 || hw[0] > 4096 || hw[1] > 4096) return 66;
        m.H = hw[0]; m.W = hw[1]; m.px.resize((size_t)m.H * m.W);
        if (!rd(in, m.px.data(), m.px.size())) return 66;
    }
    int32_t n_pairs = 0; if (!rd(in, &n_pairs, 1) || n_pairs < 0 || n_pairs > 65536) return 66;
    std::vector<int32_t> pairs((size_t)n_pairs * 2);
    if (!rd(in, pairs.data(), pairs.size())) return 66;
    fclose(in);
    FILE* out = fopen(argv[2], "wb"); if (!out) { perror(argv[2]); return 65; }
    for (int32_t p = 0; p < n_pairs; p++) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || a >= n_maps || b < 0 || b >= n_maps) return 66;
        Prep PA(maps[a]), PB(maps[b]);
        // ONE memo and ONE log for both runs, sized for the larger: the first run starts from zeros (a fresh allocation), the second from what it left
        std::vector<unsigned> memo(std::max(PA.memo_words(), PB.memo_words()), 0u), logbuf(std::max(PA.log_words(F), PB.log_words(F)), 0u);
        Result r1 = run(PA, memo, logbuf);
        if (r1.rc) return 67;                                      // the first run is an ordinary one: it must go through
        if (clear)
            for (unsigned i = 0; i < PB.M; i++) memset(&memo[(size_t)PB.lin[i] * 8], 0, 8 * sizeof(unsigned));
        Result r2 = run(PB, memo, logbuf);
        const int32_t rc = r2.rc; const int64_t np = (int64_t)r2.off.size() - 1, nt = (int64_t)r2.pts.size() / 2;
        wr(out, &rc, 1); wr(out, &np, 1); wr(out, &nt, 1); wr(out, r2.off.data(), r2.off.size()); wr(out, r2.pts.data(), r2.pts.size());
    }
    fclose(out);
    printf("ok: %d pairs, %s\n", (int)n_pairs, clear ? "the second map's words cleared" : "nothing cleared");
    return 0;
}
