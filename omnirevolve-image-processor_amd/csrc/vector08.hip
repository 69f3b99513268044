// csrc/vector08.hip -- the entry points of stage 08 (08_dedup_layer_basic.py process_layer, 08:484-557) on gfx950: orip_dedup_layer runs stage 08-A
// (vector08a.hip: greedy virtual draw, all samples in parallel), stage 08-B (vector08b.hip: skeleton merge of the lines that remain) and the travel
// reorder of the result on the layer's lane; orip_layer_front chains stages 04 .. 08 of one layer in one call.
#include "vec08.h"

extern "C" int orip_dedup_layer(orip_ctx* c, int layer, const orip_params08* prm) {
    orip_enter(c);
    if (!prm || layer < 0 || layer >= ORIP_MAX_LAYERS) ORIP_FAIL(c, "bad arguments");
    const orip_params08 P = *prm;
    const int W = P.W, H = P.H;
    ORIP_LANE_NODRAIN(c, layer + 1);       // stage 08 waits for the parts of its prefetch where it picks them up (split_small, A2)
    if (W <= 0 || H <= 0 || W > 16383 || H > 16383) ORIP_FAIL(c, "canvas %dx%d out of range", W, H);
    if (!(P.sample_step * 2.0 < P.max_jump)) ORIP_FAIL(c, "dedup_sample_step must be < max_join_jump_px / 2 (stage-A segments are assumed jump-free)");
    DPolys& S = c->polys[ORIP_SLOT_SORTED][layer]; DPolys& OUT = c->polys[ORIP_SLOT_LINES_INTRA][layer]; DTaps& TOUT = c->taps[ORIP_TAPS_INTRA][layer];
    TOUT.n = 0;
    HIPC(c, OUT.clear(LN(c).stream));
    HIPC(c, TOUT.xy.ensure(64));
    if (S.n == 0) return 0;
    DPolys& kept0 = LN(c).tp[0]; DPolys& cleaned = LN(c).tp[1]; DPolys& lines2 = LN(c).tp[2]; DPolys& merged = LN(c).tp[3];
    for (DPolys* t : {&kept0, &cleaned, &lines2, &merged}) { t->n = 0; t->total = 0; t->set_explicit(); }
    bool caps_counted = false; PhaseTimer T(c, "ORIP_TIME08");        // debug: per-phase wall times of this layer (adds stream syncs)
    ORIP_TRY(dedup08_a(c, layer, P, S, TOUT, T, caps_counted));
    T.tick("A7");
    DPolys* fin = &lines2;
    if (P.post_on && lines2.n > 0) { ORIP_TRY(dedup08_b(c, P, T)); fin = &merged; }
    T.tick("gather");
    // ---- C
    ORIP_TRY(vreorder(c, *fin, OUT, 8));
    unsigned h_dist = 0; if (caps_counted) HIPC(c, hipMemcpyAsync(&h_dist, &LN(c).flags.as<LaneFlags>()->caps_distinct, 4, hipMemcpyDeviceToHost, LN(c).stream));
    HIPC(c, hipStreamSynchronize(LN(c).stream));
    if (caps_counted) { LN(c).caps_hint = h_dist; if (T.on) { char b[48]; snprintf(b, sizeof b, " [caps distinct %u]", h_dist); T.log += b; } }
    T.tick("reorder");
    if (T.on) fprintf(stderr, "[time08] layer %d (in %lld polys %lld pts, kept %lld pts, cleaned %lld/%lld, lines2 %lld/%lld):%s\n", layer, (long long)S.n, (long long)S.total, (long long)kept0.total, (long long)cleaned.n, (long long)cleaned.total, (long long)lines2.n, (long long)lines2.total, T.log.c_str());
    return 0;
}

// The front of one layer's pipeline in ONE call: orip_contours_layer -> orip_scale_vectors -> [orip_sort_contours -> [orip_dedup_layer]] (upto = 5, 7
// or 8) on the layer's lane.  Same results as the four calls; what goes away are the returns to the (Python) caller between the stages of a resident
// chain -- three hand-overs per layer, each 0.2-0.5 ms of idle stream on the critical layer.
extern "C" int orip_layer_front(orip_ctx* c, int layer, float sx, float sy, float dx, float dy, int upto, const orip_params08* prm) {
    orip_enter(c);
    if (upto >= 8 && !prm) ORIP_FAIL(c, "stage 08 needs its parameters");
    ORIP_TRY(orip_contours_layer_impl(c, layer, false));
    ORIP_TRY(orip_scale_vectors_impl(c, layer, sx, sy, dx, dy, upto < 7));
    if (upto >= 7) ORIP_TRY(orip_sort_contours_impl(c, layer, upto < 8, upto >= 8 ? prm : nullptr));
    if (upto >= 8) ORIP_TRY(orip_dedup_layer(c, layer, prm));
    return 0;
}
