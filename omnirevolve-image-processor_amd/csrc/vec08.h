// csrc/vec08.h -- the two halves of stage 08 as orip_dedup_layer (vector08.hip) calls them, on the claimed layer lane.
#pragma once
#include "vec_common.h"

// Stage 08-A (vector08a.hip): the sorted list S -> the lane's tp[2] (lines2) and the layer's taps.  caps_counted: flags.caps_distinct holds this run's count.
int dedup08_a(orip_ctx* c, int layer, const orip_params08& P, DPolys& S, DTaps& TOUT, PhaseTimer& T, bool& caps_counted);
// Stage 08-B (vector08b.hip): post-processing of tp[2] (which holds at least one line) -> tp[3] (merged)
int dedup08_b(orip_ctx* c, const orip_params08& P, PhaseTimer& T);
