// The ring K/V cache of a banded stream: with causal_attention(model, span=W) window t attends positions t - span + 1 .. t, so a step
// needs the last span - 1 cached keys and no others.  The ring forms of the encoder step (encoder_step_ring_kernel,
// encoder_step_ring_slots_kernel) keep a cache of R = span rows per (layer, K | V, sequence, head) and never fill.
//
// The rule:
//   keys      at position t the step has n = min(t, span - 1) cached keys, positions t - n .. t - 1 (K_t and V_t take part from LDS)
//   home      position j lives in row j mod span
//   write     step t writes K_t, V_t to row t mod span.  Before the write that row holds position t - span, which is outside the band,
//             so the row written is never among the rows read in the same step
//   sweep     in AGE order, oldest first: age i = 0 .. n - 1 is position t - n + i.  Ages are dealt to lanes as positions are in the
//             plain step
//   modulo    ONE per workgroup, r0 = (t - n) mod span on the wave-uniform t.  Age i lives in row r0 + i, minus span if that reaches
//             span (one compare and one select); the write row is "age n".  r0 + i < 2 span <= 8192: nothing overflows for 0 <= t < INT_MAX
//   idle      a lane behind n loads the row of age 0 (as it loads row 0 in the plain step); what it read is dropped by select
//
// Two exact facts follow from the age order, and tests/test_gpu_ring_stream.py holds both.  While t < span the ring step IS the plain
// step: n = t, r0 = 0, row = age = position.  And a row's bits depend on the last windows only, not on t or the ring's phase: the
// same values meet the same lanes in the same order wherever the ring stands.
//
// Plain C++ for the host and the device, so that a stand-alone program can walk it (tools/ring_plan_check.cpp).
#pragma once
#include "step_slots.h"           // MMT_SLOT_HD

// cached keys of step t: min(t, span - 1).  t >= 0, span >= 1
MMT_SLOT_HD static inline int ring_keys(int t, int span) { return t < span - 1 ? t : span - 1; }

// the row of age 0, the one modulo.  t - n >= 0
MMT_SLOT_HD static inline int ring_first_row(int t, int n, int span) { return (t - n) % span; }

// the row of age i (0 <= i <= n < span; i == n: the row step t writes), r0 in [0, span)
MMT_SLOT_HD static inline int ring_row(int r0, int i, int span) {
    const int r = r0 + i;
    return r >= span ? r - span : r;
}
