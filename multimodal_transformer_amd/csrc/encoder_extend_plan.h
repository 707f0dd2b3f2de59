// Limits, the LDS carve and the index rule of the chunked encoder step (encoder_extend.h): a stream moves forward by a tile of up to
// MMT_EXTEND_ROWS = 16 consecutive windows per launch, from any position, on the stream state of encoder_step_plan.h exactly as it is.
// Plain C++ for the host and the device, so that a stand-alone program can walk it (tools/extend_plan_check.cpp).
//
// A call extends a recording by C windows; it runs as ceil(C / 16) launches in order, launch i with first = 16 i, the tile's first row
// within the call.  Every launch makes the SAME decision about a sequence, from the same inputs:
//   host form    sequence b stands at p (the call's t, by value) and gets len = C windows
//   slots form   row b of the call goes to sequence dst[b] with len[b] <= C windows; p = pos[dst[b]], which no launch of the call but
//                the LAST changes (it stores p + len there when `advance` is set), so every launch reads the value the call started on
// extend_decode is the ONE place where (dst, len, first, p) becomes "run c rows from position p + first" or "skip": a pair outside its
// ranges, an idle slot, and a slot whose p + len passes the capacity (ring: reaches INT_MAX) are skipped WHOLE, in every launch alike.
//
// The cache (encoder_step_plan.h, step_ring.h), per layer and K | V, for a tile at position t with c rows:
//   reads     plain: rows 0 .. t - 1.  Ring: the n = ring_keys(t, span) ages of step_ring.h, positions t - n .. t - 1; row i of the
//             tile attends those at or behind t + i - span + 1 (masked per element) and the tile's own rows from LDS
//   writes    plain: position t + i to row t + i, i < c.  Ring: the last min(c, span) positions of the tile only, position pos to row
//             pos mod span (step_prefill_plan.h's rule, prefill_row), so no two share a row.  Row (t + i) mod span holds position
//             t + i - span until then, which an earlier row of the same tile still reads: a layer's writes come behind ALL its reads
#pragma once
#include <limits.h>
#include <stddef.h>
#include "step_slots.h"           // MMT_SLOT_HD, slot_decode
#include "step_ring.h"            // ring_keys, ring_first_row, ring_row
#include "encoder_step_plan.h"
#include "step_prefill_plan.h"    // prefill_row

#define MMT_EXTEND_ROWS 16                        // windows per launch: the N of mfma_f32_16x16x32_bf16
#define MMT_EXTEND_THREADS 256
#define MMT_EXTEND_MAX_LDS (160 * 1024)           // the CU's LDS
#define MMT_EXTEND_SKIP (-1)

// The kernel's dynamic LDS, byte offsets from a 16-byte aligned base.  Rows are the tile's 16 windows.
//   xs   fp32 [16][xs_ld]   the residual rows
//   nb   bf16 [16][nb_ld]   bf16(LayerNorm) / the merged context: the B operand of the products over d (k padded to 32 by zeros)
//   hb   bf16 [16][hb_ld]   bf16(relu(hid)): the B operand of the product over f
//   q, k, v  bf16 [16][HDKP]   Q', K, V of the tile, [head][dkp] per row, pad columns zero
// The leading dimensions carry 8 bf16 (4 floats) of padding so that the 16 rows of an operand read start in different banks.
struct ExtendLds { int xs_ld, nb_ld, hb_ld; size_t xs, nb, hb, q, k, v, bytes; };

static inline size_t extend_align16(size_t n) { return (n + 15) / 16 * 16; }

// Returns MMT_STEP_OK, or the error class with *why naming the limit (a static string).  S: step_plan of the same shape.
static inline int extend_plan(ExtendLds& L, const StepPlan& S, int d, int f, const char** why) {
    L.xs_ld = d + 4;
    L.nb_ld = (d + 31) / 32 * 32 + 8;
    L.hb_ld = (f + 31) / 32 * 32 + 8;
    size_t o = 0;
    L.xs = o; o += extend_align16((size_t)MMT_EXTEND_ROWS * L.xs_ld * 4);
    L.nb = o; o += extend_align16((size_t)MMT_EXTEND_ROWS * L.nb_ld * 2);
    L.hb = o; o += extend_align16((size_t)MMT_EXTEND_ROWS * L.hb_ld * 2);
    L.q = o; o += extend_align16((size_t)MMT_EXTEND_ROWS * S.HDKP * 2);
    L.k = o; o += extend_align16((size_t)MMT_EXTEND_ROWS * S.HDKP * 2);
    L.v = o; o += extend_align16((size_t)MMT_EXTEND_ROWS * S.HDKP * 2);
    L.bytes = o;
    if (L.bytes > MMT_EXTEND_MAX_LDS) { *why = "encoder stream extend: the 16-row working set exceeds 160 KB of LDS (step through this shape)"; return MMT_STEP_EUNSUPPORTED; }
    return MMT_STEP_OK;
}

// What one workgroup of one launch does: dst == MMT_EXTEND_SKIP: nothing of the state (its rows of y are zeros).  Otherwise sequence
// dst runs c rows (0 <= c <= 16; 0: this tile lies behind the sequence's len) at positions t .. t + c - 1, and `next` = p + len is the
// position the call leaves behind, at most `rows` (plain) and below INT_MAX (ring).
struct ExtendRun { int dst, t, c, next; };

// dst, len: a table pair (host form: b and C).  first: the tile's first row within the call, a multiple of 16 below C.  p: the position
// the call started on, read from pos[dst] or passed by value.  C: the call's windows; rows: the capacity, or the span with ring != 0.
MMT_SLOT_HD static inline ExtendRun extend_decode(int dst, int len, int first, int p, int C, int B_state, int rows, int ring) {
    const ExtendRun skip = {MMT_EXTEND_SKIP, 0, 0, 0};
    if (dst < 0 || dst >= B_state || len < 1 || len > C || first < 0 || first >= C || rows < 1) return skip;
    if (slot_decode(p, ring ? 0 : rows) == MMT_SLOT_SKIP) return skip;                     // idle, full, INT_MAX
    if (ring ? len >= INT_MAX - p : len > rows - p) return skip;                           // p + len without overflow
    int c = len - first;
    c = c < 0 ? 0 : c > MMT_EXTEND_ROWS ? MMT_EXTEND_ROWS : c;
    return {dst, p + first, c, p + len};
}

// The ring write rule: of a tile's c rows the first extend_first_written(c, rows, ring) are NOT written (plain: 0, every row is)
MMT_SLOT_HD static inline int extend_first_written(int c, int rows, int ring) { return ring && c > rows ? c - rows : 0; }

// Row i of a tile at t (position t + i) and a CACHED key of age j (position t - n + j, j < n): inside the band?  Plain: always
MMT_SLOT_HD static inline bool extend_cached_ok(int i, int j, int n, int rows, int ring) { return !ring || j >= i + n - rows + 1; }
// ... and the tile's own key u (position t + u): causal, and inside the band
MMT_SLOT_HD static inline bool extend_tile_ok(int i, int u, int rows, int ring) { return u <= i && (!ring || u >= i - rows + 1); }
