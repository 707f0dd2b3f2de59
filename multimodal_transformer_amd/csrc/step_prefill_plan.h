// The prefill of a stream state: a recording that already has a history opens from ONE batch forward over that history instead of
// one step per window.  The fused stack's forward leaves K and V of every layer in its workspace (api.hip LayerWs::KR / VR, the R
// layout of common.h), and lstm_scan returns the decoder's h_all / c_all; the two kernels of step_prefill.h move them into the stream
// states of encoder_step_plan.h and decoder_step_plan.h.  This header is the index rule: which source element becomes which state
// element.  Plain C++ for the host and the device, so that a stand-alone program can walk it (tools/prefill_plan_check.cpp).
//
// The two layouts side by side, per layer and per K | V, bf16:
//   source   [b * h + head][tile = pos >> 5][e >> 3][pos & 31][e & 7]     Tp = round_up(P, 32) rows per head, heads padded to DKP in {16, 32, 64}
//   cache    [dst][head][row][e]                                          rows = capacity (plain) or span (ring), heads padded to dkp = pad8(d_k)
// Both are made of 16-byte chunks of 8 features of one position, so a lane moves a chunk: chunk c < dkp / 8 of (b, head, pos) goes
// to chunk c of (dst[b], head, row).  K carries no folded scale (only Q' is scaled: rowgemm.h scale_first), and both paths round K and
// V at the same site, bf16(n0 W^T + b), so the move is a copy.  The columns d_k <= e < dkp of the last chunk are written as zeros
// whatever the workspace holds there, as a step writes them.
//
// The rule:
//   lengths   sequence b < B_src has len[b] windows, 1 <= len[b] <= P, and goes to sequence dst[b] < B_state of the state
//   plain     positions 0 <= pos < len[b] are copied, position pos to row pos; len[b] <= capacity
//   ring      positions max(0, len[b] - span) <= pos < len[b] are copied, position pos to row pos mod span (step_ring.h: home).  These
//             are the last min(len, span) positions, so no two share a row, and they include the span - 1 that step len[b] reads
//   untouched rows >= len[b] (plain), every other sequence of the state, the prepared weights
//   decoder   n_layers == 1: h_all[len[b] - 1, b, :] and c_all[len[b] - 1, b, :] (fp32, time-major) go to copy len[b] & 1 of slot dst[b],
//             the copy step len[b] reads (decoder_step_plan.h: step p reads copy p & 1)
// prefill_seq is the ONE place where a (dst, len) pair, which the slots form reads from device memory, becomes addresses: a pair
// outside the ranges above is skipped, nothing of it is written.
#pragma once
#include <stddef.h>
#include "step_slots.h"           // MMT_SLOT_HD
#include "encoder_step_plan.h"
#include "decoder_step_plan.h"

#define MMT_PREFILL_THREADS 256
#define MMT_PREFILL_SKIP (-1)

// element (pos, e) of one (batch, head) matrix in the R layout: fragR_index of common.h, restated without HIP
MMT_SLOT_HD static inline size_t prefill_fragR_index(int pos, int e, int DKP) {
    return ((size_t)(pos >> 5) * (size_t)(DKP >> 3) + (size_t)(e >> 3)) * 256 + (size_t)(pos & 31) * 8 + (size_t)(e & 7);
}
// the batch path's padded head width (rowgemm.h make_layout)
MMT_SLOT_HD static inline int prefill_DKP(int dk) { return dk <= 16 ? 16 : dk <= 32 ? 32 : 64; }

struct PrefillGeom {
    int B_src, P, Tp, DKP;                // the forward's batch, windows, windows padded to 32, padded head
    int B_state, rows, ring;              // the state's batch; capacity, or span with ring != 0
    int h, N, dk, dkp, nchunk;
    size_t src_head;                      // Tp * DKP elements
    size_t cache_head, cache_seq, cache_kv, cache_layer;
};

static inline void prefill_geom(PrefillGeom& G, const StepPlan& S, int B_src, int P, int B_state, int rows, int ring, int h, int N) {
    G.B_src = B_src; G.P = P; G.Tp = (P + 31) / 32 * 32; G.DKP = prefill_DKP(S.dk);
    G.B_state = B_state; G.rows = rows; G.ring = ring;
    G.h = h; G.N = N; G.dk = S.dk; G.dkp = S.dkp; G.nchunk = S.nchunk;
    G.src_head = (size_t)G.Tp * G.DKP;
    G.cache_head = S.cache_head; G.cache_seq = S.cache_seq; G.cache_kv = S.cache_kv; G.cache_layer = S.cache_layer;
}

// the sequence a source row fills and the positions [first, len) that are copied; dst == MMT_PREFILL_SKIP: nothing
struct PrefillSeq { int dst, first, len; };
MMT_SLOT_HD static inline PrefillSeq prefill_seq(int dst, int len, int P, int B_state, int rows, int ring) {
    if (dst < 0 || dst >= B_state || len < 1 || len > P || rows < 1 || (!ring && len > rows)) return {MMT_PREFILL_SKIP, 0, 0};
    return {dst, ring && len > rows ? len - rows : 0, len};
}
// the cache row of position pos
MMT_SLOT_HD static inline int prefill_row(int pos, int rows, int ring) { return ring ? pos % rows : pos; }

// chunk c of (layer, kv, source sequence b, head, position pos): element offsets of its 8 features in the layer's KR | VR and in the cache
struct PrefillAt { size_t src, dst; };
MMT_SLOT_HD static inline PrefillAt prefill_at(const PrefillGeom& G, int layer, int kv, int b, int dst, int head, int pos, int c) {
    PrefillAt at;
    at.src = ((size_t)b * G.h + head) * G.src_head + prefill_fragR_index(pos, 8 * c, G.DKP);
    at.dst = (size_t)layer * G.cache_layer + (size_t)kv * G.cache_kv + (size_t)dst * G.cache_seq + (size_t)head * G.cache_head
             + (size_t)prefill_row(pos, G.rows, G.ring) * G.dkp + (size_t)8 * c;
    return at;
}
// item i of a (layer, kv, sequence) job: chunks fastest, then positions, then heads, so that consecutive lanes write consecutive
// 16-byte chunks of the cache and read two to eight runs of consecutive chunks of the source
struct PrefillItem { int head, pos, c; };
MMT_SLOT_HD static inline size_t prefill_items(const PrefillGeom& G, const PrefillSeq& q) { return (size_t)G.h * (size_t)(q.len - q.first) * G.nchunk; }
MMT_SLOT_HD static inline PrefillItem prefill_item(const PrefillGeom& G, const PrefillSeq& q, size_t i) {
    const int n = q.len - q.first;
    const int c = (int)(i % G.nchunk);
    const size_t r = i / G.nchunk;
    return {(int)(r / n), q.first + (int)(r % n), c};
}

// The decoder's carried state (n_layers == 1: seq_floats = 2 d, [h (d) | c (d)]): float j < d of h (which = 0) or c (which = 1) of
// source sequence b with len windows -> offsets in h_all | c_all (T, B_src, d) and in the carried state behind dyn_off
struct DecPrefillAt { size_t src, dst; };
MMT_SLOT_HD static inline DecPrefillAt dec_prefill_at(int B_src, int B_state, int d, size_t seq_floats, int b, int dst, int len, int which, int j) {
    DecPrefillAt at;
    at.src = ((size_t)(len - 1) * B_src + b) * d + j;
    at.dst = ((size_t)(len & 1) * B_state + dst) * seq_floats + (size_t)which * d + j;
    return at;
}
