// Limits and layout of the stream state of the one-window LSTM-baseline step (lstm_step.h): plain host C++ with no HIP in it, so that a
// stand-alone program can exercise it (tools/lstm_step_plan_check.cpp) and api.hip only adds the base pointer to the offsets computed here.
//
// The model (models._LocalAttnLSTM with attend_over_taps on): embed Linear(in -> E) + ReLU, the attention MLP E -> E -> L, nn.LSTM(E, H,
// n_layers) from zero states, the local attention over the last L outputs of the top layer, the read-out MLP H -> E -> 1.
//
// The state is one buffer of `bytes` bytes, every piece starting at a multiple of 256 bytes (a piece of no bytes takes none):
//   the prepared bf16 weights, each matrix in the step kernels' layout [k / 8][output row][k % 8] with k padded to a multiple of 8 by
//       zeros: We (E x in), Wa0 (E x E), Wa2 (L x E), per layer wih[l] (4H x E for l = 0, else 4H x H) and whh[l] (4H x H), Wd0 (E x H),
//       Wd2 (1 x E): at most 13 matrices;
//   the fp32 vectors: be (E), ba0 (E), ba2 (L), per layer b_ih + b_hh (4H), bd0 (E), bd2 (1): at most 9.
//       Both written by mmt_lstm_stream_prepare, read by every step.
//   [dyn_off, ring_off)   two copies of the carried state, fp32 [copy][b][layer][h (H) | c (H)]:
//       step p reads copy p & 1 (at p == 0 nothing: the states start from zero, by branch) and writes copy (p + 1) & 1.
//   [ring_off, bytes)     the ring of the local attention, fp32 [b][slot < L][H]: slot p % L holds m_p * h_top of step p.  Step p writes
//       slot p % L and reads the slots (p - i) % L for 1 <= i <= min(p, L - 1), which never name the slot it writes.
#pragma once
#include <stddef.h>
#include "step_prep.h"

#define MMT_LSTM_STEP_MAX_IN 2048         // width of the input row (B1's concatenated front end: 1556)
#define MMT_LSTM_STEP_MAX_E 512           // embed_dim
#define MMT_LSTM_STEP_MAX_H 512           // h_dim
#define MMT_LSTM_STEP_MAX_LAYERS 4        // LSTM layers, at least 1
#define MMT_LSTM_STEP_MAX_TAPS 16         // attn_len (MMT_LA_MAXL)
#define MMT_LSTM_STEP_THREADS 256

#define MMT_LSTM_STEP_OK 0
#define MMT_LSTM_STEP_EINVAL 1            // MMT_EINVAL
#define MMT_LSTM_STEP_EUNSUPPORTED 2      // MMT_EUNSUPPORTED

struct LstmStepPlan {
    int in, E, H, NL, L, KPin, KPe, KPh;              // KP*: the widths padded to 8
    size_t we, wa0, wa2, wih[MMT_LSTM_STEP_MAX_LAYERS], whh[MMT_LSTM_STEP_MAX_LAYERS], wd0, wd2;      // byte offsets of the matrices
    size_t be, ba0, ba2, bl[MMT_LSTM_STEP_MAX_LAYERS], bd0, bd2;                                      // of the fp32 vectors
    size_t dyn_off, seq_floats, dyn_floats;           // the carried (h, c): byte offset, floats per sequence and copy (2 NL H), floats in all
    size_t ring_off, ring_seq_floats, ring_floats;    // the ring: byte offset, floats per sequence (L H), floats in all
    size_t bytes;
};

static inline size_t lstm_step_align256(size_t n) { return (n + 255) / 256 * 256; }
static inline int lstm_step_pad8(int n) { return (n + 7) / 8 * 8; }

// Returns MMT_LSTM_STEP_OK, or the error class with *why naming the limit (a static string).
static inline int lstm_step_plan(LstmStepPlan& P, int B, int in, int E, int H, int n_layers, int attn_len, const char** why) {
    if (B <= 0 || in <= 0 || E <= 0 || H <= 0 || n_layers <= 0 || attn_len <= 0) { *why = "lstm stream: non-positive dimension"; return MMT_LSTM_STEP_EINVAL; }
    if (in > MMT_LSTM_STEP_MAX_IN) { *why = "lstm stream: input width > 2048 not supported"; return MMT_LSTM_STEP_EUNSUPPORTED; }
    if (E > MMT_LSTM_STEP_MAX_E) { *why = "lstm stream: embed_dim > 512 not supported"; return MMT_LSTM_STEP_EUNSUPPORTED; }
    if (H > MMT_LSTM_STEP_MAX_H) { *why = "lstm stream: h_dim > 512 not supported"; return MMT_LSTM_STEP_EUNSUPPORTED; }
    if (n_layers > MMT_LSTM_STEP_MAX_LAYERS) { *why = "lstm stream: n_layers > 4 not supported"; return MMT_LSTM_STEP_EUNSUPPORTED; }
    if (attn_len > MMT_LSTM_STEP_MAX_TAPS) { *why = "lstm stream: attn_len > 16 not supported"; return MMT_LSTM_STEP_EUNSUPPORTED; }
    const int NL = n_layers, L = attn_len;
    P.in = in; P.E = E; P.H = H; P.NL = NL; P.L = L;
    P.KPin = lstm_step_pad8(in); P.KPe = lstm_step_pad8(E); P.KPh = lstm_step_pad8(H);
    size_t off = 0;
    P.we = off; off += lstm_step_align256((size_t)E * P.KPin * 2);
    P.wa0 = off; off += lstm_step_align256((size_t)E * P.KPe * 2);
    P.wa2 = off; off += lstm_step_align256((size_t)L * P.KPe * 2);
    for (int l = 0; l < MMT_LSTM_STEP_MAX_LAYERS; ++l) {
        P.wih[l] = off; off += lstm_step_align256(l < NL ? (size_t)4 * H * (l == 0 ? P.KPe : P.KPh) * 2 : 0);
        P.whh[l] = off; off += lstm_step_align256(l < NL ? (size_t)4 * H * P.KPh * 2 : 0);
    }
    P.wd0 = off; off += lstm_step_align256((size_t)E * P.KPh * 2);
    P.wd2 = off; off += lstm_step_align256((size_t)P.KPe * 2);
    P.be = off; off += lstm_step_align256((size_t)E * 4);
    P.ba0 = off; off += lstm_step_align256((size_t)E * 4);
    P.ba2 = off; off += lstm_step_align256((size_t)L * 4);
    for (int l = 0; l < MMT_LSTM_STEP_MAX_LAYERS; ++l) { P.bl[l] = off; off += lstm_step_align256(l < NL ? (size_t)4 * H * 4 : 0); }
    P.bd0 = off; off += lstm_step_align256((size_t)E * 4);
    P.bd2 = off; off += lstm_step_align256(4);
    P.dyn_off = off;
    P.seq_floats = (size_t)2 * NL * H;
    P.dyn_floats = (size_t)2 * B * P.seq_floats;
    off += lstm_step_align256(P.dyn_floats * 4);
    P.ring_off = off;
    P.ring_seq_floats = (size_t)L * H;
    P.ring_floats = (size_t)B * P.ring_seq_floats;
    P.bytes = P.ring_off + lstm_step_align256(P.ring_floats * 4);
    return MMT_LSTM_STEP_OK;
}

// What mmt_lstm_stream_prepare writes, as the job table of step_prep_kernel (step_prep.h): every matrix and vector of the layout above
// and no byte of the carried state or the ring.  params: embed (W, b), attn[0] (W, b), attn[2] (W, b), per layer nn.LSTM's weight_ih_l,
// weight_hh_l, bias_ih_l, bias_hh_l, then the read-out's first (W, b) and last (W, b): 10 + 4 n_layers pointers.
#define MMT_LSTM_STEP_NPARAMS(NL) (10 + 4 * (NL))
static_assert(5 + 2 * MMT_LSTM_STEP_MAX_LAYERS <= MMT_STEP_PREP_MATS && 5 + MMT_LSTM_STEP_MAX_LAYERS <= MMT_STEP_PREP_VECS, "the table's capacities");
static inline void lstm_step_prep_table(const LstmStepPlan& S, const float* const* params, StepPrepParams& P, size_t& most) {
    P.nmat = P.nvec = 0;
    most = 1;
    const int E = S.E, H = S.H, G = 4 * S.H;
    auto mat = [&](const float* src, size_t dst, int rows, int K) { step_prep_mat(P, most, src, K, 0, nullptr, 0, 0, dst, rows, K, rows); };
    mat(params[0], S.we, E, S.in);
    step_prep_vec(P, params[1], nullptr, S.be, E);
    mat(params[2], S.wa0, E, E);
    step_prep_vec(P, params[3], nullptr, S.ba0, E);
    mat(params[4], S.wa2, S.L, E);
    step_prep_vec(P, params[5], nullptr, S.ba2, S.L);
    for (int l = 0; l < S.NL; ++l) {
        const float* const* lp = params + 6 + 4 * l;
        mat(lp[0], S.wih[l], G, l == 0 ? E : H);
        mat(lp[1], S.whh[l], G, H);
        step_prep_vec(P, lp[2], lp[3], S.bl[l], G);
    }
    const float* const* dp = params + 6 + 4 * S.NL;
    mat(dp[0], S.wd0, E, H);
    step_prep_vec(P, dp[1], nullptr, S.bd0, E);
    mat(dp[2], S.wd2, 1, E);
    step_prep_vec(P, dp[3], nullptr, S.bd2, 1);
}
