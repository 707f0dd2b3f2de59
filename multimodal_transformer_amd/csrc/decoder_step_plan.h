// Limits and layout of the stream state of the one-window decoder step (decoder_step.h): plain host C++ with no HIP in it, so that a
// stand-alone program can exercise it (tools/decoder_step_plan_check.cpp) and api.hip only adds the base pointer to the offsets computed here.
//
// The decoder: nn.LSTM(2d, d, L) fed [o_{t-1} ; enc_t] with o the top layer's output, then the read-out MLP d -> h_dim -> 1
// (multiTransformer._DecoderMixin); L = 0 is the read-out alone (UniFullTransformer).
//
// The state is one buffer of `bytes` bytes, every piece starting at a multiple of 256 bytes (a piece of no bytes takes none):
//   the prepared bf16 weights, each matrix in the step kernels' layout [k / 8][output row][k % 8] with k padded to a multiple of 8 by
//       zeros: Wx = W_ih_l0[:, d:] (4d x d; L >= 1); per layer l the pair (wa[l], wb[l]), 4d x d each:
//           L == 1:  wa[0] = W_rec = W_ih_l0[:, :d] + W_hh_l0 (summed in fp32, rounded once), wb[0] = W_hh_l0 (multiplies dec_h0 at position 0)
//           L >= 2:  wa[0] = W_ih_l0[:, :d] (multiplies o_prev), wb[0] = W_hh_l0; wa[l] = W_ih_l (multiplies h^{l-1}_t), wb[l] = W_hh_l
//       then W1 (h_dim x d) and W2 (1 x h_dim) of the read-out.
//   the fp32 vectors: per layer b_ih + b_hh (4d), b1 (h_dim), b2 (1), dec_h0 (L d), dec_c0 (L d).
//       Both written by mmt_decoder_stream_prepare, read by every step.
//   [dyn_off, bytes)  two copies of the carried state, fp32 [copy][b][layer][h (d) | c (d)]:
//       step p reads copy p & 1 (at p == 0 nothing: dec_h0 / dec_c0 / zeros stand for it) and writes copy (p + 1) & 1.
#pragma once
#include <stddef.h>
#include "step_prep.h"

#define MMT_DEC_STEP_MAX_D 512            // embed_dim: the width of the encoder's row and of every LSTM layer
#define MMT_DEC_STEP_MAX_HDIM 512         // hidden units of the read-out
#define MMT_DEC_STEP_MAX_L 4              // LSTM layers (0: read-out only)
#define MMT_DEC_STEP_THREADS 256

#define MMT_DEC_STEP_OK 0
#define MMT_DEC_STEP_EINVAL 1             // MMT_EINVAL
#define MMT_DEC_STEP_EUNSUPPORTED 2       // MMT_EUNSUPPORTED

struct DecStepPlan {
    int d, hdim, L, KPd, KPh;                         // KPd, KPh: d and h_dim padded to 8
    size_t wx, wa[MMT_DEC_STEP_MAX_L], wb[MMT_DEC_STEP_MAX_L], w1, w2;      // byte offsets of the matrices
    size_t bl[MMT_DEC_STEP_MAX_L], b1, b2, h0, c0;    // of the fp32 vectors
    size_t dyn_off, seq_floats, dyn_floats;           // the carried state: byte offset, floats per sequence and copy (2 L d), floats in all
    size_t bytes;
};

static inline size_t dec_step_align256(size_t n) { return (n + 255) / 256 * 256; }
static inline int dec_step_pad8(int n) { return (n + 7) / 8 * 8; }

// Returns MMT_DEC_STEP_OK, or the error class with *why naming the limit (a static string).
static inline int decoder_step_plan(DecStepPlan& P, int B, int d, int h_dim, int n_layers, const char** why) {
    if (B <= 0 || d <= 0 || h_dim <= 0 || n_layers < 0) { *why = "decoder stream: non-positive dimension"; return MMT_DEC_STEP_EINVAL; }
    if (n_layers > MMT_DEC_STEP_MAX_L) { *why = "decoder stream: n_layers > 4 not supported"; return MMT_DEC_STEP_EUNSUPPORTED; }
    if (d % 4) { *why = "decoder stream: embed_dim must be a multiple of 4"; return MMT_DEC_STEP_EUNSUPPORTED; }
    if (d > MMT_DEC_STEP_MAX_D) { *why = "decoder stream: embed_dim > 512 not supported"; return MMT_DEC_STEP_EUNSUPPORTED; }
    if (h_dim > MMT_DEC_STEP_MAX_HDIM) { *why = "decoder stream: h_dim > 512 not supported"; return MMT_DEC_STEP_EUNSUPPORTED; }
    const int L = n_layers;
    P.d = d; P.hdim = h_dim; P.L = L; P.KPd = dec_step_pad8(d); P.KPh = dec_step_pad8(h_dim);
    const size_t gate_mat = (size_t)4 * d * P.KPd * 2;
    size_t off = 0;
    P.wx = off; off += dec_step_align256(L ? gate_mat : 0);
    for (int l = 0; l < MMT_DEC_STEP_MAX_L; ++l) {
        P.wa[l] = off; off += dec_step_align256(l < L ? gate_mat : 0);
        P.wb[l] = off; off += dec_step_align256(l < L ? gate_mat : 0);
    }
    P.w1 = off; off += dec_step_align256((size_t)h_dim * P.KPd * 2);
    P.w2 = off; off += dec_step_align256((size_t)P.KPh * 2);
    for (int l = 0; l < MMT_DEC_STEP_MAX_L; ++l) { P.bl[l] = off; off += dec_step_align256(l < L ? (size_t)4 * d * 4 : 0); }
    P.b1 = off; off += dec_step_align256((size_t)h_dim * 4);
    P.b2 = off; off += dec_step_align256(4);
    P.h0 = off; off += dec_step_align256((size_t)L * d * 4);
    P.c0 = off; off += dec_step_align256((size_t)L * d * 4);
    P.dyn_off = off;
    P.seq_floats = (size_t)2 * L * d;
    P.dyn_floats = (size_t)2 * B * P.seq_floats;
    P.bytes = P.dyn_off + dec_step_align256(P.dyn_floats * 4);
    return MMT_DEC_STEP_OK;
}

// What mmt_decoder_stream_prepare writes, as the job table of step_prep_kernel (step_prep.h): every matrix and vector of the layout above
// and no byte of the carried state.  lstm_params: per layer nn.LSTM's weight_ih_l (4d, 2d for l = 0, else d), weight_hh_l (4d, d),
// bias_ih_l, bias_hh_l; dec_h0 / dec_c0 (L d) and lstm_params are not read when L == 0.
static_assert(3 + 2 * MMT_DEC_STEP_MAX_L <= MMT_STEP_PREP_MATS && 4 + MMT_DEC_STEP_MAX_L <= MMT_STEP_PREP_VECS, "the table's capacities");
static inline void decoder_step_prep_table(const DecStepPlan& S, const float* const* lstm_params, const float* dec_h0, const float* dec_c0,
                                           const float* W1, const float* b1, const float* W2, const float* b2, StepPrepParams& P, size_t& most) {
    P.nmat = P.nvec = 0;
    most = 1;
    const int L = S.L, d = S.d, G = 4 * S.d;
    auto mat = [&](const float* src, int ld, int col0, const float* src2, int ld2, int col2, size_t dst, int rows, int K) {
        step_prep_mat(P, most, src, ld, col0, src2, ld2, col2, dst, rows, K, rows);
    };
    for (int l = 0; l < L; ++l) {
        const float* const* lp = lstm_params + 4 * l;
        if (l == 0) {
            mat(lp[0], 2 * d, d, nullptr, 0, 0, S.wx, G, d);                                  // Wx = W_ih[:, d:]
            if (L == 1) mat(lp[0], 2 * d, 0, lp[1], d, 0, S.wa[0], G, d);                     // W_rec = W_ih[:, :d] + W_hh, as decoder_pack
            else mat(lp[0], 2 * d, 0, nullptr, 0, 0, S.wa[0], G, d);                          // P_0's first half, as decoder_stack_pack
        } else {
            mat(lp[0], d, 0, nullptr, 0, 0, S.wa[l], G, d);
        }
        mat(lp[1], d, 0, nullptr, 0, 0, S.wb[l], G, d);
        step_prep_vec(P, lp[2], lp[3], S.bl[l], G);
    }
    mat(W1, d, 0, nullptr, 0, 0, S.w1, S.hdim, d);
    mat(W2, S.hdim, 0, nullptr, 0, 0, S.w2, 1, S.hdim);
    step_prep_vec(P, b1, nullptr, S.b1, S.hdim);
    step_prep_vec(P, b2, nullptr, S.b2, 1);
    if (L) { step_prep_vec(P, dec_h0, nullptr, S.h0, L * d); step_prep_vec(P, dec_c0, nullptr, S.c0, L * d); }
}
