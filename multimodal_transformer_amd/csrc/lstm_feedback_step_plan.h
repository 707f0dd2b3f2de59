// Limits and layout of the stream state of the one-window steps of the two LSTM baselines whose read-out feeds its own prediction back
// (lstm_step.h with a tail): plain host C++ with no HIP in it, so that a stand-alone program can exercise it
// (tools/lstm_feedback_plan_check.cpp) and api.hip only adds the base pointer to the offsets computed here.
//
// tail 1, the read-out in the recurrence (models.MultiEDLSTM, one encoder layer): the front of the LSTM baseline with `encoder` as its
//   LSTM, started from enc_h0 / enc_c0, then a decoder cell on [q_{t-1} ; ctx_t] from dec_h0 / dec_c0 whose read-out MLP gives q_t.
// tail 2, the autoregressive read-out (models.MultiARLSTM, 1 to 4 layers): the front from zero states, the read-out MLP (in_part) and
//   ar_order coefficients w from ctx_t; p_t = in_part + sum_k w[k] p_{t-K+k}, predictions before step 0 being p_init.
//
// The state is one buffer of `bytes` bytes.  [0, front.bytes) is the plain step's state unchanged (lstm_step_plan.h): its read-out
// pieces wd0 / bd0 hold out.0 (tail 1) or decoder.0 (tail 2), bd2 the last bias; wd2 holds the last weight as bf16, which tail 1 does
// not read (its w2 is fp32, below).  Behind it, every piece at a multiple of 256 bytes:
//   tail 1: W_c = decoder.weight_ih_l0[:, 1:] (4H x H) and W_hh,dec (4H x H) as prepared bf16 matrices; w_p = decoder.weight_ih_l0[:, 0]
//       (4H), (b_ih + b_hh)_dec (4H), w2 (E) in fp32; the rows enc_h0, enc_c0, dec_h0, dec_c0 (H each); then two copies of the
//       decoder's carried state, fp32 [copy][b][hd (H) | cd (H) | q (1), padded to a multiple of 4 floats]: step p reads copy p & 1 (at
//       p == 0 nothing: the prepared rows and the launch argument p_init stand in, by branch) and writes copy (p + 1) & 1.
//   tail 2: Wa = autoreg.weight (K x H, prepared bf16), ba (K) fp32; then the history ring, fp32 [b][K + 1]: step p writes slot
//       p % (K + 1) with its unmasked prediction and reads the slots (p - K + k) % (K + 1) for k < K where p - K + k >= 0, K consecutive
//       positions below p, which never name the slot it writes: a step that does not advance is repeatable.
#pragma once
#include <stddef.h>
#include "lstm_step_plan.h"

#define MMT_LSTM_TAIL_PLAIN 0             // lstm_step.h's own kernel: no LstmFeedbackPlan
#define MMT_LSTM_TAIL_FB 1                // the read-out in the recurrence
#define MMT_LSTM_TAIL_AR 2                // the autoregressive read-out
#define MMT_LSTM_FEEDBACK_MAX_AR 16       // ar_order (MMT_AR_MAXK)

struct LstmFeedbackPlan {
    LstmStepPlan front;
    int tail, K;                                      // K: ar_order (tail 2), else 0
    size_t wc, whd;                                   // tail 1: byte offsets of the prepared matrices
    size_t wp, bdec, w2, enc_h0, enc_c0, dec_h0, dec_c0;      // of the fp32 vectors
    size_t fb_off, fb_seq_floats, fb_floats;          // the decoder's carried (hd, cd, q): byte offset, floats per sequence and copy, floats in all
    size_t wa, ba;                                    // tail 2: Wa and ba
    size_t hist_off, hist_seq_floats, hist_floats;    // the history ring: byte offset, floats per sequence (K + 1), floats in all
    size_t bytes;
};

// Returns MMT_LSTM_STEP_OK, or the error class with *why naming the limit (a static string).
static inline int lstm_feedback_plan(LstmFeedbackPlan& P, int tail, int ar_order, int B, int in, int E, int H, int n_layers, int attn_len,
                                     const char** why) {
    if (tail != MMT_LSTM_TAIL_FB && tail != MMT_LSTM_TAIL_AR) {
        *why = "lstm feedback stream: tail must be 1 (read-out in the recurrence) or 2 (autoregressive)";
        return MMT_LSTM_STEP_EINVAL;
    }
    const int rc = lstm_step_plan(P.front, B, in, E, H, n_layers, attn_len, why);
    if (rc) return rc;
    if (tail == MMT_LSTM_TAIL_FB && n_layers != 1) {
        *why = "lstm feedback stream: the read-out in the recurrence takes n_layers == 1";
        return MMT_LSTM_STEP_EUNSUPPORTED;
    }
    if (tail == MMT_LSTM_TAIL_AR && ar_order < 1) { *why = "lstm feedback stream: ar_order < 1"; return MMT_LSTM_STEP_EINVAL; }
    if (tail == MMT_LSTM_TAIL_AR && ar_order > MMT_LSTM_FEEDBACK_MAX_AR) {
        *why = "lstm feedback stream: ar_order > 16 not supported";
        return MMT_LSTM_STEP_EUNSUPPORTED;
    }
    const LstmStepPlan& S = P.front;
    const bool fb = tail == MMT_LSTM_TAIL_FB;
    const int K = fb ? 0 : ar_order;
    P.tail = tail; P.K = K;
    size_t off = S.bytes;
    auto piece = [&](size_t& at, size_t nbytes) { at = off; off += lstm_step_align256(nbytes); };
    piece(P.wc, fb ? (size_t)4 * H * S.KPh * 2 : 0);
    piece(P.whd, fb ? (size_t)4 * H * S.KPh * 2 : 0);
    piece(P.wp, fb ? (size_t)4 * H * 4 : 0);
    piece(P.bdec, fb ? (size_t)4 * H * 4 : 0);
    piece(P.w2, fb ? (size_t)E * 4 : 0);
    piece(P.enc_h0, fb ? (size_t)H * 4 : 0);
    piece(P.enc_c0, fb ? (size_t)H * 4 : 0);
    piece(P.dec_h0, fb ? (size_t)H * 4 : 0);
    piece(P.dec_c0, fb ? (size_t)H * 4 : 0);
    piece(P.wa, fb ? 0 : (size_t)K * S.KPh * 2);
    piece(P.ba, fb ? 0 : (size_t)K * 4);
    P.fb_seq_floats = fb ? ((size_t)2 * H + 1 + 3) / 4 * 4 : 0;
    P.fb_floats = (size_t)2 * B * P.fb_seq_floats;
    piece(P.fb_off, P.fb_floats * 4);
    P.hist_seq_floats = fb ? 0 : (size_t)K + 1;
    P.hist_floats = (size_t)B * P.hist_seq_floats;
    piece(P.hist_off, P.hist_floats * 4);
    P.bytes = off;
    return MMT_LSTM_STEP_OK;
}

// What mmt_lstm_feedback_stream_prepare writes, as the job table of step_prep_kernel (step_prep.h): the front's table from the first
// MMT_LSTM_STEP_NPARAMS(n_layers) pointers (lstm_step_prep_table: the LSTM that reads the embedding, then the first and last layer of
// the read-out MLP), then the tail's pieces, and no byte of a carried block or ring.  params behind the front's:
//   tail 1 (9 more): decoder.weight_ih_l0 (4H, 1 + H), w_p = its column 0 as a CONTIGUOUS (4H) vector (a vector job copies contiguous
//       floats only), decoder.weight_hh_l0 (4H, H), decoder.bias_ih_l0, decoder.bias_hh_l0, enc_h0, enc_c0, dec_h0, dec_c0 (H each).
//       The front's last matrix (1, E) is out.2.weight: it is also copied in fp32, as w2.
//   tail 2 (2 more): autoreg.weight (K, H), autoreg.bias (K).
#define MMT_LSTM_FEEDBACK_NPARAMS(TAIL, NL) (MMT_LSTM_STEP_NPARAMS(NL) + ((TAIL) == MMT_LSTM_TAIL_FB ? 9 : 2))
static_assert(5 + 2 * 1 + 2 <= MMT_STEP_PREP_MATS && 5 + 1 + 7 <= MMT_STEP_PREP_VECS, "the table's capacities, tail 1: 9 matrices, 13 vectors");
static_assert(5 + 2 * MMT_LSTM_STEP_MAX_LAYERS + 1 <= MMT_STEP_PREP_MATS && 5 + MMT_LSTM_STEP_MAX_LAYERS + 1 <= MMT_STEP_PREP_VECS,
              "the table's capacities, tail 2: 14 matrices, 10 vectors");
static inline void lstm_feedback_prep_table(const LstmFeedbackPlan& F, const float* const* params, StepPrepParams& P, size_t& most) {
    const LstmStepPlan& S = F.front;
    lstm_step_prep_table(S, params, P, most);
    const int E = S.E, H = S.H, G = 4 * S.H;
    const float* const* tp = params + MMT_LSTM_STEP_NPARAMS(S.NL);
    if (F.tail == MMT_LSTM_TAIL_FB) {
        step_prep_mat(P, most, tp[0], 1 + H, 1, nullptr, 0, 0, F.wc, G, H, G);             // W_c: the columns behind the first
        step_prep_mat(P, most, tp[2], H, 0, nullptr, 0, 0, F.whd, G, H, G);
        step_prep_vec(P, tp[1], nullptr, F.wp, G);
        step_prep_vec(P, tp[3], tp[4], F.bdec, G);
        step_prep_vec(P, params[MMT_LSTM_STEP_NPARAMS(S.NL) - 2], nullptr, F.w2, E);       // out.2.weight (1, E), unrounded
        step_prep_vec(P, tp[5], nullptr, F.enc_h0, H);
        step_prep_vec(P, tp[6], nullptr, F.enc_c0, H);
        step_prep_vec(P, tp[7], nullptr, F.dec_h0, H);
        step_prep_vec(P, tp[8], nullptr, F.dec_c0, H);
    } else {
        step_prep_mat(P, most, tp[0], H, 0, nullptr, 0, 0, F.wa, F.K, H, F.K);
        step_prep_vec(P, tp[1], nullptr, F.ba, F.K);
    }
}
