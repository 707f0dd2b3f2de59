// One window of the LSTM baseline per launch: lstm_step_kernel runs the embed, the attention MLP, the n_layers LSTM cells, the local
// attention over the last L outputs and the read-out MLP (models._LocalAttnLSTM._front / .forward for one t, with attend_over_taps on:
// the softmax over the L taps of a row, local_attn.h's second mode) for each of B sequences, carrying (h, c) of every layer and a ring
// of the last L masked outputs of the top layer in a stream state (layout and limits: lstm_step_plan.h).  Its input row is x_t (B, in);
// its output y_t (B, 1) is what the model's eval forward gives at [:, t] of the windows stepped so far.
//
// Shape of the kernel, as decoder_step.h and mfn_step.h: grid = B, one workgroup of 256 threads per sequence; workgroups share nothing
// and never communicate, so a sequence's result does not depend on the batch it is stepped in.  Every product is step_matvec
// (step_common.h) over prepared bf16 weights, the row lives in LDS between the stages.
//
// Arithmetic: the batch path's, row for row (bf16_ref.linear / linear_pair, lstm_scan, functional.local_attention): the left operand of
// every product is rounded to bf16, every weight is bf16, and sums, biases, the activations (sigmoid_f / tanh_f of scan_common.h), c, h,
// the softmax, the context and everything stored are fp32.  No site depends on a tile, so one reference serves the step and the batch
// path (tests/lstm_stream_ref.py).  At position p, eval mode:
//   embed = relu(bf16(x) We^T + be)
//   hid   = relu(bf16(embed) Wa0^T + ba0);  z = bf16(hid) Wa2^T + ba2                                      (L logits)
//   pre^0 = (bf16(embed) W_ih_l0^T + (b_ih + b_hh)) + [p > 0] bf16(h^0_prev) W_hh_l0^T
//   pre^l = (bf16(h^{l-1}_t) W_ih_l^T + (b_ih + b_hh)) + [p > 0] bf16(h^l_prev) W_hh_l^T
//   a     = la_row_softmax(z)                                                                             (local_attn.h)
//   ctx   = a[0] (m_t h_top) + sum_{1 <= i < L, i <= p} a[i] ring[(p - i) % L]                             (taps in index order)
//   y     = (bf16(relu(bf16(ctx) Wd0^T + bd0)) Wd2^T + bd2) * m_t
//
// State discipline.  Step p reads copy p & 1 of (h, c) and writes copy (p + 1) & 1; it writes ring slot p % L (m_t h_top) and reads only
// the slots (p - i) % L for 1 <= i <= min(p, L - 1): nothing written in a launch is read back in it.  At p == 0 no word of the dynamic
// state is read (by branch, not by multiplying), so a state of any bit pattern cannot reach a result and a new recording needs no
// launch.  Every address comes from (b < B, layer, p & 1, (p - i) % L) and the plan's offsets alone: t is a launch argument checked by
// the host, and the kernel returns at once when t < 0.  No address is derived from device data.
//
// The positioned form, lstm_step_slots_kernel: the same body with the position of each sequence read from device memory, as
// step_common.h describes it for every carried-state step.  What slot_decode lets through selects the copy, p & 1, and the ring slots.
//
// The tails (a compile-time switch of the one body; layout and limits: lstm_feedback_step_plan.h).  Stages 0 to 4 are the front of all
// three; what follows the context differs.  TAIL = plain is everything above.  The other two are the models whose read-out feeds its
// own prediction back (models.MultiEDLSTM, models.MultiARLSTM), free-running: the fed-back value is one more carried word, and the
// launch argument p_init stands in for the predictions before step 0.
//   TAIL = fb (MultiEDLSTM, one encoder layer; rounding sites: bf16_ref.lstm_fb_scan).  The encoder cell starts from the prepared rows
//   enc_h0 / enc_c0, which are values: at position 0 its recurrent product runs too, on bf16(enc_h0), and the cell keeps its forget
//   term (a property of the tail, not a test at run time).  Then, with hd, cd, q the decoder's carried state (at position 0 the
//   prepared dec_h0 / dec_c0 and p_init, by branch):
//     pre = (bf16(ctx) W_c^T + (b_ih + b_hh)_dec) + q_prev w_p + bf16(hd_prev) W_hh,dec^T          (w_p and q fp32)
//     (hd, cd) = cell(pre, cd_prev);  u = relu(bf16(hd) W1^T + b1)                                 (u fp32, NOT rounded)
//     q = sum_e u[e] w2[e] + b2                                                                    (w2 fp32; step_block_sum: a fixed order)
//     y = q m_t;  carried: (h, c) of the encoder, (hd, cd) and the UNMASKED q.
//   TAIL = ar (MultiARLSTM, 1 to 4 layers, zero initial states by branch as the plain tail).  K = ar_order:
//     in_part = bf16(relu(bf16(ctx) Wd0^T + bd0)) Wd2^T + bd2                                      (step_readout, no mask, into LDS)
//     w[k] = bf16(ctx) Wa^T + ba, k < K
//     acc = in_part;  for k = 0 .. K - 1: acc = fmaf(w[k], hist_k, acc),  hist_k = p_{t-K+k} where t - K + k >= 0, else p_init
//     y = acc m_t     (one thread; ar_combine.h's ar_free_fwd_kernel: its chain and order)
//   The unmasked acc is fed back through a ring of K + 1 fp32 slots per sequence: step t writes slot t % (K + 1) and reads the slots
//   (t - K + k) % (K + 1), K consecutive positions below t, which never name the slot it writes.
// The state discipline above holds for both: two copies of every carried block, nothing written in a launch is read back in it, no
// address from device data except through slot_decode, and a state of any bit pattern cannot reach a result at position 0.
#pragma once
#include "common.h"
#include "step_common.h"                 // step_matvec and the spine: step_enter, step_state, step_lstm_cell, step_readout, step_advance
#include "local_attn.h"                  // la_row_softmax
#include "lstm_step_plan.h"
#include "lstm_feedback_step_plan.h"

static_assert(MMT_LSTM_STEP_THREADS == MMT_STEP_THREADS, "step_matvec is written for one workgroup size");
static_assert(MMT_LSTM_STEP_MAX_TAPS == MMT_LA_MAXL, "the taps of the batch path");

struct LstmStepParams {
    const float* x;                            // (B, in)
    const float* mask;                         // (B) or nullptr
    float* y;                                  // (B, 1)
    char* state;
    int t, B;
    LstmStepPlan pl;
};

// The steps with a tail: the same fields, the plan with the tail's pieces, and what stands in for the predictions before step 0.
struct LstmFeedbackParams {
    const float* x;
    const float* mask;
    float* y;
    char* state;
    int t, B;
    float p_init;
    LstmFeedbackPlan pl;
};

__device__ __forceinline__ const LstmStepPlan& lstm_step_front(const LstmStepPlan& pl) { return pl; }
__device__ __forceinline__ const LstmStepPlan& lstm_step_front(const LstmFeedbackPlan& pl) { return pl.front; }

// SLOTS: the positioned form (step_common.h: step_enter).  TAIL: what follows the context (MMT_LSTM_TAIL_*); Params is LstmStepParams
// for the plain tail and LstmFeedbackParams for the other two.
template <bool SLOTS, int TAIL, typename Params>
__device__ __forceinline__ void lstm_step_body(const Params& P, int* pos, int limit, int advance) {
    constexpr bool FB = TAIL == MMT_LSTM_TAIL_FB, AR = TAIL == MMT_LSTM_TAIL_AR;
    constexpr int KI = MMT_LSTM_STEP_MAX_IN, KE = MMT_LSTM_STEP_MAX_E, KH = MMT_LSTM_STEP_MAX_H, ML = MMT_LSTM_STEP_MAX_LAYERS;
    __shared__ __attribute__((aligned(16))) float xs[KI];                    // bf16(x), padded row
    __shared__ __attribute__((aligned(16))) float emb[KE];                   // bf16(embed), padded row
    __shared__ __attribute__((aligned(16))) float hid[KE];                   // bf16(relu(.)) of the attention MLP, later of the read-out
    __shared__ __attribute__((aligned(16))) float hp[ML * KH];               // bf16(h_prev of layer l), padded rows (p == 0: not read)
    __shared__ __attribute__((aligned(16))) float hc[KH];                    // bf16(h of the layer just run), later bf16(ctx), padded row
    __shared__ __attribute__((aligned(16))) float pre[4 * KH];               // gate pre-activations of the layer, [i f g o][H]
    __shared__ float htop[KH];                                               // m_t h of the top layer, fp32
    __shared__ float zs[MMT_LSTM_STEP_MAX_TAPS], as[MMT_LSTM_STEP_MAX_TAPS]; // the logits and their softmax

    const LstmStepPlan& S = lstm_step_front(P.pl);
    const int tid = threadIdx.x, b = blockIdx.x;
    const int t = step_enter<SLOTS>(pos, b, limit, P.t);
    if (t == MMT_SLOT_SKIP) {                                                    // idle or full: a zero row and nothing else
        if (SLOTS && tid == 0) P.y[b] = 0.f;
        return;
    }
    const int E = S.E, H = S.H, NL = S.NL, L = S.L, G = 4 * H;
    const bool first = t == 0;                                                   // uniform: no word of the dynamic state is read
    const StepState st = step_state(P.state, S.dyn_off, S.seq_floats, t, P.B, b);
    float* ring = reinterpret_cast<float*>(P.state + S.ring_off) + (size_t)b * S.ring_seq_floats;
    const bool masked = P.mask != nullptr;
    const float mk = masked ? P.mask[b] : 1.f;

    // 0. stage x and, per layer, what multiplies the layer's recurrent matrix (rounded: both feed products only); zero the pads
    {
        const float* xr = P.x + (size_t)b * S.in;
        for (int k = tid; k < S.KPin; k += MMT_LSTM_STEP_THREADS) xs[k] = k < S.in ? step_bf16_round(xr[k]) : 0.f;
        for (int k = E + tid; k < S.KPe; k += MMT_LSTM_STEP_THREADS) { emb[k] = 0.f; hid[k] = 0.f; }
        for (int k = H + tid; k < S.KPh; k += MMT_LSTM_STEP_THREADS) hc[k] = 0.f;                 // the cells write [0, H): the pad stays zero
        if (!first)
            for (int l = 0; l < NL; ++l)
                for (int k = tid; k < S.KPh; k += MMT_LSTM_STEP_THREADS)
                    hp[l * KH + k] = k < H ? step_bf16_round(st.in[(size_t)l * 2 * H + k]) : 0.f;
        if constexpr (FB) {                                                      // one encoder layer; row 1 of hp: bf16(hd_prev)
            const float* h0 = st.V(P.pl.enc_h0);
            const float* hd = first ? st.V(P.pl.dec_h0) : step_state(P.state, P.pl.fb_off, P.pl.fb_seq_floats, t, P.B, b).in;
            for (int k = tid; k < S.KPh; k += MMT_LSTM_STEP_THREADS) {
                if (first) hp[k] = k < H ? step_bf16_round(h0[k]) : 0.f;         // the prepared row: a value, so the product runs
                hp[KH + k] = k < H ? step_bf16_round(hd[k]) : 0.f;
            }
        }
        __syncthreads();
    }

    // 1. embed: it feeds two products and nothing else, so only its rounded value is kept
    {
        const float* be = st.V(S.be);
        step_matvec(st.W(S.we), xs, S.KPin, E, [&](int n, float acc) { emb[n] = step_bf16_round(fmaxf(acc + be[n], 0.f)); });
        __syncthreads();
    }

    // 2. the attention MLP's hidden row and layer 0's input product (linear_pair on the embedding), then the logits
    {
        const float* ba0 = st.V(S.ba0);
        const float* b0 = st.V(S.bl[0]);
        step_matvec(st.W(S.wa0), emb, S.KPe, E, [&](int n, float acc) { hid[n] = step_bf16_round(fmaxf(acc + ba0[n], 0.f)); });
        step_matvec(st.W(S.wih[0]), emb, S.KPe, G, [&](int n, float acc) { pre[n] = acc + b0[n]; });
        __syncthreads();
        const float* ba2 = st.V(S.ba2);
        step_matvec(st.W(S.wa2), hid, S.KPe, L, [&](int n, float acc) { zs[n] = acc + ba2[n]; });
    }

    // 3. the layers, bottom up; a row of pre has the same owner in every product of a layer (step_matvec: the owner depends on nout alone)
    for (int l = 0; l < NL; ++l) {
        if (l > 0) {
            const float* bias = st.V(S.bl[l]);
            step_matvec(st.W(S.wih[l]), hc, S.KPh, G, [&](int n, float acc) { pre[n] = acc + bias[n]; });                         // h^{l-1}_t
        }
        if (FB || !first) step_matvec(st.W(S.whh[l]), hp + l * KH, S.KPh, G, [&](int n, float acc) { pre[n] += acc; });
        __syncthreads();                                                         // pre is whole; every read of hc by this layer is over
        const bool top = l == NL - 1;
        for (int j = tid; j < H; j += MMT_LSTM_STEP_THREADS) {
            float cprev;
            if constexpr (FB) cprev = first ? st.V(P.pl.enc_c0)[j] : st.in[(size_t)l * 2 * H + H + j];
            else cprev = first ? 0.f : st.in[(size_t)l * 2 * H + H + j];
            const StepCell u = step_lstm_cell(pre, H, j, cprev, FB ? false : first);
            st.out[(size_t)l * 2 * H + j] = u.h; st.out[(size_t)l * 2 * H + H + j] = u.c;
            hc[j] = step_bf16_round(u.h);
            if (top) htop[j] = masked ? u.h * mk : u.h;
        }
        __syncthreads();                                                         // hc (and zs, htop) whole; every read of pre is over
    }

    // 4. the local attention over the taps (fp32): tap 0 is this step's row, tap i the ring's slot of step p - i; then the ring's new slot
    {
        if (tid == 0) la_row_softmax(zs, L, as);
        __syncthreads();
        const float* a = as;
        const int taps = t < L - 1 ? t : L - 1;                                  // taps that reach before step 0 bring zeros
        for (int j = tid; j < H; j += MMT_LSTM_STEP_THREADS) {
            const float mine = htop[j];
            float acc = a[0] * mine;
            for (int i = 1; i <= taps; ++i) acc += a[i] * ring[(size_t)((t - i) % L) * H + j];
            ring[(size_t)(t % L) * H + j] = mine;                                // never one of the slots read above
            hc[j] = step_bf16_round(acc);
        }
        __syncthreads();
    }

    // 5. read-out and the window's mask
    if constexpr (FB) {
        // the decoder cell on [q_prev ; ctx] and its read-out; hp row 1 holds bf16(hd_prev), pre / hc / hid are free again
        __shared__ float red[4];
        const LstmFeedbackPlan& F = P.pl;
        const StepState fs = step_state(P.state, F.fb_off, F.fb_seq_floats, t, P.B, b);
        const float qprev = first ? P.p_init : fs.in[2 * H];
        {
            const float* bdec = st.V(F.bdec);
            const float* wp = st.V(F.wp);
            step_matvec(st.W(F.wc), hc, S.KPh, G, [&](int n, float acc) { pre[n] = acc + bdec[n]; });                              // gxc
            step_matvec(st.W(F.whd), hp + KH, S.KPh, G, [&](int n, float acc) { pre[n] = (pre[n] + qprev * wp[n]) + acc; });      // same owner
            __syncthreads();                                                     // pre is whole; every read of hc (ctx) is over
        }
        for (int j = tid; j < H; j += MMT_LSTM_STEP_THREADS) {
            const float cprev = first ? st.V(F.dec_c0)[j] : fs.in[H + j];
            const StepCell u = step_lstm_cell(pre, H, j, cprev, false);
            fs.out[j] = u.h; fs.out[H + j] = u.c;
            hc[j] = step_bf16_round(u.h);
        }
        __syncthreads();
        {
            const float* b1 = st.V(S.bd0);
            step_matvec(st.W(S.wd0), hc, S.KPh, E, [&](int n, float acc) { hid[n] = fmaxf(acc + b1[n], 0.f); });                  // u: fp32
            __syncthreads();
        }
        const float* w2 = st.V(F.w2);
        float part = 0.f;
        for (int e = tid; e < E; e += MMT_LSTM_STEP_THREADS) part = fmaf(hid[e], w2[e], part);
        const float q = step_block_sum(part, red) + st.V(S.bd2)[0];
        if (tid == 0) {
            fs.out[2 * H] = q;                                                   // fed back unmasked
            P.y[b] = masked ? q * mk : q;
        }
    } else if constexpr (AR) {
        __shared__ float wk[MMT_LSTM_FEEDBACK_MAX_AR], inpart[1];
        const LstmFeedbackPlan& F = P.pl;
        const int K = F.K;
        const float* ba = st.V(F.ba);
        step_matvec(st.W(F.wa), hc, S.KPh, K, [&](int n, float acc) { wk[n] = acc + ba[n]; });
        step_readout(st.W(S.wd0), st.V(S.bd0), st.W(S.wd2), st.V(S.bd2), hc, S.KPh, hid, E, S.KPe, nullptr, b, inpart, 1);
        __syncthreads();
        if (tid == 0) {
            float* hist = reinterpret_cast<float*>(P.state + F.hist_off) + (size_t)b * F.hist_seq_floats;
            float acc = inpart[0];
            for (int k = 0; k < K; ++k) {
                const int s = t - K + k;                                         // the step whose prediction tap k reads
                acc = fmaf(wk[k], s >= 0 ? hist[s % (K + 1)] : P.p_init, acc);
            }
            hist[t % (K + 1)] = acc;                                             // never one of the slots read above; fed back unmasked
            P.y[b] = masked ? acc * mk : acc;
        }
    } else {
        step_readout(st.W(S.wd0), st.V(S.bd0), st.W(S.wd2), st.V(S.bd2), hc, S.KPh, hid, E, S.KPe, P.mask, b, P.y + b, 1);
    }
    step_advance<SLOTS>(pos, b, t, advance);
}

__global__ __launch_bounds__(MMT_LSTM_STEP_THREADS) void lstm_step_kernel(const LstmStepParams P) {
    lstm_step_body<false, MMT_LSTM_TAIL_PLAIN>(P, nullptr, 0, 0);
}

__global__ __launch_bounds__(MMT_LSTM_STEP_THREADS) void lstm_step_slots_kernel(const LstmStepParams P, int* pos, int limit, int advance) {
    lstm_step_body<true, MMT_LSTM_TAIL_PLAIN>(P, pos, limit, advance);
}

// The steps with a tail: the read-out in the recurrence (fb) and the autoregressive read-out (ar), both forms each.
__global__ __launch_bounds__(MMT_LSTM_STEP_THREADS) void lstm_step_fb_kernel(const LstmFeedbackParams P) {
    lstm_step_body<false, MMT_LSTM_TAIL_FB>(P, nullptr, 0, 0);
}

__global__ __launch_bounds__(MMT_LSTM_STEP_THREADS) void lstm_step_fb_slots_kernel(const LstmFeedbackParams P, int* pos, int limit, int advance) {
    lstm_step_body<true, MMT_LSTM_TAIL_FB>(P, pos, limit, advance);
}

__global__ __launch_bounds__(MMT_LSTM_STEP_THREADS) void lstm_step_ar_kernel(const LstmFeedbackParams P) {
    lstm_step_body<false, MMT_LSTM_TAIL_AR>(P, nullptr, 0, 0);
}

__global__ __launch_bounds__(MMT_LSTM_STEP_THREADS) void lstm_step_ar_slots_kernel(const LstmFeedbackParams P, int* pos, int limit, int advance) {
    lstm_step_body<true, MMT_LSTM_TAIL_AR>(P, pos, limit, advance);
}
