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
#pragma once
#include "common.h"
#include "step_common.h"                 // step_matvec and the spine: step_enter, step_state, step_lstm_cell, step_readout, step_advance
#include "local_attn.h"                  // la_row_softmax
#include "lstm_step_plan.h"

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

// SLOTS: the positioned form (step_common.h: step_enter).
template <bool SLOTS>
__device__ __forceinline__ void lstm_step_body(const LstmStepParams& P, int* pos, int limit, int advance) {
    constexpr int KI = MMT_LSTM_STEP_MAX_IN, KE = MMT_LSTM_STEP_MAX_E, KH = MMT_LSTM_STEP_MAX_H, ML = MMT_LSTM_STEP_MAX_LAYERS;
    __shared__ __attribute__((aligned(16))) float xs[KI];                    // bf16(x), padded row
    __shared__ __attribute__((aligned(16))) float emb[KE];                   // bf16(embed), padded row
    __shared__ __attribute__((aligned(16))) float hid[KE];                   // bf16(relu(.)) of the attention MLP, later of the read-out
    __shared__ __attribute__((aligned(16))) float hp[ML * KH];               // bf16(h_prev of layer l), padded rows (p == 0: not read)
    __shared__ __attribute__((aligned(16))) float hc[KH];                    // bf16(h of the layer just run), later bf16(ctx), padded row
    __shared__ __attribute__((aligned(16))) float pre[4 * KH];               // gate pre-activations of the layer, [i f g o][H]
    __shared__ float htop[KH];                                               // m_t h of the top layer, fp32
    __shared__ float zs[MMT_LSTM_STEP_MAX_TAPS], as[MMT_LSTM_STEP_MAX_TAPS]; // the logits and their softmax

    const LstmStepPlan& S = P.pl;
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
        if (!first) step_matvec(st.W(S.whh[l]), hp + l * KH, S.KPh, G, [&](int n, float acc) { pre[n] += acc; });
        __syncthreads();                                                         // pre is whole; every read of hc by this layer is over
        const bool top = l == NL - 1;
        for (int j = tid; j < H; j += MMT_LSTM_STEP_THREADS) {
            const float cprev = first ? 0.f : st.in[(size_t)l * 2 * H + H + j];
            const StepCell u = step_lstm_cell(pre, H, j, cprev, first);
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
    step_readout(st.W(S.wd0), st.V(S.bd0), st.W(S.wd2), st.V(S.bd2), hc, S.KPh, hid, E, S.KPe, P.mask, b, P.y + b, 1);
    step_advance<SLOTS>(pos, b, t, advance);
}

__global__ __launch_bounds__(MMT_LSTM_STEP_THREADS) void lstm_step_kernel(const LstmStepParams P) { lstm_step_body<false>(P, nullptr, 0, 0); }

__global__ __launch_bounds__(MMT_LSTM_STEP_THREADS) void lstm_step_slots_kernel(const LstmStepParams P, int* pos, int limit, int advance) {
    lstm_step_body<true>(P, pos, limit, advance);
}
