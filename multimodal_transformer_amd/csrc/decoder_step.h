// One window of the LSTM decoder and the read-out per launch: decoder_step_kernel advances the L layers of the autoregressive decoder
// (transformer/SFT/multiTransformer.py:463-483 for one t; multiTransformer._DecoderMixin._decode / _decode_stacked) by one position for
// each of B sequences and runs the read-out MLP on the top layer's h, carrying (h, c) of every layer in a stream state (layout and
// limits: decoder_step_plan.h).  Its input row is the encoder step's output e_t (B, d); its output y_t (B, 1) is what the model's eval
// forward gives at [:, t] of the windows stepped so far.  L = 0: the read-out alone (UniFullTransformer), no cell and no carried state.
//
// Shape of the kernel, as mfn_step.h: grid = B, one workgroup of 256 threads per sequence; workgroups share nothing and never
// communicate, so a sequence's result does not depend on the batch it is stepped in.  Every product is step_matvec (step_common.h)
// over prepared bf16 weights, the row lives in LDS between the stages, and the stages are a chain of dependent round trips.
//
// Arithmetic: the batch path's, row for row (bf16_ref.linear, lstm_scan, lstm_stack_scan): the left operand of every product is rounded
// to bf16 (e, h_prev / dec_h0, o_prev, the h of the layer below, h_top, relu(W1 h_top + b1)), every weight is bf16, and sums, biases,
// the activations (sigmoid_f / tanh_f of scan_common.h), c, h and everything stored are fp32.  No site depends on a tile, so the same
// reference serves the step and the batch path (tests/decoder_stream_ref.py).
//   L == 1:  pre = bf16(e) Wx^T + b  +  (p > 0 ? bf16(h_prev) W_rec^T : bf16(dec_h0) W_hh^T)
//   L >= 2:  pre^0 = bf16(e) Wx^T + b_0 + bf16(o_prev) wa_0^T + bf16(h^0_prev) wb_0^T        o_prev: the top layer's previous h; p == 0: absent
//            pre^l = bf16(h^{l-1}_t) wa_l^T + b_l + bf16(h^l_prev) wb_l^T                    p == 0: h^l_prev = dec_h0[l], c^l_prev = dec_c0[l]
//   read-out: y = (bf16(relu(bf16(h_top) W1^T + b1)) W2^T + b2) * mask_t[b]
//
// State discipline.  Step p reads copy p & 1 of (h, c) and writes copy (p + 1) & 1: nothing written in a launch is read back in it.
// At p == 0 no word of either copy is read (dec_h0 / dec_c0 / nothing stand for the state, by branch, not by multiplying), so a state
// of any bit pattern cannot reach a result and a new recording needs no launch.  Every address comes from (b < B, layer, p & 1) and the
// plan's offsets alone: t is a launch argument checked by the host, and the kernel returns at once when t < 0.  No address is derived
// from device data.
//
// The positioned form, decoder_step_slots_kernel: the same body with the position of each sequence read from device memory, as
// step_common.h describes it for every carried-state step; both contracts above hold for it, with slot_decode in the host's place.
#pragma once
#include "common.h"
#include "step_common.h"                 // step_matvec and the spine: step_enter, step_state, step_lstm_cell, step_readout, step_advance
#include "decoder_step_plan.h"

static_assert(MMT_DEC_STEP_THREADS == MMT_STEP_THREADS, "step_matvec is written for one workgroup size");

struct DecStepParams {
    const float* e;                            // (B, d): the encoder step's output row
    const float* mask;                         // (B) or nullptr
    float* y;                                  // (B, 1)
    char* state;
    int t, B;
    DecStepPlan pl;
};

// SLOTS: the positioned form (step_common.h: step_enter).
template <bool SLOTS>
__device__ __forceinline__ void decoder_step_body(const DecStepParams& P, int* pos, int limit, int advance) {
    constexpr int KD = MMT_DEC_STEP_MAX_D, ML = MMT_DEC_STEP_MAX_L;
    __shared__ __attribute__((aligned(16))) float es[KD];                    // bf16(e), padded row
    __shared__ __attribute__((aligned(16))) float hp[ML * KD];               // bf16(h_prev of layer l) (p == 0: bf16(dec_h0[l])), padded rows
    __shared__ __attribute__((aligned(16))) float hc[KD];                    // bf16(h of the layer just run), padded row
    __shared__ __attribute__((aligned(16))) float pre[4 * KD];               // gate pre-activations of the layer, [i f g o][d]
    __shared__ __attribute__((aligned(16))) float hid[MMT_DEC_STEP_MAX_HDIM];   // bf16(relu(W1 h_top + b1)), padded row

    const DecStepPlan& S = P.pl;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int t = step_enter<SLOTS>(pos, b, limit, P.t);
    if (t == MMT_SLOT_SKIP) {                                                    // idle or full: a zero row and nothing else
        if (SLOTS && tid == 0) P.y[b] = 0.f;
        return;
    }
    const int d = S.d, KPd = S.KPd, L = S.L, G = 4 * d;
    const bool first = t == 0;                                                   // uniform: no word of the carried state is read
    const StepState st = step_state(P.state, S.dyn_off, S.seq_floats, t, P.B, b);

    // 0. stage e and, per layer, what multiplies the layer's recurrent matrix (rounded: both feed products only)
    {
        const float* er = P.e + (size_t)b * d;
        const float* h0 = st.V(S.h0);
        for (int k = tid; k < KPd; k += MMT_DEC_STEP_THREADS) {
            es[k] = k < d ? step_bf16_round(er[k]) : 0.f;
            hc[k] = 0.f;                                                         // the cells write [0, d): the pad stays zero
        }
        for (int l = 0; l < L; ++l)
            for (int k = tid; k < KPd; k += MMT_DEC_STEP_THREADS) {
                float v = 0.f;
                if (k < d) v = step_bf16_round(first ? h0[l * d + k] : st.in[(size_t)l * 2 * d + k]);
                hp[l * KD + k] = v;
            }
        for (int k = S.hdim + tid; k < S.KPh; k += MMT_DEC_STEP_THREADS) hid[k] = 0.f;          // the pad of the read-out's second input
        __syncthreads();
    }

    // 1. the layers, bottom up; a row of pre has the same owner in every product of a layer (step_matvec: the owner depends on nout alone)
    for (int l = 0; l < L; ++l) {
        const float* bias = st.V(S.bl[l]);
        if (l == 0) {
            step_matvec(st.W(S.wx), es, KPd, G, [&](int n, float acc) { pre[n] = acc + bias[n]; });
            if (L == 1) {                                                        // W_rec on h_prev; at position 0 o_prev = 0: W_hh on dec_h0
                step_matvec(st.W(first ? S.wb[0] : S.wa[0]), hp, KPd, G, [&](int n, float acc) { pre[n] += acc; });
            } else {
                if (!first) step_matvec(st.W(S.wa[0]), hp + (L - 1) * KD, KPd, G, [&](int n, float acc) { pre[n] += acc; });     // o_prev
                step_matvec(st.W(S.wb[0]), hp, KPd, G, [&](int n, float acc) { pre[n] += acc; });
            }
        } else {
            step_matvec(st.W(S.wa[l]), hc, KPd, G, [&](int n, float acc) { pre[n] = acc + bias[n]; });                           // h^{l-1}_t
            step_matvec(st.W(S.wb[l]), hp + l * KD, KPd, G, [&](int n, float acc) { pre[n] += acc; });
        }
        __syncthreads();                                                         // pre is whole; every read of hc by this layer is over
        const float* c0 = st.V(S.c0);
        for (int j = tid; j < d; j += MMT_DEC_STEP_THREADS) {
            const float cprev = first ? c0[l * d + j] : st.in[(size_t)l * 2 * d + d + j];
            const StepCell u = step_lstm_cell(pre, d, j, cprev, false);
            st.out[(size_t)l * 2 * d + j] = u.h; st.out[(size_t)l * 2 * d + d + j] = u.c;
            hc[j] = step_bf16_round(u.h);
        }
        __syncthreads();                                                         // hc is whole; every read of pre is over
    }

    // 2. read-out (multiTransformer.py:480-483) and the window's mask
    step_readout(st.W(S.w1), st.V(S.b1), st.W(S.w2), st.V(S.b2), L ? hc : es, KPd, hid, S.hdim, S.KPh, P.mask, b, P.y + b, 1);
    step_advance<SLOTS>(pos, b, t, advance);
}

__global__ __launch_bounds__(MMT_DEC_STEP_THREADS) void decoder_step_kernel(const DecStepParams P) { decoder_step_body<false>(P, nullptr, 0, 0); }

__global__ __launch_bounds__(MMT_DEC_STEP_THREADS) void decoder_step_slots_kernel(const DecStepParams P, int* pos, int limit, int advance) {
    decoder_step_body<true>(P, pos, limit, advance);
}
