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
// The positioned form, decoder_step_slots_kernel: the same body (a compile-time switch), with the position of each sequence read from
// device memory, int pos[B] (step_slots.h).  Workgroup b reads p = pos[b] once, before anything else, makes it wave-uniform
// (readfirstlane) and decodes it against the launch argument `limit` (<= 0: none).  An idle or full slot is skipped: its row of y is
// written as zeros and nothing else, no carried state, no pos.  Otherwise the body runs with t = p, per sequence, and if `advance` is
// set one thread stores p + 1 to pos[b] after the last stage.  No other workgroup reads pos[b], so both contracts above hold.  The last
// sentence of the state discipline changes for this form: every address derived from pos[b] passes slot_decode first, with the limit
// taken from the launch arguments; what it lets through only selects the copy, p & 1.
#pragma once
#include "common.h"
#include "scan_common.h"                 // sigmoid_f, tanh_f
#include "step_common.h"
#include "decoder_step_plan.h"
#include "step_slots.h"                  // slot_decode

static_assert(MMT_DEC_STEP_THREADS == MMT_STEP_THREADS, "step_matvec is written for one workgroup size");

struct DecStepParams {
    const float* e;                            // (B, d): the encoder step's output row
    const float* mask;                         // (B) or nullptr
    float* y;                                  // (B, 1)
    char* state;
    int t, B;
    DecStepPlan pl;
};

// SLOTS false: t = P.t (pos, limit and advance unused).  SLOTS true: t = slot_decode(pos[b], limit), P.t unused.
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
    int t;
    if (SLOTS) {
        t = slot_decode(__builtin_amdgcn_readfirstlane(pos[b]), limit);          // the one read of pos[b]; uniform, so t lives in an SGPR
        if (t == MMT_SLOT_SKIP) {                                                // idle or full: a zero row and nothing else
            if (tid == 0) P.y[b] = 0.f;
            return;
        }
    } else {
        t = P.t;
        if (t < 0) return;                                                       // the host refuses such a call
    }
    const int d = S.d, KPd = S.KPd, L = S.L, G = 4 * d;
    const bool first = t == 0;                                                   // uniform: no word of the carried state is read
    float* dyn = reinterpret_cast<float*>(P.state + S.dyn_off);
    const float* st_in = dyn + ((size_t)(t & 1) * P.B + b) * S.seq_floats;
    float* st_out = dyn + ((size_t)((t & 1) ^ 1) * P.B + b) * S.seq_floats;
    auto W = [&](size_t off) { return reinterpret_cast<const bf16*>(P.state + off); };
    auto Bv = [&](size_t off) { return reinterpret_cast<const float*>(P.state + off); };

    // 0. stage e and, per layer, what multiplies the layer's recurrent matrix (rounded: both feed products only)
    {
        const float* er = P.e + (size_t)b * d;
        const float* h0 = Bv(S.h0);
        for (int k = tid; k < KPd; k += MMT_DEC_STEP_THREADS) {
            es[k] = k < d ? step_bf16_round(er[k]) : 0.f;
            hc[k] = 0.f;                                                         // the cells write [0, d): the pad stays zero
        }
        for (int l = 0; l < L; ++l)
            for (int k = tid; k < KPd; k += MMT_DEC_STEP_THREADS) {
                float v = 0.f;
                if (k < d) v = step_bf16_round(first ? h0[l * d + k] : st_in[(size_t)l * 2 * d + k]);
                hp[l * KD + k] = v;
            }
        for (int k = S.hdim + tid; k < S.KPh; k += MMT_DEC_STEP_THREADS) hid[k] = 0.f;          // the pad of the read-out's second input
        __syncthreads();
    }

    // 1. the layers, bottom up; a row of pre has the same owner in every product of a layer (step_matvec: the owner depends on nout alone)
    for (int l = 0; l < L; ++l) {
        const float* bias = Bv(S.bl[l]);
        if (l == 0) {
            step_matvec(W(S.wx), es, KPd, G, [&](int n, float acc) { pre[n] = acc + bias[n]; });
            if (L == 1) {                                                        // W_rec on h_prev; at position 0 o_prev = 0: W_hh on dec_h0
                step_matvec(W(first ? S.wb[0] : S.wa[0]), hp, KPd, G, [&](int n, float acc) { pre[n] += acc; });
            } else {
                if (!first) step_matvec(W(S.wa[0]), hp + (L - 1) * KD, KPd, G, [&](int n, float acc) { pre[n] += acc; });     // o_prev
                step_matvec(W(S.wb[0]), hp, KPd, G, [&](int n, float acc) { pre[n] += acc; });
            }
        } else {
            step_matvec(W(S.wa[l]), hc, KPd, G, [&](int n, float acc) { pre[n] = acc + bias[n]; });                           // h^{l-1}_t
            step_matvec(W(S.wb[l]), hp + l * KD, KPd, G, [&](int n, float acc) { pre[n] += acc; });
        }
        __syncthreads();                                                         // pre is whole; every read of hc by this layer is over
        const float* c0 = Bv(S.c0);
        for (int j = tid; j < d; j += MMT_DEC_STEP_THREADS) {
            const float cprev = first ? c0[l * d + j] : st_in[(size_t)l * 2 * d + d + j];
            const float ig = sigmoid_f(pre[j]), fg = sigmoid_f(pre[d + j]), gg = tanh_f(pre[2 * d + j]), og = sigmoid_f(pre[3 * d + j]);
            const float c = fg * cprev + ig * gg;
            const float h = og * tanh_f(c);
            st_out[(size_t)l * 2 * d + j] = h; st_out[(size_t)l * 2 * d + d + j] = c;
            hc[j] = step_bf16_round(h);
        }
        __syncthreads();                                                         // hc is whole; every read of pre is over
    }

    // 2. read-out (multiTransformer.py:480-483) and the window's mask
    {
        const float* top = L ? hc : es;
        const float* b1 = Bv(S.b1);
        step_matvec(W(S.w1), top, KPd, S.hdim, [&](int n, float acc) { hid[n] = step_bf16_round(fmaxf(acc + b1[n], 0.f)); });
        __syncthreads();
        const float* b2 = Bv(S.b2);
        const bool masked = P.mask != nullptr;
        const float mk = masked ? P.mask[b] : 1.f;
        step_matvec(W(S.w2), hid, S.KPh, 1, [&](int n, float acc) {
            const float v = acc + b2[n];
            P.y[b + n] = masked ? v * mk : v;
        });
    }
    if (SLOTS && advance != 0 && tid == 0) pos[b] = t + 1;                       // t < INT_MAX by slot_decode: no overflow.  Read by the next launch only
}

__global__ __launch_bounds__(MMT_DEC_STEP_THREADS) void decoder_step_kernel(const DecStepParams P) { decoder_step_body<false>(P, nullptr, 0, 0); }

__global__ __launch_bounds__(MMT_DEC_STEP_THREADS) void decoder_step_slots_kernel(const DecStepParams P, int* pos, int limit, int advance) {
    decoder_step_body<true>(P, pos, limit, advance);
}
