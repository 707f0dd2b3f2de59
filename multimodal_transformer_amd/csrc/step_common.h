// What the one-window step kernels share (encoder_step.h, mfn_step.h, decoder_step.h, lstm_step.h): one workgroup of MMT_STEP_THREADS
// threads per sequence, the row in LDS between the stages, every product a vector dot product over prepared bf16 weights
// [k / 8][output row][k % 8].  Below step_matvec: the spine of the steps that carry a recurrent state (MFN gate, decoder, LSTM baseline).
#pragma once
#include "common.h"
#include "scan_common.h"                // sigmoid_f, tanh_f
#include "encoder_step_plan.h"          // MMT_STEP_THREADS
#include "step_slots.h"                 // slot_decode

__device__ __forceinline__ float step_bf16_round(float v) { return (float)(bf16)v; }

// sum over the workgroup's 256 threads, the same value in every thread; red: 4 floats of LDS.  Two barriers.
__device__ __forceinline__ float step_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                   // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// epi(n, sum_k W[n][k] in[k]) for every row n < nout of the prepared matrix W ([KP / 8][nout][8] bf16) and the LDS vector in[KP] (pad
// entries zero).  `ks` adjacent lanes share a row where there are fewer rows than threads (chunk kc goes to lane kc % ks; their partial
// sums meet by lane exchange), and MMT_STEP_INFLIGHT loads of 16 bytes are in flight per thread: a step is bound by the latency of these
// dependent round trips, not by their bytes.  Every thread of the workgroup calls it (the trip counts are uniform).
#define MMT_STEP_INFLIGHT 16           // weight chunks a thread has in flight in a product
template <typename Epi>
__device__ __forceinline__ void step_matvec(const bf16* __restrict__ W, const float* in, int KP, int nout, Epi epi) {
    const int sh = nout > 128 ? 0 : nout > 64 ? 1 : nout > 32 ? 2 : 3, ks = 1 << sh;
    const int nkc = KP >> 3, total = nout << sh;
    const bf16x8* wp = reinterpret_cast<const bf16x8*>(W);
    for (int i0 = 0; i0 < total; i0 += MMT_STEP_THREADS) {
        const int i = i0 + threadIdx.x;
        const bool ok = i < total;                             // total is a multiple of ks: the lanes of a row are in or out together
        const int n = ok ? i >> sh : 0, part = i & (ks - 1), end = ok ? nkc : 0;
        float acc = 0.f;
        for (int base = part; base < nkc; base += MMT_STEP_INFLIGHT * ks) {     // uniform trips
            bf16x8 w[MMT_STEP_INFLIGHT];                                        // phase 1: every load of the block is issued ...
#pragma unroll
            for (int u = 0; u < MMT_STEP_INFLIGHT; ++u) {
                const int kc = base + u * ks;
                w[u] = wp[(size_t)(kc < end ? kc : 0) * nout + n];              // a chunk behind the row's end reads chunk 0 and is dropped below
            }
            __builtin_amdgcn_sched_barrier(0);                                  // or the scheduler sinks every load to its first use
#pragma unroll
            for (int u = 0; u < MMT_STEP_INFLIGHT; ++u) {                       // ... phase 2: before the first sum waits for one
                const int kc = base + u * ks;
                const bool live = kc < end;
                const int kcl = live ? kc : 0;
                const f32x4 a = *reinterpret_cast<const f32x4*>(in + 8 * kcl), b = *reinterpret_cast<const f32x4*>(in + 8 * kcl + 4);
                float sum = acc;
#pragma unroll
                for (int e = 0; e < 4; ++e) sum = fmaf((float)w[u][e], a[e], sum);
#pragma unroll
                for (int e = 0; e < 4; ++e) sum = fmaf((float)w[u][4 + e], b[e], sum);
                acc = live ? sum : acc;                                         // a select
            }
        }
        for (int o = 1; o < ks; o <<= 1) acc += __shfl_xor(acc, o);
        if (ok && part == 0) epi(n, acc);
    }
}

// ------------------------------------------------------------------------------------ the spine of the carried-state steps
// mfn_step.h, decoder_step.h and lstm_step.h are one body each in two forms (a compile-time switch): the plain form takes the position t
// as a launch argument, the positioned form reads it from device memory, int pos[B] (step_slots.h).  What the three bodies do in the same
// way stands here once; the headers of the families say what they carry and in which arithmetic.
//
// The positioned form.  Workgroup b reads p = pos[b] once, before anything else, makes it wave-uniform (readfirstlane) and decodes it
// against the launch argument `limit` (<= 0: none).  An idle or full slot is skipped: its row of y is written as zeros and nothing else,
// no carried state, no pos.  Otherwise the body runs with t = p, per sequence, and if `advance` is set one thread stores p + 1 to pos[b]
// after the last stage.  No other workgroup reads pos[b], so workgroups still share nothing and nothing written in a launch is read back
// in it.  Every address derived from pos[b] passes slot_decode first, with the limit taken from the launch arguments; what it lets
// through only selects the copy of the carried state, p & 1 (and, in lstm_step.h, the ring's slots).

// The position this workgroup runs, or MMT_SLOT_SKIP: return at once (the positioned form writes its row of y as zeros first; the widths
// differ, so the family does that).  SLOTS false: t_host, refused when negative as the host refuses it (pos and limit unused).  SLOTS true:
// the one read of pos[b]; uniform, so the position lives in an SGPR.
template <bool SLOTS>
__device__ __forceinline__ int step_enter(const int* pos, int b, int limit, int t_host) {
    if (SLOTS) return slot_decode(__builtin_amdgcn_readfirstlane(pos[b]), limit);
    return t_host < 0 ? MMT_SLOT_SKIP : t_host;
}

// if `advance` is set one thread stores t + 1 to pos[b], after the last stage.  t < INT_MAX by slot_decode: no overflow.  Read by the
// next launch only
template <bool SLOTS>
__device__ __forceinline__ void step_advance(int* pos, int b, int t, int advance) {
    if (SLOTS && advance != 0 && threadIdx.x == 0) pos[b] = t + 1;
}

// A prepared stream state as a step sees it: the prepared matrices and vectors by the plan's byte offsets, and the two copies of the
// carried state of sequence b, fp32 [copy][b][seq_floats] from byte dyn_off.  Step t reads copy t & 1 (`in`) and writes copy (t + 1) & 1
// (`out`).  At t == 0 the family reads no word of `in`, by branch, never by multiplying.
struct StepState {
    const char* base;
    const float* in;
    float* out;
    __device__ __forceinline__ const bf16* W(size_t off) const { return reinterpret_cast<const bf16*>(base + off); }
    __device__ __forceinline__ const float* V(size_t off) const { return reinterpret_cast<const float*>(base + off); }
};
__device__ __forceinline__ StepState step_state(char* state, size_t dyn_off, size_t seq_floats, int t, int B, int b) {
    float* dyn = reinterpret_cast<float*>(state + dyn_off);
    return {state, dyn + ((size_t)(t & 1) * B + b) * seq_floats, dyn + ((size_t)((t & 1) ^ 1) * B + b) * seq_floats};
}

// Unit j of an LSTM cell of width H from its gate pre-activations pre[i f g o][H]: c = f c_prev + i g, h = o tanh(c), all fp32.
// `no_forget`: c = i g, the form of a cell whose c_prev is absent (lstm_step.h at position 0; c_prev is not looked at then).  A cell that
// starts from a value, or from a zero it multiplies (decoder_step.h, mfn_step.h), passes false: f * 0 + x is not bit for bit x.
struct StepCell { float h, c; };
__device__ __forceinline__ StepCell step_lstm_cell(const float* pre, int H, int j, float cprev, bool no_forget) {
    const float ig = sigmoid_f(pre[j]), fg = sigmoid_f(pre[H + j]), gg = tanh_f(pre[2 * H + j]), og = sigmoid_f(pre[3 * H + j]);
    const float c = no_forget ? ig * gg : fg * cprev + ig * gg;
    return {og * tanh_f(c), c};
}

// The two-layer read-out and the window's mask: y[n] = (bf16(relu(bf16(top) W1^T + b1)) W2^T + b2)[n] * mask[b] for n < nout (mask null:
// no factor).  top[KPtop] holds rounded values, hid[KPhid] is LDS of the workgroup whose pad [nhid, KPhid) is zero already.  Every thread
// calls it; one barrier inside, between the products.
__device__ __forceinline__ void step_readout(const bf16* W1, const float* b1, const bf16* W2, const float* b2, const float* top, int KPtop,
                                             float* hid, int nhid, int KPhid, const float* mask, int b, float* y, int nout) {
    step_matvec(W1, top, KPtop, nhid, [&](int n, float acc) { hid[n] = step_bf16_round(fmaxf(acc + b1[n], 0.f)); });
    __syncthreads();
    const bool masked = mask != nullptr;
    const float mk = masked ? mask[b] : 1.f;
    step_matvec(W2, hid, KPhid, nout, [&](int n, float acc) {
        const float v = acc + b2[n];
        y[n] = masked ? v * mk : v;
    });
}
