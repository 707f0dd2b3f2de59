// One window of the MFN gate per launch: mfn_step_kernel advances the per-modality LSTM cells, the attention over the cell states, the
// delta-memory and the read-out by one position t for each of B sequences (transformer/MFT/multiTransformer.py:200-247 for one t),
// carrying (h_m, c_m, mem) in a stream state (layout and limits: mfn_step_plan.h).  Its output row is what MFN.forward in eval mode
// gives at [:, t] of the windows stepped so far.
//
// Shape of the kernel, as encoder_step.h: grid = B, one workgroup of 256 threads per sequence; workgroups share nothing and never
// communicate, so a sequence's result does not depend on the batch it is stepped in.  Every product is step_matvec (step_common.h)
// over prepared bf16 weights, the row lives in LDS between the stages, and the stages are a chain of dependent round trips.
//
// Arithmetic: the batch path's, row for row (functional._MfnGateFn and the scans it runs between): the left operand of every product
// is rounded to bf16 (x_m, h_prev, cStar, relu(att1_fc1), attended, relu(att2_fc1), mem_prev, u, [h ; mem], relu(out_fc1)), every weight
// is bf16, and sums, biases, the activations (sigmoid_f / tanh_f of scan_common.h), the softmax, c, h, mem and everything stored are
// fp32.  No site depends on a tile, so the same reference serves the step and the batch path (tests/mfn_stream_ref.py).
//
// State discipline.  Step t reads copy t & 1 of (h, c, mem) and writes copy (t + 1) & 1: nothing written in a launch is read back in
// it.  At t == 0 no word of either copy is read (zeros stand for the state, by branch, not by multiplying), so a state of any bit
// pattern cannot reach a result and a new recording needs no launch.  Every address comes from (b < B, t & 1) and the plan's offsets
// alone: t is a launch argument checked by the host, and the kernel returns at once when t < 0.  No address is derived from device data.
//
// The positioned form, mfn_step_slots_kernel: the same body with the position of each sequence read from device memory, as
// step_common.h describes it for every carried-state step; both contracts above hold for it, with slot_decode in the host's place.
#pragma once
#include "common.h"
#include "step_common.h"                 // step_matvec and the spine: step_enter, step_state, step_lstm_cell, step_readout, step_advance
#include "mfn_step_plan.h"

static_assert(MMT_MFN_STEP_THREADS == MMT_STEP_THREADS, "step_matvec is written for one workgroup size");

struct MfnStepParams {
    const float* x[MMT_MFN_STEP_MAX_MODS];     // (B, D_m) each
    const float* mask;                         // (B) or nullptr
    float* y;                                  // (B, output_dim)
    char* state;
    int t, B;
    MfnStepPlan pl;
};

// maximum over the workgroup's 256 threads, the same value in every thread; red: 4 floats of LDS.  Two barriers.
__device__ __forceinline__ float step_block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();                                   // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// SLOTS: the positioned form (step_common.h: step_enter).
template <bool SLOTS>
__device__ __forceinline__ void mfn_step_body(const MfnStepParams& P, int* pos, int limit, int advance) {
    constexpr int MD = MMT_MFN_STEP_MD, HG = MMT_MFN_STEP_HG, SHM = MMT_MFN_STEP_MAX_SH;
    __shared__ __attribute__((aligned(16))) float xs[MMT_MFN_STEP_MAX_MODS * MMT_MFN_STEP_MAX_IN];     // bf16(x_m), padded rows
    __shared__ __attribute__((aligned(16))) float hs[SHM + 8 * MMT_MFN_STEP_MAX_MODS];                 // bf16(h_prev of m), padded rows
    __shared__ __attribute__((aligned(16))) float pre[4 * SHM];                                        // gate pre-activations, [m][i f g o][H_m]
    __shared__ __attribute__((aligned(16))) float cs[2 * SHM];                                         // cStar, fp32
    __shared__ __attribute__((aligned(16))) float csr[2 * SHM];                                        // bf16(cStar)
    __shared__ __attribute__((aligned(16))) float lg[2 * SHM];                                         // att1's logits
    __shared__ __attribute__((aligned(16))) float at[2 * SHM];                                         // bf16(attended)
    __shared__ __attribute__((aligned(16))) float a1[MMT_MFN_STEP_ATT1];                               // bf16(relu(att1_fc1))
    __shared__ __attribute__((aligned(16))) float a2[MMT_MFN_STEP_ATT2];                               // bf16(relu(att2_fc1))
    __shared__ __attribute__((aligned(16))) float memf[MD];                                            // mem_prev, fp32
    __shared__ __attribute__((aligned(16))) float memr[MD];                                            // bf16(mem_prev)
    __shared__ __attribute__((aligned(16))) float us[2 * HG];                                          // apre, then bf16(u)
    __shared__ __attribute__((aligned(16))) float chat[MD];
    __shared__ __attribute__((aligned(16))) float g1[MD];
    __shared__ __attribute__((aligned(16))) float last[SHM + MD + 8];                                  // bf16([h of every modality ; mem])
    __shared__ __attribute__((aligned(16))) float hid[MMT_MFN_STEP_OUTH];                              // bf16(relu(out_fc1))
    __shared__ float red[4];

    const MfnStepPlan& L = P.pl;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int t = step_enter<SLOTS>(pos, b, limit, P.t);
    if (t == MMT_SLOT_SKIP) {                                                    // idle or full: a zero row and nothing else
        if (SLOTS) for (int n = tid; n < L.OD; n += MMT_MFN_STEP_THREADS) P.y[(size_t)b * L.OD + n] = 0.f;
        return;
    }
    const int SH = L.SH, A = L.A, nm = L.nm;
    const bool first = t == 0;                                                   // uniform: no word of the state is read
    const StepState st = step_state(P.state, L.dyn_off, L.seq_floats, t, P.B, b);

    // the cell unit of this thread: modality mu, unit ju of it
    int mu = 0;
    for (int m = 1; m < nm; ++m) mu = tid >= L.hoff[m] ? m : mu;
    const bool unit = tid < SH;
    const int ju = tid - L.hoff[mu], Hu = L.H[mu];

    // 0. stage x_m, h_prev and mem_prev (rounded where they feed a product); c_prev of this thread's unit stays in a register
    float cprev = 0.f;
    if (!first && unit) cprev = st.in[SH + tid];
    for (int m = 0; m < nm; ++m) {
        const int D = L.D[m], H = L.H[m];
        const float* xr = P.x[m] + (size_t)b * D;
        for (int k = tid; k < L.KPD[m]; k += MMT_MFN_STEP_THREADS) xs[L.xoff[m] + k] = k < D ? step_bf16_round(xr[k]) : 0.f;
        for (int k = tid; k < L.KPH[m]; k += MMT_MFN_STEP_THREADS) {
            float v = 0.f;
            if (!first && k < H) v = step_bf16_round(st.in[L.hoff[m] + k]);
            hs[L.hpoff[m] + k] = v;
        }
    }
    if (tid < MD) {
        float v = 0.f;
        if (!first) v = st.in[2 * SH + tid];
        memf[tid] = v; memr[tid] = step_bf16_round(v);
    }
    for (int k = L.KL + tid; k < L.KPL; k += MMT_MFN_STEP_THREADS) last[k] = 0.f;           // the pad of the read-out's input
    __syncthreads();

    // 1. LSTM cells (:207-208): pre = bf16(x) W_ih^T + (b_ih + b_hh) + bf16(h_prev) W_hh^T; a row has the same owner in both products
    for (int m = 0; m < nm; ++m) {
        float* pm = pre + 4 * L.hoff[m];
        const float* bias = st.V(L.blstm[m]);
        step_matvec(st.W(L.wih[m]), xs + L.xoff[m], L.KPD[m], 4 * L.H[m], [&](int n, float acc) { pm[n] = acc + bias[n]; });
        if (!first) step_matvec(st.W(L.whh[m]), hs + L.hpoff[m], L.KPH[m], 4 * L.H[m], [&](int n, float acc) { pm[n] += acc; });
    }
    __syncthreads();
    if (unit) {
        const StepCell u = step_lstm_cell(pre + 4 * L.hoff[mu], Hu, ju, cprev, false);
        const float h = u.h, c = u.c;
        st.out[tid] = h; st.out[SH + tid] = c;
        // 2. cStar = [c_prev of every modality ; c_new of every modality] (:212-217)
        cs[tid] = cprev; cs[SH + tid] = c;
        csr[tid] = step_bf16_round(cprev); csr[SH + tid] = step_bf16_round(c);
        last[tid] = step_bf16_round(h);
    }
    __syncthreads();

    // 3. attention over the A features (:218-219), softmax_mul_fwd_kernel's formula
    {
        const float* b1 = st.V(L.b[MFN_B_A11]);
        step_matvec(st.W(L.w[MFN_W_A11]), csr, A, MMT_MFN_STEP_ATT1, [&](int n, float acc) { a1[n] = step_bf16_round(fmaxf(acc + b1[n], 0.f)); });
        __syncthreads();
        const float* b2 = st.V(L.b[MFN_B_A12]);
        step_matvec(st.W(L.w[MFN_W_A12]), a1, MMT_MFN_STEP_ATT1, A, [&](int n, float acc) { lg[n] = acc + b2[n]; });
        __syncthreads();
        float mx = -INFINITY;
        for (int n = tid; n < A; n += MMT_MFN_STEP_THREADS) mx = fmaxf(mx, lg[n]);
        mx = step_block_max(mx, red);
        float sum = 0.f;
        for (int n = tid; n < A; n += MMT_MFN_STEP_THREADS) sum += __expf(lg[n] - mx);
        sum = step_block_sum(sum, red);
        const float inv = 1.0f / sum;
        for (int n = tid; n < A; n += MMT_MFN_STEP_THREADS) at[n] = step_bf16_round((__expf(lg[n] - mx) * inv) * cs[n]);
        __syncthreads();
    }

    // 4. att2_fc1 and the gates' first layers (:220-223): all three read bf16(attended) or bf16(mem_prev) only
    {
        const float* b21 = st.V(L.b[MFN_B_A21]);
        step_matvec(st.W(L.w[MFN_W_A21]), at, A, MMT_MFN_STEP_ATT2, [&](int n, float acc) { a2[n] = step_bf16_round(fmaxf(acc + b21[n], 0.f)); });
        const float* bg = st.V(L.b[MFN_B_G1]);
        step_matvec(st.W(L.w[MFN_W_WA]), at, A, 2 * HG, [&](int n, float acc) {                 // apre; with mem = 0 it is already u's argument
            const float v = acc + bg[n];
            us[n] = first ? step_bf16_round(fmaxf(v, 0.f)) : v;
        });
        if (!first)                                                                          // the same owner per row as the product above
            step_matvec(st.W(L.w[MFN_W_WM]), memr, MD, 2 * HG, [&](int n, float acc) { us[n] = step_bf16_round(fmaxf(us[n] + acc, 0.f)); });
        __syncthreads();
    }

    // 5. chat (:220), the gates (:222-223) and the memory (:224)
    {
        const float* b22 = st.V(L.b[MFN_B_A22]);
        step_matvec(st.W(L.w[MFN_W_A22]), a2, MMT_MFN_STEP_ATT2, MD, [&](int n, float acc) { chat[n] = tanh_f(acc + b22[n]); });
        const float* bz1 = st.V(L.b[MFN_B_G21]);
        step_matvec(st.W(L.w[MFN_W_W21]), us, HG, MD, [&](int n, float acc) { g1[n] = sigmoid_f(acc + bz1[n]); });
        __syncthreads();
        const float* bz2 = st.V(L.b[MFN_B_G22]);
        step_matvec(st.W(L.w[MFN_W_W22]), us + HG, HG, MD, [&](int n, float acc) {
            const float mem = g1[n] * memf[n] + sigmoid_f(acc + bz2[n]) * chat[n];
            st.out[2 * SH + n] = mem;
            last[SH + n] = step_bf16_round(mem);
        });
        __syncthreads();
    }

    // 6. read-out (:241-247) and the window's mask
    step_readout(st.W(L.w[MFN_W_O1]), st.V(L.b[MFN_B_O1]), st.W(L.w[MFN_W_O2]), st.V(L.b[MFN_B_O2]), last, L.KPL, hid, MMT_MFN_STEP_OUTH, MMT_MFN_STEP_OUTH,
                 P.mask, b, P.y + (size_t)b * L.OD, L.OD);
    step_advance<SLOTS>(pos, b, t, advance);
}

__global__ __launch_bounds__(MMT_MFN_STEP_THREADS) void mfn_step_kernel(const MfnStepParams P) { mfn_step_body<false>(P, nullptr, 0, 0); }

__global__ __launch_bounds__(MMT_MFN_STEP_THREADS) void mfn_step_slots_kernel(const MfnStepParams P, int* pos, int limit, int advance) {
    mfn_step_body<true>(P, pos, limit, advance);
}
