// Limits and layout of the stream state of the one-window MFN gate step (mfn_step.h): plain host C++ with no HIP in it, so that a
// stand-alone program can exercise it (tools/mfn_step_plan_check.cpp) and api.hip only adds the base pointer to the offsets computed here.
//
// The state is one buffer of `bytes` bytes, every piece starting at a multiple of 256 bytes:
//   the prepared bf16 weights, each matrix in the step kernels' layout [k / 8][output row][k % 8] with k padded to a multiple of 8 by
//       zeros: per modality W_ih (4H x D) and W_hh (4H x H); att1_fc1 (128 x A), att1_fc2 (A x 128), att2_fc1 (256 x A),
//       att2_fc2 (128 x 256); Wa (128 x A) and Wm (128 x 128), the column split of gamma{1,2}_fc1.weight with gamma1's 64 rows above
//       gamma2's; W2 of either gate (128 x 64); out_fc1 (64 x (sum H + 128)), out_fc2 (output_dim x 64).  A = 2 sum H.
//   the fp32 biases: per modality b_ih + b_hh (4H), then those of the ten gate layers (gamma1_fc1's above gamma2_fc1's).
//       Both written by mmt_mfn_stream_prepare, read by every step.
//   [dyn_off, bytes)  two copies of the carried state, fp32 [copy][b][h of every modality (sum H) | c of every modality (sum H) | mem (128)]:
//       step t reads copy t & 1 (at t == 0 nothing: zeros stand for it) and writes copy (t + 1) & 1.
#pragma once
#include <stddef.h>
#include "step_prep.h"

#define MMT_MFN_STEP_MAX_MODS 4
#define MMT_MFN_STEP_MAX_SH 256           // sum of the LSTM hidden sizes: one cell unit per thread
#define MMT_MFN_STEP_MAX_IN 512           // input width of a modality
#define MMT_MFN_STEP_MAX_OUT 256          // output_dim: one read-out row per thread
#define MMT_MFN_STEP_MD 128               // MFN_MD of mfn_scan.h
#define MMT_MFN_STEP_HG 64                // MFN_HG
#define MMT_MFN_STEP_ATT1 128             // hidden units of att1_fc1
#define MMT_MFN_STEP_ATT2 256             // of att2_fc1
#define MMT_MFN_STEP_OUTH 64              // of out_fc1
#define MMT_MFN_STEP_THREADS 256

#define MMT_MFN_STEP_OK 0
#define MMT_MFN_STEP_EINVAL 1             // MMT_EINVAL
#define MMT_MFN_STEP_EUNSUPPORTED 2       // MMT_EUNSUPPORTED

// matrices and bias vectors behind the per-modality ones, in the state's order
enum { MFN_W_A11 = 0, MFN_W_A12, MFN_W_A21, MFN_W_A22, MFN_W_WA, MFN_W_WM, MFN_W_W21, MFN_W_W22, MFN_W_O1, MFN_W_O2, MFN_W_COUNT };
enum { MFN_B_A11 = 0, MFN_B_A12, MFN_B_A21, MFN_B_A22, MFN_B_G1, MFN_B_G21, MFN_B_G22, MFN_B_O1, MFN_B_O2, MFN_B_COUNT };

struct MfnStepPlan {
    int nm, SH, A, KL, KPL, OD;                       // modalities, sum H, 2 sum H, sum H + 128 and that padded to 8, output_dim
    int D[MMT_MFN_STEP_MAX_MODS], KPD[MMT_MFN_STEP_MAX_MODS];      // input width, padded to 8
    int H[MMT_MFN_STEP_MAX_MODS], KPH[MMT_MFN_STEP_MAX_MODS];      // hidden size, padded to 8
    int hoff[MMT_MFN_STEP_MAX_MODS + 1];              // first unit of a modality among the sum H
    int xoff[MMT_MFN_STEP_MAX_MODS + 1];              // first float of a modality's padded input row in the kernel's LDS
    int hpoff[MMT_MFN_STEP_MAX_MODS + 1];             // of its padded h_prev row
    size_t wih[MMT_MFN_STEP_MAX_MODS], whh[MMT_MFN_STEP_MAX_MODS], blstm[MMT_MFN_STEP_MAX_MODS];     // byte offsets
    size_t w[MFN_W_COUNT], b[MFN_B_COUNT];            // byte offsets
    int w_rows[MFN_W_COUNT], w_k[MFN_W_COUNT], w_kp[MFN_W_COUNT], b_n[MFN_B_COUNT];
    size_t dyn_off, seq_floats, dyn_floats;           // the carried state: byte offset, floats per sequence and copy, floats in all
    size_t bytes;
};

static inline size_t mfn_step_align256(size_t n) { return (n + 255) / 256 * 256; }
static inline int mfn_step_pad8(int n) { return (n + 7) / 8 * 8; }

// Returns MMT_MFN_STEP_OK, or the error class with *why naming the limit (a static string).
static inline int mfn_step_plan(MfnStepPlan& P, int B, int nmods, const int* in_dims, const int* hidden, int output_dim, const char** why) {
    if (!in_dims || !hidden) { *why = "mfn stream: null pointer argument"; return MMT_MFN_STEP_EINVAL; }
    if (B <= 0 || nmods <= 0 || output_dim <= 0) { *why = "mfn stream: non-positive dimension"; return MMT_MFN_STEP_EINVAL; }
    if (nmods > MMT_MFN_STEP_MAX_MODS) { *why = "mfn stream: more than 4 modalities not supported"; return MMT_MFN_STEP_EUNSUPPORTED; }
    for (int m = 0; m < nmods; ++m)
        if (in_dims[m] <= 0 || hidden[m] <= 0) { *why = "mfn stream: non-positive dimension"; return MMT_MFN_STEP_EINVAL; }
    if (output_dim > MMT_MFN_STEP_MAX_OUT) { *why = "mfn stream: output_dim > 256 not supported"; return MMT_MFN_STEP_EUNSUPPORTED; }
    P.nm = nmods; P.OD = output_dim;
    P.hoff[0] = P.xoff[0] = P.hpoff[0] = 0;
    for (int m = 0; m < MMT_MFN_STEP_MAX_MODS; ++m) {
        const bool on = m < nmods;
        if (on && in_dims[m] % 4) { *why = "mfn stream: input widths must be multiples of 4"; return MMT_MFN_STEP_EUNSUPPORTED; }
        if (on && in_dims[m] > MMT_MFN_STEP_MAX_IN) { *why = "mfn stream: input width > 512 not supported"; return MMT_MFN_STEP_EUNSUPPORTED; }
        if (on && hidden[m] % 4) { *why = "mfn stream: LSTM hidden sizes must be multiples of 4"; return MMT_MFN_STEP_EUNSUPPORTED; }
        if (on && hidden[m] > MMT_MFN_STEP_MAX_SH) { *why = "mfn stream: sum of the LSTM hidden sizes > 256 not supported"; return MMT_MFN_STEP_EUNSUPPORTED; }
        P.D[m] = on ? in_dims[m] : 0; P.KPD[m] = mfn_step_pad8(P.D[m]);
        P.H[m] = on ? hidden[m] : 0; P.KPH[m] = mfn_step_pad8(P.H[m]);
        P.hoff[m + 1] = P.hoff[m] + P.H[m];
        P.xoff[m + 1] = P.xoff[m] + P.KPD[m];
        P.hpoff[m + 1] = P.hpoff[m] + P.KPH[m];
        if (P.hoff[m + 1] > MMT_MFN_STEP_MAX_SH) { *why = "mfn stream: sum of the LSTM hidden sizes > 256 not supported"; return MMT_MFN_STEP_EUNSUPPORTED; }
    }
    P.SH = P.hoff[nmods]; P.A = 2 * P.SH; P.KL = P.SH + MMT_MFN_STEP_MD; P.KPL = mfn_step_pad8(P.KL);
    const int rows[MFN_W_COUNT] = {MMT_MFN_STEP_ATT1, P.A, MMT_MFN_STEP_ATT2, MMT_MFN_STEP_MD, 2 * MMT_MFN_STEP_HG, 2 * MMT_MFN_STEP_HG,
                                   MMT_MFN_STEP_MD, MMT_MFN_STEP_MD, MMT_MFN_STEP_OUTH, output_dim};
    const int ks[MFN_W_COUNT] = {P.A, MMT_MFN_STEP_ATT1, P.A, MMT_MFN_STEP_ATT2, P.A, MMT_MFN_STEP_MD, MMT_MFN_STEP_HG, MMT_MFN_STEP_HG,
                                 P.KL, MMT_MFN_STEP_OUTH};
    const int bn[MFN_B_COUNT] = {MMT_MFN_STEP_ATT1, P.A, MMT_MFN_STEP_ATT2, MMT_MFN_STEP_MD, 2 * MMT_MFN_STEP_HG, MMT_MFN_STEP_MD, MMT_MFN_STEP_MD,
                                 MMT_MFN_STEP_OUTH, output_dim};
    size_t off = 0;
    for (int m = 0; m < MMT_MFN_STEP_MAX_MODS; ++m) {
        P.wih[m] = off; off += mfn_step_align256((size_t)4 * P.H[m] * P.KPD[m] * 2);
        P.whh[m] = off; off += mfn_step_align256((size_t)4 * P.H[m] * P.KPH[m] * 2);
    }
    for (int i = 0; i < MFN_W_COUNT; ++i) {
        P.w_rows[i] = rows[i]; P.w_k[i] = ks[i]; P.w_kp[i] = mfn_step_pad8(ks[i]);
        P.w[i] = off; off += mfn_step_align256((size_t)rows[i] * P.w_kp[i] * 2);
    }
    for (int m = 0; m < MMT_MFN_STEP_MAX_MODS; ++m) { P.blstm[m] = off; off += mfn_step_align256((size_t)4 * P.H[m] * 4); }
    for (int i = 0; i < MFN_B_COUNT; ++i) { P.b_n[i] = bn[i]; P.b[i] = off; off += mfn_step_align256((size_t)bn[i] * 4); }
    P.dyn_off = off;
    P.seq_floats = (size_t)2 * P.SH + MMT_MFN_STEP_MD;
    P.dyn_floats = (size_t)2 * B * P.seq_floats;
    P.bytes = P.dyn_off + mfn_step_align256(P.dyn_floats * 4);
    return MMT_MFN_STEP_OK;
}

// What mmt_mfn_stream_prepare writes, as the job table of step_prep_kernel (step_prep.h): every matrix and vector of the layout above
// and no byte of the carried state.  lstm_params: per modality nn.LSTMCell's weight_ih (4H,D), weight_hh (4H,H), bias_ih, bias_hh;
// gate_params: att1_fc1.{w,b} att1_fc2 att2_fc1 att2_fc2 gamma1_fc1 gamma1_fc2 gamma2_fc1 gamma2_fc2 out_fc1 out_fc2 (_MfnGateFn's order).
static_assert(MMT_STEP_PREP_MATS == 2 * MMT_MFN_STEP_MAX_MODS + 12 && MMT_STEP_PREP_VECS == MMT_MFN_STEP_MAX_MODS + 10, "the table's capacities");
static inline void mfn_step_prep_table(const MfnStepPlan& S, const float* const* lstm_params, const float* const* gate_params,
                                       StepPrepParams& P, size_t& most) {
    P.nmat = P.nvec = 0;
    most = 1;
    auto mat = [&](const float* src, size_t dst, int ld, int col0, int rows, int K, int nout, int row0) {
        step_prep_mat(P, most, src, ld, col0, nullptr, 0, 0, dst + (size_t)row0 * 8 * 2, rows, K, nout);
    };
    auto vec = [&](const float* a, const float* b, size_t dst, int n, int dst0) { step_prep_vec(P, a, b, dst + (size_t)4 * dst0, n); };
    for (int m = 0; m < S.nm; ++m) {
        const float* const* lp = lstm_params + 4 * m;
        mat(lp[0], S.wih[m], S.D[m], 0, 4 * S.H[m], S.D[m], 4 * S.H[m], 0);
        mat(lp[1], S.whh[m], S.H[m], 0, 4 * S.H[m], S.H[m], 4 * S.H[m], 0);
        vec(lp[2], lp[3], S.blstm[m], 4 * S.H[m], 0);
    }
    const float* const* g = gate_params;
    const int A = S.A, MD = MMT_MFN_STEP_MD, HG = MMT_MFN_STEP_HG;
    mat(g[0], S.w[MFN_W_A11], A, 0, MMT_MFN_STEP_ATT1, A, MMT_MFN_STEP_ATT1, 0);   vec(g[1], nullptr, S.b[MFN_B_A11], MMT_MFN_STEP_ATT1, 0);
    mat(g[2], S.w[MFN_W_A12], MMT_MFN_STEP_ATT1, 0, A, MMT_MFN_STEP_ATT1, A, 0);   vec(g[3], nullptr, S.b[MFN_B_A12], A, 0);
    mat(g[4], S.w[MFN_W_A21], A, 0, MMT_MFN_STEP_ATT2, A, MMT_MFN_STEP_ATT2, 0);   vec(g[5], nullptr, S.b[MFN_B_A21], MMT_MFN_STEP_ATT2, 0);
    mat(g[6], S.w[MFN_W_A22], MMT_MFN_STEP_ATT2, 0, MD, MMT_MFN_STEP_ATT2, MD, 0); vec(g[7], nullptr, S.b[MFN_B_A22], MD, 0);
    for (int i = 0; i < 2; ++i) {                             // gamma{1,2}: fc1 = [attended part | memory part], gamma1's rows above gamma2's
        const float* w1 = g[8 + 4 * i]; const float* b1 = g[9 + 4 * i]; const float* w2 = g[10 + 4 * i]; const float* b2 = g[11 + 4 * i];
        mat(w1, S.w[MFN_W_WA], A + MD, 0, HG, A, 2 * HG, i * HG);
        mat(w1, S.w[MFN_W_WM], A + MD, A, HG, MD, 2 * HG, i * HG);
        vec(b1, nullptr, S.b[MFN_B_G1], HG, i * HG);
        mat(w2, S.w[i ? MFN_W_W22 : MFN_W_W21], HG, 0, MD, HG, MD, 0);
        vec(b2, nullptr, S.b[i ? MFN_B_G22 : MFN_B_G21], MD, 0);
    }
    mat(g[16], S.w[MFN_W_O1], S.KL, 0, MMT_MFN_STEP_OUTH, S.KL, MMT_MFN_STEP_OUTH, 0);    vec(g[17], nullptr, S.b[MFN_B_O1], MMT_MFN_STEP_OUTH, 0);
    mat(g[18], S.w[MFN_W_O2], MMT_MFN_STEP_OUTH, 0, S.OD, MMT_MFN_STEP_OUTH, S.OD, 0);    vec(g[19], nullptr, S.b[MFN_B_O2], S.OD, 0);
}
