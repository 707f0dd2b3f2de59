// Limits and layout of the stream state of the one-window encoder step (encoder_step.h): plain host C++ with no HIP in it, so that a
// stand-alone program can exercise it (tools/step_plan_check.cpp) and api.hip only adds the base pointer to the offsets computed here.
//
// The state is one buffer of `bytes` bytes:
//   [0, cache_off)        the prepared bf16 weights, per layer four matrices (QKV stacked as 3d rows, Wo, W1, W2), each in the step
//                         kernel's layout [k / 8][output row][k % 8] with k padded to a multiple of 8 by zeros, so that the lane of an
//                         output row reads 16 contiguous bytes per 8 inputs and consecutive lanes read consecutive addresses.  Every
//                         matrix starts at a multiple of 256 bytes.  Written by mmt_encoder_stream_prepare, read by every step.
//   [cache_off, bytes)    the K/V cache, bf16 [layer][K | V][b][head][position < capacity][d_k padded to 8]: one head's sweep reads
//                         contiguous 16-byte rows.  Row t is written by step t (pad columns as zeros) and read by steps > t only.
#pragma once
#include <stddef.h>

#define MMT_STEP_MAX_LAYERS 16            // MAX_LAYERS of api.hip
#define MMT_STEP_MAX_D 512
#define MMT_STEP_MAX_F 2048
#define MMT_STEP_MAX_DK 64
#define MMT_STEP_MAX_CAPACITY 4096        // the limit the attention map has
#define MMT_STEP_MAX_HDKP 2048            // heads x padded d_k: the Q', K_t, V_t rows of the kernel's LDS (d_k = 1 at d_model = 512 is outside)
#define MMT_STEP_THREADS 256

#define MMT_STEP_OK 0
#define MMT_STEP_EINVAL 1                 // MMT_EINVAL
#define MMT_STEP_EUNSUPPORTED 2           // MMT_EUNSUPPORTED

struct StepPlan {
    int dk, dkp, nchunk;                  // head width, padded to 8, in 16-byte chunks
    int KPd, KPf, HDKP;                   // d and f padded to 8 (inputs of a product), h * dkp
    size_t w_off[4], w_elems[4];          // bf16 elements inside one layer's weights: QKV (3d x KPd), Wo (d x KPd), W1 (f x KPd), W2 (d x KPf)
    size_t w_layer_elems;                 // stride between layers
    size_t cache_off;                     // bytes
    size_t cache_row, cache_head, cache_seq, cache_kv, cache_layer, cache_elems;      // strides in bf16 elements
    size_t bytes;
};

static inline size_t step_align256(size_t n) { return (n + 255) / 256 * 256; }

// Returns MMT_STEP_OK, or the error class with *why naming the limit (a static string).
static inline int step_plan(StepPlan& P, int B, int capacity, int d, int h, int f, int N, const char** why) {
    if (B <= 0 || capacity <= 0 || d <= 0 || h <= 0 || f <= 0 || N <= 0) { *why = "encoder stream: non-positive dimension"; return MMT_STEP_EINVAL; }
    if (N > MMT_STEP_MAX_LAYERS) { *why = "encoder stream: n_layers > 16"; return MMT_STEP_EUNSUPPORTED; }
    if (d % h) { *why = "encoder stream: d_model not divisible by h"; return MMT_STEP_EUNSUPPORTED; }
    if (d % 4 || f % 4) { *why = "encoder stream: d_model and d_ff must be multiples of 4"; return MMT_STEP_EUNSUPPORTED; }
    if (d / h > MMT_STEP_MAX_DK) { *why = "encoder stream: d_k > 64 not supported"; return MMT_STEP_EUNSUPPORTED; }
    if (d > MMT_STEP_MAX_D) { *why = "encoder stream: d_model > 512 not supported"; return MMT_STEP_EUNSUPPORTED; }
    if (f > MMT_STEP_MAX_F) { *why = "encoder stream: d_ff > 2048 not supported"; return MMT_STEP_EUNSUPPORTED; }
    if (capacity > MMT_STEP_MAX_CAPACITY) { *why = "encoder stream: capacity > 4096 not supported"; return MMT_STEP_EUNSUPPORTED; }
    P.dk = d / h;
    P.dkp = (P.dk + 7) / 8 * 8;
    P.nchunk = P.dkp / 8;
    P.HDKP = h * P.dkp;
    if (P.HDKP > MMT_STEP_MAX_HDKP) { *why = "encoder stream: h x (d_k padded to 8) > 2048 not supported"; return MMT_STEP_EUNSUPPORTED; }
    P.KPd = (d + 7) / 8 * 8;
    P.KPf = (f + 7) / 8 * 8;
    P.w_elems[0] = (size_t)3 * d * P.KPd;
    P.w_elems[1] = (size_t)d * P.KPd;
    P.w_elems[2] = (size_t)f * P.KPd;
    P.w_elems[3] = (size_t)d * P.KPf;
    size_t off = 0;
    for (int i = 0; i < 4; ++i) { P.w_off[i] = off; off += step_align256(P.w_elems[i] * 2) / 2; }
    P.w_layer_elems = off;
    P.cache_off = step_align256((size_t)N * P.w_layer_elems * 2);
    P.cache_row = (size_t)P.dkp;
    P.cache_head = (size_t)capacity * P.cache_row;
    P.cache_seq = (size_t)h * P.cache_head;
    P.cache_kv = (size_t)B * P.cache_seq;
    P.cache_layer = 2 * P.cache_kv;
    P.cache_elems = (size_t)N * P.cache_layer;
    P.bytes = P.cache_off + step_align256(P.cache_elems * 2);
    return MMT_STEP_OK;
}

// Flat fp32 parameter buffer (mmt_hip.h, mmt_encoder_param_count): offsets of a layer's tensors, in floats
struct StepParamLayout { size_t wq, bq, wk, bk, wv, bv, wo, bo, w1, b1, w2, b2, ln1a, ln1b, ln2a, ln2b, layer, final_a, final_b; };
static inline StepParamLayout step_param_layout(int d, int f, int N) {
    StepParamLayout L;
    const size_t dd = (size_t)d * d, fd = (size_t)f * d;
    size_t o = 0;
    L.wq = o; o += dd; L.bq = o; o += d;
    L.wk = o; o += dd; L.bk = o; o += d;
    L.wv = o; o += dd; L.bv = o; o += d;
    L.wo = o; o += dd; L.bo = o; o += d;
    L.w1 = o; o += fd; L.b1 = o; o += f;
    L.w2 = o; o += fd; L.b2 = o; o += d;
    L.ln1a = o; o += d; L.ln1b = o; o += d; L.ln2a = o; o += d; L.ln2b = o; o += d;
    L.layer = o;
    L.final_a = (size_t)N * o; L.final_b = L.final_a + d;
    return L;
}
