// Prefill of a stream state from one batch forward (the rule, the two layouts and the limits: step_prefill_plan.h).
//
// encoder_prefill_kernel / encoder_prefill_ring_kernel: one body, two forms, as step_ring.h's for the step.  Grid = (x, B_src, 2 N):
// workgroup (., b, 2 layer + kv) moves the K or V rows of source sequence b of one layer, 16 bytes per lane and item, grid-stride over
// the items of prefill_item.  The columns d_k <= e < dkp of a head's last chunk are zeroed in registers before the store, so the
// workspace's pad columns cannot reach the cache.  (dst, len) of a sequence come by value (dst[b] = b, len[b] = P: the host's form) or
// from two int arrays in device memory (the slots form); either way they pass prefill_seq before any address is formed, with every
// limit taken from the launch arguments, and a pair it refuses is skipped.  Where `pos` is given, the workgroup (0, b, 0) stores
// pos[dst[b]] = len[b]; nothing in this launch reads pos.
//
// decoder_prefill_kernel: grid = B_src; workgroup b copies h_all[len - 1, b, :] and c_all[len - 1, b, :] to copy len & 1 of slot dst[b]
// (n_layers == 1), then stores pos[dst[b]] = len where `pos` is given.  n_layers == 0: the position alone.
//
// Neither kernel reads a word it or its launch writes, workgroups share nothing, and every store lies inside the cache / the carried
// state of sequence dst[b] (tools/prefill_plan_check.cpp walks exactly these functions on host buffers).
#pragma once
#include "common.h"
#include "step_prefill_plan.h"

struct EncPrefillParams {
    const bf16* kr[MMT_STEP_MAX_LAYERS];      // the forward's workspace, per layer
    const bf16* vr[MMT_STEP_MAX_LAYERS];
    bf16* cache;                              // state + cache_off
    const int* dst; const int* len;           // device arrays (B_src) of the slots form, or null: dst[b] = b, len[b] = P
    int* pos;                                 // the stream's positions (B_state), or null
    PrefillGeom g;
};

__device__ __forceinline__ void encoder_prefill_body(const EncPrefillParams& P) {
    const PrefillGeom& G = P.g;
    const int b = blockIdx.y, layer = blockIdx.z >> 1, kv = blockIdx.z & 1;
    if (b >= G.B_src || layer >= G.N) return;
    const int dst_in = P.dst ? __builtin_amdgcn_readfirstlane(P.dst[b]) : b;
    const int len_in = P.len ? __builtin_amdgcn_readfirstlane(P.len[b]) : G.P;
    const PrefillSeq q = prefill_seq(dst_in, len_in, G.P, G.B_state, G.rows, G.ring);
    if (q.dst == MMT_PREFILL_SKIP) return;
    const bf16* src = kv ? P.vr[layer] : P.kr[layer];
    const size_t total = prefill_items(G, q);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const PrefillItem it = prefill_item(G, q, i);
        const PrefillAt at = prefill_at(G, layer, kv, b, q.dst, it.head, it.pos, it.c);
        bf16x8 v = *reinterpret_cast<const bf16x8*>(src + at.src);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 8 * it.c + e < G.dk ? v[e] : (bf16)0.f;        // a select: the pad columns are zeros
        *reinterpret_cast<bf16x8*>(P.cache + at.dst) = v;
    }
    if (P.pos != nullptr && blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) P.pos[q.dst] = q.len;
}

__global__ __launch_bounds__(MMT_PREFILL_THREADS) void encoder_prefill_kernel(const EncPrefillParams P) { encoder_prefill_body(P); }
// The ring form: g.ring is set and g.rows is the span.  The body is the same; its own name shows in a trace which cache was filled.
__global__ __launch_bounds__(MMT_PREFILL_THREADS) void encoder_prefill_ring_kernel(const EncPrefillParams P) { encoder_prefill_body(P); }

struct DecPrefillParams {
    const float* h_all; const float* c_all;   // (P, B_src, d) fp32, time-major (lstm_scan); unused when L == 0
    float* dyn;                               // state + dyn_off
    const int* dst; const int* len;           // as above
    int* pos;
    int B_src, B_state, P, d, L, limit;       // limit: the encoder's capacity, <= 0: none (a ring)
    size_t seq_floats;
};

__global__ __launch_bounds__(MMT_PREFILL_THREADS) void decoder_prefill_kernel(const DecPrefillParams P) {
    const int b = blockIdx.x;
    if (b >= P.B_src) return;
    const int dst_in = P.dst ? __builtin_amdgcn_readfirstlane(P.dst[b]) : b;
    const int len_in = P.len ? __builtin_amdgcn_readfirstlane(P.len[b]) : P.P;
    // the encoder's fill of the same call skipped what this skips: a ring has no limit, so it is given P rows
    const PrefillSeq q = prefill_seq(dst_in, len_in, P.P, P.B_state, P.limit > 0 ? P.limit : P.P, 0);
    if (q.dst == MMT_PREFILL_SKIP) return;
    if (P.L == 1)
        for (int i = threadIdx.x; i < 2 * P.d; i += MMT_PREFILL_THREADS) {
            const int which = i >= P.d, j = i - which * P.d;
            const DecPrefillAt at = dec_prefill_at(P.B_src, P.B_state, P.d, P.seq_floats, b, q.dst, q.len, which, j);
            P.dyn[at.dst] = (which ? P.c_all : P.h_all)[at.src];
        }
    if (P.pos != nullptr && threadIdx.x == 0) P.pos[q.dst] = q.len;
}
