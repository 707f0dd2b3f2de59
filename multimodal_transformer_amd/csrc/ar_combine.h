// Autoregressive read-out of the LSTM baseline MultiARLSTM (transformer/MFT/models.py:376-399; the SFT, B2-Trans, B3-MFN,
// Performance-Eval and B1-LSTM copies are the same code).  in_part (B,T) = decoder(context), w (B,T,K) = autoreg(context), K = ar_order.
//
//   teacher-forced (a target is given, :381-386):  p[b,t] = in_part[b,t] + sum_{i<K} w[b,t,i] target[b,t-i],   target[b,s<0] = 0
//                                                  (pad_shift pads with zeros, not with tgt_init; tap 0 reads the CURRENT target)
//   free-running  (no target, :388-397):           p[b,t] = in_part[b,t] + sum_{k<K} w[b,t,k] p[b,t-K+k],      p[b,s<0] = p_init
//                                                  (tap K-1 reads the newest prediction: the reverse of the order above)
//   out[b,t] = p[b,t] mask[b,t]                    (:399)
//
// The reference detaches the history of the free-running loop (:392), so in both branches the backward is element-wise, with
// g = dout * mask and hist[b,t,k] = target[b,t-k] (zero before step 0) or p[b,t-K+k] (p_init before step 0):
//   d in_part[b,t] = g[b,t],   d w[b,t,k] = g[b,t] hist[b,t,k]
//
// fp32 throughout and no MFMA: at most 16 taps per step, nothing to contract.  No atomics, no LDS, no barriers.
//
// The free-running forward is a linear recurrence with time-varying coefficients; the reference runs it as a Python loop of about five
// small launches per step.  Here: one wave per sequence, MMT_AR_SEQS sequences (waves) per workgroup.  The wave reads in_part and w in
// chunks of MMT_AR_CHUNK = 64 steps, lane = step (the chunk of w is one contiguous run of 64 K floats), the next chunk's loads in flight
// while the current one is walked.  The walk takes step j's coefficients out of lane j with v_readlane (they become scalar operands of
// the multiply-adds) and keeps the last K predictions in registers, the same in every lane; lane j keeps p of its own step and the chunk
// is written back with one coalesced store.  The taps over the older predictions do not depend on the newest one, so the chain from
// step to step is ONE multiply-add (tap K-1), which is the floor for this recurrence.  The walk runs in groups of MMT_AR_GROUP steps;
// a last group that is not full walks zero coefficients (at most MMT_AR_GROUP - 1 idle steps per sequence), nothing of it is stored.
#pragma once
#include "common.h"

#define MMT_AR_MAXK 16
#define MMT_AR_CHUNK 64          // steps per chunk = lanes of a wave
#define MMT_AR_GROUP 16          // steps per unrolled group of the walk
#define MMT_AR_SEQS 4            // sequences per workgroup, one wave each

__device__ __forceinline__ float ar_lane_value(float v, int lane) {       // v of lane `lane` (wave-uniform) as a scalar
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int K>
__global__ __launch_bounds__(MMT_AR_SEQS * 64) void ar_free_fwd_kernel(const float* __restrict__ in_part, const float* __restrict__ w,
                                                                        const float* __restrict__ mask, float p_init,
                                                                        float* __restrict__ p, float* __restrict__ out, int B, int T) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * MMT_AR_SEQS + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (b >= B) return;                                  // whole waves leave: no barrier follows
    const float* cb = in_part + (size_t)b * T;
    const float* wb = w + (size_t)b * T * K;
    float hist[K];                                       // hist[k] = p[t-K+k], wave-uniform
#pragma unroll
    for (int k = 0; k < K; ++k) hist[k] = p_init;
    float c_nx = 0.f, w_nx[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w_nx[k] = 0.f;
    if (lane < T) {
        c_nx = cb[lane];
#pragma unroll
        for (int k = 0; k < K; ++k) w_nx[k] = wb[(size_t)lane * K + k];
    }
    for (int t0 = 0; t0 < T; t0 += MMT_AR_CHUNK) {
        const float c_cur = c_nx;
        float w_cur[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w_cur[k] = w_nx[k];
        const int tn = t0 + MMT_AR_CHUNK + lane;          // this lane's step of the next chunk
        c_nx = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) w_nx[k] = 0.f;
        if (tn < T) {
            c_nx = cb[tn];
#pragma unroll
            for (int k = 0; k < K; ++k) w_nx[k] = wb[(size_t)tn * K + k];
        }
        const int n = min(MMT_AR_CHUNK, T - t0);           // live steps of this chunk; lanes >= n hold zero coefficients
        float mine = 0.f;
        for (int j0 = 0; j0 < n; j0 += MMT_AR_GROUP) {
#pragma unroll
            for (int jj = 0; jj < MMT_AR_GROUP; ++jj) {
                const int j = j0 + jj;
                float acc = ar_lane_value(c_cur, j);
#pragma unroll
                for (int k = 0; k < K - 1; ++k) acc = fmaf(ar_lane_value(w_cur[k], j), hist[k], acc);
                const float pj = fmaf(ar_lane_value(w_cur[K - 1], j), hist[K - 1], acc);      // the only link to step j - 1
#pragma unroll
                for (int k = 0; k < K - 1; ++k) hist[k] = hist[k + 1];
                hist[K - 1] = pj;
                mine = lane == j ? pj : mine;
            }
        }
        const int t = t0 + lane;
        if (t < T) {
            const size_t o = (size_t)b * T + t;
            p[o] = mine;
            out[o] = mine * mask[o];
        }
    }
}

// Teacher-forced forward: element-wise with a K-step halo into the target.  One thread per (b,t), grid-stride.
__global__ __launch_bounds__(256) void ar_teacher_fwd_kernel(const float* __restrict__ in_part, const float* __restrict__ w,
                                                              const float* __restrict__ mask, const float* __restrict__ target,
                                                              float* __restrict__ p, float* __restrict__ out, int B, int T, int K) {
    const size_t n = (size_t)B * T;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < n; o += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(o % T);
        const float* wr = w + o * K;
        const float* tr = target + o;                      // tr[-i] = target[b,t-i] while i <= t
        float acc = 0.f;
        const int taps = min(K, t + 1);
        for (int i = 0; i < taps; ++i) acc = fmaf(wr[i], tr[-i], acc);
        const float v = in_part[o] + acc;
        p[o] = v;
        out[o] = v * mask[o];
    }
}

// Backward of both branches: one thread per (b,t,k), grid-stride; the thread of tap 0 writes d in_part.
// hist = target (teacher != 0; tap k reads step t-k, zero before step 0) or the saved p (tap k reads step t-K+k, pad before step 0).
__global__ __launch_bounds__(256) void ar_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ mask,
                                                      const float* __restrict__ hist, float pad, int teacher,
                                                      float* __restrict__ din, float* __restrict__ dw, int B, int T, int K) {
    const size_t n = (size_t)B * T * K;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t o = e / K;
        const int k = (int)(e - o * K), t = (int)(o % T);
        const float g = dout[o] * mask[o];
        const int back = teacher ? k : K - k;              // the tap reads step t - back
        const float h = back <= t ? hist[o - back] : pad;
        dw[e] = g * h;
        if (k == 0) din[o] = g;
    }
}
