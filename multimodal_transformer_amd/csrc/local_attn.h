// Local attention of the LSTM baselines: the `attn` MLP's softmax and `convolve` over the LSTM outputs
// (transformer/B1-LSTM/models.py:10-25,186-207; the shared copy of MultiLSTM, transformer/SFT/models.py:188-216, is the same code).
//
//   a[b,t,i]   = exp(z[b,t,i] - m[b,i]) / s[b,i]      m, s: max and sum of exp of COLUMN i of z[b] over all T steps.  The reference's
//                                                     nn.Softmax(dim=1) on the (B,T,L) logits normalises over time, padded steps
//                                                     included, not over the L taps its comments describe; this is what it computes.
//   ctx[b,t,:] = sum_{i<L, t-i>=0} a[b,t,i] valid[b,t-i] h[t-i,b,:]      (pad_packed_sequence zeroes h at s >= len_b; pad_shift
//                                                                          brings zeros in for s < 0)
// backward, given dctx:
//   dh[s,b,:]  = valid[b,s] sum_{i<L, s+i<T} a[b,s+i,i] dctx[b,s+i,:]
//   da[b,t,i]  = [t>=i] valid[b,t-i] <dctx[b,t,:], h[t-i,b,:]>
//   dz[b,t,i]  = a[b,t,i] (da[b,t,i] - sum_t' a[b,t',i] da[b,t',i])
//
// The second mode, TAPS (mmt_local_attn_*_taps; models.attend_over_taps, off by default): the softmax runs over the L taps of a row,
// what the reference's comment describes and what an online predictor needs: row t then depends on steps <= t alone.
//   a[b,t,i]   = exp(z[b,t,i] - m[b,t]) / s[b,t]      m, s: max and sum of exp over the L taps of ROW (b,t), summed in tap order.  All L
//                                                     taps take part, also those that reach before step 0 or onto a masked step (their
//                                                     rows of h are zeros, as above)
//   dz[b,t,i]  = a[b,t,i] (da[b,t,i] - sum_i' a[b,t,i'] da[b,t,i'])
//   ctx, dh, da as above.  One body per kernel, the mode a compile-time switch (local_attn_fwd_taps_kernel, local_attn_dz_taps_kernel
//   beside the kernels of the time mode, which keep their names): the forward skips the column statistics, the dz kernel needs no
//   reduction across threads.  la_row_softmax is the one expression of the row's softmax (lstm_step.h uses it too).
//
// fp32 throughout and no MFMA: at most 16 taps, nothing to contract.  The kernels stream h / ctx (forward) and h / dctx / dh (backward)
// once per tile of MMT_LA_TT steps plus an (L-1)-step halo; the rows a tile re-reads for its other taps come from L1 / L2.
// Layouts: z, a, dz (B,T,L); valid (B,T); h, dh (T,B,H) time-major as the LSTM scan has them; ctx, dctx (B,T,H) batch-major.
// Workgroup = 256 threads = 4 waves; lane = one column unit of V floats (V = 4: float4 accesses, V = 1: H % 4 != 0), wave w takes the
// tile's steps w, w+4, ...  grid = (T tiles, column chunks of 64 units, B).
// Deterministic: no atomics; every reduction (column statistics, wave sums, the chunk partials of da) runs in a fixed order.
#pragma once
#include "common.h"

#define MMT_LA_MAXL 16
#define MMT_LA_TT 32
#define MMT_LA_CU 64

template <int V> struct LaVec;
template <> struct LaVec<4> {
    typedef f32x4 T;
    static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ void store(float* p, T v) { *reinterpret_cast<f32x4*>(p) = v; }
    static __device__ __forceinline__ float dot(T a, T b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
    static __device__ __forceinline__ T zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
};
template <> struct LaVec<1> {
    typedef float T;
    static __device__ __forceinline__ T load(const float* p) { return *p; }
    static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
    static __device__ __forceinline__ float dot(T a, T b) { return a * b; }
    static __device__ __forceinline__ T zero() { return 0.f; }
};

__device__ __forceinline__ float la_wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// butterfly: every lane ends with the same bits (a + b == b + a), so any lane may write the sum
__device__ __forceinline__ float la_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Column statistics of z[b] (T x L): s_max[i], s_sum[i] for i < L.  Every workgroup of sequence b computes the same bits (same
// partition over the 256 threads, same reduction order).  red: 4 x 16 floats of LDS.
__device__ __forceinline__ void la_col_stats(const float* __restrict__ zb, int T, int L, float* s_max, float* s_sum, float* red) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float v[MMT_LA_MAXL];
#pragma unroll
    for (int i = 0; i < MMT_LA_MAXL; ++i) v[i] = -INFINITY;
    for (int t = tid; t < T; t += MMT_THREADS) {
#pragma unroll
        for (int i = 0; i < MMT_LA_MAXL; ++i)
            if (i < L) v[i] = fmaxf(v[i], zb[(size_t)t * L + i]);
    }
#pragma unroll
    for (int i = 0; i < MMT_LA_MAXL; ++i)
        if (i < L) {
            const float m = la_wave_max(v[i]);
            if (lane == 0) red[w * MMT_LA_MAXL + i] = m;
        }
    __syncthreads();
    if (tid < L) s_max[tid] = fmaxf(fmaxf(red[tid], red[MMT_LA_MAXL + tid]), fmaxf(red[2 * MMT_LA_MAXL + tid], red[3 * MMT_LA_MAXL + tid]));
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MMT_LA_MAXL; ++i) v[i] = 0.f;
    for (int t = tid; t < T; t += MMT_THREADS) {
#pragma unroll
        for (int i = 0; i < MMT_LA_MAXL; ++i)
            if (i < L) v[i] += expf(zb[(size_t)t * L + i] - s_max[i]);
    }
#pragma unroll
    for (int i = 0; i < MMT_LA_MAXL; ++i)
        if (i < L) {
            const float s = la_wave_sum(v[i]);
            if (lane == 0) red[w * MMT_LA_MAXL + i] = s;
        }
    __syncthreads();
    if (tid < L) s_sum[tid] = ((red[tid] + red[MMT_LA_MAXL + tid]) + red[2 * MMT_LA_MAXL + tid]) + red[3 * MMT_LA_MAXL + tid];
    __syncthreads();
}

// TAPS: a[i] = expf(z[i] - max) / sum over the L taps of one row, max and sum taken in tap-index order.
__device__ __forceinline__ void la_row_softmax(const float* z, int L, float* a) {
    float m = -INFINITY, s = 0.f;
    for (int i = 0; i < L; ++i) m = fmaxf(m, z[i]);
    for (int i = 0; i < L; ++i) s += expf(z[i] - m);
    for (int i = 0; i < L; ++i) a[i] = expf(z[i] - m) / s;
}

// ctx (B,T,H) and a (B,T,L; written by the workgroups of column chunk 0) from z, h, valid.  TAPS: the softmax per row, no statistics.
template <int V, bool TAPS>
__device__ __forceinline__ void local_attn_fwd_body(const float* __restrict__ z, const float* __restrict__ h,
                                                    const float* __restrict__ valid, float* __restrict__ ctx,
                                                    float* __restrict__ attn, int B, int T, int H, int L) {
    typedef LaVec<V> Vec;
    __shared__ float s_max[MMT_LA_MAXL], s_sum[MMT_LA_MAXL], red[4 * MMT_LA_MAXL];
    __shared__ float a_s[MMT_LA_TT][MMT_LA_MAXL];
    __shared__ float v_s[MMT_LA_TT + MMT_LA_MAXL - 1];          // valid[b, t0-15 .. t0+TT-1]
    const int tid = threadIdx.x, b = blockIdx.z, t0 = blockIdx.x * MMT_LA_TT;
    const float* zb = z + (size_t)b * T * L;
    if (TAPS) {
        for (int r = tid; r < MMT_LA_TT; r += MMT_THREADS) {
            const int t = t0 + r;
            if (t < T) {
                la_row_softmax(zb + (size_t)t * L, L, a_s[r]);
                if (blockIdx.y == 0)
                    for (int i = 0; i < L; ++i) attn[((size_t)b * T + t) * L + i] = a_s[r][i];
            }
        }
    } else {
        la_col_stats(zb, T, L, s_max, s_sum, red);
        for (int k = tid; k < MMT_LA_TT * L; k += MMT_THREADS) {
            const int r = k / L, i = k - r * L, t = t0 + r;
            if (t < T) {
                const float a = expf(zb[(size_t)t * L + i] - s_max[i]) / s_sum[i];
                a_s[r][i] = a;
                if (blockIdx.y == 0) attn[((size_t)b * T + t) * L + i] = a;
            }
        }
    }
    for (int k = tid; k < MMT_LA_TT + MMT_LA_MAXL - 1; k += MMT_THREADS) {
        const int t = t0 - (MMT_LA_MAXL - 1) + k;
        v_s[k] = (t >= 0 && t < T) ? valid[(size_t)b * T + t] : 0.f;
    }
    __syncthreads();
    const int cu = blockIdx.y * MMT_LA_CU + (tid & 63);
    if (cu >= H / V) return;                                  // no barrier below
    const size_t col = (size_t)cu * V;
    for (int r = tid >> 6; r < MMT_LA_TT; r += 4) {
        const int t = t0 + r;
        if (t >= T) break;
        typename Vec::T acc = Vec::zero();
#pragma unroll
        for (int i = 0; i < MMT_LA_MAXL; ++i) {
            if (i < L && t - i >= 0) {
                const float vv = v_s[r + MMT_LA_MAXL - 1 - i];
                if (vv != 0.f) acc += (a_s[r][i] * vv) * Vec::load(h + ((size_t)(t - i) * B + b) * H + col);
            }
        }
        Vec::store(ctx + ((size_t)b * T + t) * H + col, acc);
    }
}

// The two instances of the forward's body: the time mode keeps the name (and so the code object) it always had.
template <int V>
__global__ __launch_bounds__(MMT_THREADS) void local_attn_fwd_kernel(const float* __restrict__ z, const float* __restrict__ h,
                                                                     const float* __restrict__ valid, float* __restrict__ ctx,
                                                                     float* __restrict__ attn, int B, int T, int H, int L) {
    local_attn_fwd_body<V, false>(z, h, valid, ctx, attn, B, T, H, L);
}
template <int V>
__global__ __launch_bounds__(MMT_THREADS) void local_attn_fwd_taps_kernel(const float* __restrict__ z, const float* __restrict__ h,
                                                                          const float* __restrict__ valid, float* __restrict__ ctx,
                                                                          float* __restrict__ attn, int B, int T, int H, int L) {
    local_attn_fwd_body<V, true>(z, h, valid, ctx, attn, B, T, H, L);
}

// dh (T,B,H) and the per-chunk partials of da: da_part[chunk][b][t][i] (summed over the chunk's columns).
template <int V>
__global__ __launch_bounds__(MMT_THREADS) void local_attn_bwd_kernel(const float* __restrict__ dctx, const float* __restrict__ attn,
                                                                     const float* __restrict__ h, const float* __restrict__ valid,
                                                                     float* __restrict__ dh, float* __restrict__ da_part,
                                                                     int B, int T, int H, int L) {
    typedef LaVec<V> Vec;
    __shared__ float a_s[MMT_LA_TT + MMT_LA_MAXL - 1][MMT_LA_MAXL];   // a[b, t0 .. t0+TT+14]
    __shared__ float v_s[MMT_LA_TT + MMT_LA_MAXL - 1];                // valid[b, t0-15 .. t0+TT-1]
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.z, t0 = blockIdx.x * MMT_LA_TT;
    for (int k = tid; k < (MMT_LA_TT + MMT_LA_MAXL - 1) * L; k += MMT_THREADS) {
        const int r = k / L, i = k - r * L, t = t0 + r;
        a_s[r][i] = t < T ? attn[((size_t)b * T + t) * L + i] : 0.f;
    }
    for (int k = tid; k < MMT_LA_TT + MMT_LA_MAXL - 1; k += MMT_THREADS) {
        const int t = t0 - (MMT_LA_MAXL - 1) + k;
        v_s[k] = (t >= 0 && t < T) ? valid[(size_t)b * T + t] : 0.f;
    }
    __syncthreads();
    const int cu = blockIdx.y * MMT_LA_CU + lane;
    const bool active = cu < H / V;                           // inactive lanes still take part in the wave sums (with zeros)
    const size_t col = (size_t)cu * V;
    float* dab = da_part + ((size_t)blockIdx.y * B + b) * T * L;
    for (int r = tid >> 6; r < MMT_LA_TT; r += 4) {
        const int t = t0 + r;                                 // wave-uniform
        if (t >= T) break;
        const float vt = v_s[r + MMT_LA_MAXL - 1];
        if (active) {
            typename Vec::T acc = Vec::zero();
            if (vt != 0.f) {
#pragma unroll
                for (int i = 0; i < MMT_LA_MAXL; ++i)
                    if (i < L && t + i < T) acc += a_s[r + i][i] * Vec::load(dctx + ((size_t)b * T + t + i) * H + col);
                acc *= vt;
            }
            Vec::store(dh + ((size_t)t * B + b) * H + col, acc);
        }
        const typename Vec::T g = active ? Vec::load(dctx + ((size_t)b * T + t) * H + col) : Vec::zero();
        float mine = 0.f;
#pragma unroll
        for (int i = 0; i < MMT_LA_MAXL; ++i) {
            if (i < L) {                                      // wave-uniform
                const float vv = t - i >= 0 ? v_s[r + MMT_LA_MAXL - 1 - i] : 0.f;
                float p = 0.f;
                if (active && vv != 0.f) p = vv * Vec::dot(g, Vec::load(h + ((size_t)(t - i) * B + b) * H + col));
                p = la_wave_sum(p);
                if (lane == i) mine = p;
            }
        }
        if (lane < L) dab[(size_t)t * L + lane] = mine;
    }
}

// dz (B,T,L) = a (da - sum_t a da), da = the chunk partials summed in chunk order.  One workgroup per sequence.
// TAPS: dz = a (da - sum_i a da) per row, the sum in tap order: a thread owns a row, nothing crosses threads.
template <bool TAPS>
__device__ __forceinline__ void local_attn_dz_body(const float* __restrict__ attn, const float* __restrict__ da_part,
                                                   float* __restrict__ dz, int B, int T, int L, int nchunks) {
    __shared__ float red[4 * MMT_LA_MAXL], S[MMT_LA_MAXL];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x;
    const size_t TL = (size_t)T * L;
    const float* ab = attn + b * TL;
    if (TAPS) {
        for (int t = tid; t < T; t += MMT_THREADS) {
            float d[MMT_LA_MAXL], s = 0.f;
#pragma unroll
            for (int i = 0; i < MMT_LA_MAXL; ++i)
                if (i < L) {
                    d[i] = 0.f;
                    for (int k = 0; k < nchunks; ++k) d[i] += da_part[((size_t)k * B + b) * TL + (size_t)t * L + i];
                    s += ab[(size_t)t * L + i] * d[i];
                }
#pragma unroll
            for (int i = 0; i < MMT_LA_MAXL; ++i)
                if (i < L) dz[b * TL + (size_t)t * L + i] = ab[(size_t)t * L + i] * (d[i] - s);
        }
        return;
    }
    float acc[MMT_LA_MAXL];
#pragma unroll
    for (int i = 0; i < MMT_LA_MAXL; ++i) acc[i] = 0.f;
    for (int t = tid; t < T; t += MMT_THREADS) {
#pragma unroll
        for (int i = 0; i < MMT_LA_MAXL; ++i)
            if (i < L) {
                float d = 0.f;
                for (int k = 0; k < nchunks; ++k) d += da_part[((size_t)k * B + b) * TL + (size_t)t * L + i];
                acc[i] += ab[(size_t)t * L + i] * d;
            }
    }
#pragma unroll
    for (int i = 0; i < MMT_LA_MAXL; ++i)
        if (i < L) {
            const float s = la_wave_sum(acc[i]);
            if (lane == 0) red[w * MMT_LA_MAXL + i] = s;
        }
    __syncthreads();
    if (tid < L) S[tid] = ((red[tid] + red[MMT_LA_MAXL + tid]) + red[2 * MMT_LA_MAXL + tid]) + red[3 * MMT_LA_MAXL + tid];
    __syncthreads();
    for (int t = tid; t < T; t += MMT_THREADS) {
#pragma unroll
        for (int i = 0; i < MMT_LA_MAXL; ++i)
            if (i < L) {
                float d = 0.f;
                for (int k = 0; k < nchunks; ++k) d += da_part[((size_t)k * B + b) * TL + (size_t)t * L + i];
                dz[b * TL + (size_t)t * L + i] = ab[(size_t)t * L + i] * (d - S[i]);
            }
    }
}

__global__ __launch_bounds__(MMT_THREADS) void local_attn_dz_kernel(const float* __restrict__ attn, const float* __restrict__ da_part,
                                                                    float* __restrict__ dz, int B, int T, int L, int nchunks) {
    local_attn_dz_body<false>(attn, da_part, dz, B, T, L, nchunks);
}
__global__ __launch_bounds__(MMT_THREADS) void local_attn_dz_taps_kernel(const float* __restrict__ attn, const float* __restrict__ da_part,
                                                                         float* __restrict__ dz, int B, int T, int L, int nchunks) {
    local_attn_dz_body<true>(attn, da_part, dz, B, T, L, nchunks);
}
