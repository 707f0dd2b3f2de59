// What the one-window step kernels share (encoder_step.h, mfn_step.h): one workgroup of MMT_STEP_THREADS threads per sequence, the
// row in LDS between the stages, every product a vector dot product over prepared bf16 weights [k / 8][output row][k % 8].
#pragma once
#include "common.h"
#include "encoder_step_plan.h"          // MMT_STEP_THREADS

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
