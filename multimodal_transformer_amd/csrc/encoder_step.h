// One window of a causal encoder stack per launch: encoder_step_kernel advances all N layers and the final LayerNorm by one position t
// for each of B sequences, against a K/V cache (layout and limits: encoder_step_plan.h).  Its output row is what Encoder.forward with
// causal attention gives at [:, t] (transformer/MFT/multiTransformer.py:73-76; departs from :27-31 as the causal kernels of attn.h do).
//
// Shape of the kernel.  Grid = B, one workgroup of 256 threads per sequence; workgroups share nothing and never communicate (no flag,
// no spin, no atomic), so a sequence's result does not depend on the batch it is stepped in.  One row cannot fill an MFMA tile: every
// product is a vector dot product over prepared bf16 weights [k / 8][row][k % 8] (16 bytes per load, consecutive lanes at consecutive
// addresses, fp32 accumulation; step_matvec).  The row lives in LDS between the stages.  The kernel is a chain of dependent round
// trips, so every loop over global memory issues a block of loads first and sums behind a scheduling barrier.
//
// Attention.  Heads are dealt to the four waves.  A wave splits its 64 lanes into key groups of `cl` lanes (cl = chunks of 8 columns of
// the padded head, rounded up to a power of two): lane (kg, c) holds chunk c of Q' in registers, reads chunk c of key kg, kg + KG, ...
// and the `cl` partial dot products are summed by lane exchange.  Two sweeps over the cached keys: the first takes the row's EXACT maximum m of the scores
// (log2 domain), the second recomputes each score and accumulates
//     P_j = bf16(2^(S_j - m)),   l = sum_j 2^(S_j - m) in fp32 (the unrounded values),   ctx = bf16((sum_j P_j V_j) / l).
// This is NOT the batch kernel's rule: attn.h keeps a lazily moved maximum per 32-query tile, a decision that looks at later queries of
// the tile, which a one-query step cannot see.  tests/stream_ref.py restates the rule above.  The rounding sites are otherwise those of
// the batch path (tests/causal_ref.py): bf16 LayerNorm outputs, weights, Q' = bf16((q + b_q) log2(e) / sqrt(d_k)), K, V, P, the merged
// context and relu(hid); fp32 sums, biases, residuals and LayerNorm.  A blanked query row (mask_t[b] == 0) has Q' = 0 by SELECT, so it is
// uniform over its t + 1 keys; its K_t and V_t are appended like any other.
//
// Cache discipline.  K_t and V_t of this step take part in the attention from LDS; cache row t is written and never read in step t,
// rows > t are never touched, rows < t are only read.  The pad columns of a row are written as zeros, so a cache with any bit pattern
// behind position t cannot reach a result.  Every cache address comes from (b, layer, head, j <= t < capacity) alone: t and capacity
// are launch arguments checked by the host, and the kernel returns at once when t is outside [0, capacity).  No address is derived
// from device data.
//
// The positioned form, encoder_step_slots_kernel: the same body (a compile-time switch, as attn.h's plain / keys / causal), with the
// position of each sequence read from device memory, int pos[B] (step_slots.h).  Workgroup b reads p = pos[b] once, before anything
// else, makes it wave-uniform (readfirstlane: the sweeps' trip counts stay scalar, as with t a launch argument) and decodes it.  An idle
// or full slot is skipped: its row of y is written as zeros and nothing else, no cache row, no pos.  Otherwise the body runs with t = p,
// and if `advance` is set one thread stores p + 1 to pos[b] after the last stage.  No other workgroup reads pos[b], so both contracts
// above hold: nothing written in a launch is read back in it, and workgroups do not communicate.  The last sentence of the cache
// discipline changes for this form: every address derived from pos[b] passes slot_decode first, with the limit (capacity) taken from
// the launch arguments, so such an address is that of a row j <= t < capacity exactly as above.
//
// The ring forms, encoder_step_ring_kernel and encoder_step_ring_slots_kernel: the same body again (a second compile-time switch), for a
// stack with a span (attn.h's band kernels: window t attends t - span + 1 .. t).  The cache has `span` rows, position j lives in row
// j mod span, and the sweeps cover the last n = min(t, span - 1) positions in AGE order, oldest first, dealt to lanes as positions are
// above (step_ring.h states the rule and why the order matters).  The cache discipline is the one above with "row t mod span" for
// "row t": that row held position t - span, which is outside the band, so it is written and never read in step t; every other row
// is only read or not touched.  Every cache address comes from (b, layer, head, a row < span) with the row computed from t and span by
// step_ring.h's three functions; no position below INT_MAX is refused, so the positioned form decodes with no limit and stores
// p + 1 <= INT_MAX, the value that never runs.
#pragma once
#include "common.h"
#include "encoder_step_plan.h"
#include "step_common.h"          // step_bf16_round, step_block_sum, step_matvec
#include "step_slots.h"           // slot_decode
#include "step_ring.h"            // ring_keys, ring_first_row, ring_row

struct EncStepParams {
    const float* x;            // (B, d)
    const float* mask;         // (B) or nullptr
    const float* params;       // flat fp32 parameters (biases and LayerNorm weights are read from here)
    float* y;                  // (B, d)
    const bf16* weights;       // prepared, state + 0
    bf16* cache;               // state + cache_off
    int t, B, capacity, d, h, f, N;
    int dk, dkp, nchunk, KPd, KPf;
    float eps, qscale;
    size_t w_off[4], w_layer_elems;
    size_t cache_head, cache_seq, cache_kv, cache_layer;
    StepParamLayout pl;
};

// mmt_encoder_stream_prepare: blockIdx.y = matrix (0 QKV, 1 Wo, 2 W1, 3 W2), blockIdx.z = layer; grid-stride over the destination.
struct EncStepPrepParams {
    const float* params; bf16* weights;
    int d, f, KPd, KPf;
    size_t w_off[4], w_layer_elems;
    StepParamLayout pl;
};

__global__ __launch_bounds__(256) void encoder_step_prep_kernel(const EncStepPrepParams P) {
    const int mat = blockIdx.y, layer = blockIdx.z;
    const int d = P.d, f = P.f;
    const int nout = mat == 0 ? 3 * d : mat == 2 ? f : d;
    const int K = mat == 3 ? f : d, KP = mat == 3 ? P.KPf : P.KPd;
    const float* lp = P.params + (size_t)layer * P.pl.layer;
    bf16* dst = P.weights + (size_t)layer * P.w_layer_elems + P.w_off[mat];
    const size_t total = (size_t)nout * KP;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const size_t r = i >> 3;
        const int n = (int)(r % nout), k = (int)(r / nout) * 8 + j;
        const float* src;
        if (mat == 0) src = lp + (n < d ? P.pl.wq : n < 2 * d ? P.pl.wk : P.pl.wv) + (size_t)(n % d) * d;
        else if (mat == 1) src = lp + P.pl.wo + (size_t)n * d;
        else if (mat == 2) src = lp + P.pl.w1 + (size_t)n * d;
        else src = lp + P.pl.w2 + (size_t)n * f;
        dst[i] = k < K ? (bf16)src[k] : (bf16)0.f;
    }
}

// LayerNorm of the reference (unbiased std, eps added to the std) of the LDS row xs[d]; every thread gets (mean, rstd)
__device__ __forceinline__ void step_ln_stats(const float* xs, int d, float eps, float* red, float& mean, float& rstd) {
    float s = 0.f;
    for (int c = threadIdx.x; c < d; c += MMT_STEP_THREADS) s += xs[c];
    mean = step_block_sum(s, red) / (float)d;
    float q = 0.f;
    for (int c = threadIdx.x; c < d; c += MMT_STEP_THREADS) { const float u = xs[c] - mean; q += u * u; }
    q = step_block_sum(q, red);
    rstd = 1.0f / (sqrtf(q / (float)(d - 1)) + eps);
}

#define MMT_STEP_KEYS_INFLIGHT 4       // keys a lane has in flight in an attention sweep

// SLOTS false: t = P.t (pos and advance unused).  SLOTS true: t = slot_decode(pos[b], limit), P.t unused.
// RING false: the cache has `capacity` rows, position j lives in row j, the limit is the capacity.  RING true (step_ring.h): P.capacity
// is the span, the cache is a ring of that many rows, the sweeps cover the last n = min(t, span - 1) positions in age order and there is
// no limit.  With RING false the three ring values below are the constants (n = t, r0 = 0, row = age), so those two instances compile
// from the source they had.
template <bool SLOTS, bool RING>
__device__ __forceinline__ void encoder_step_body(const EncStepParams& P, int* pos, int advance) {
    __shared__ __attribute__((aligned(16))) float xs[MMT_STEP_MAX_D];            // the residual row, fp32
    __shared__ __attribute__((aligned(16))) float ns[MMT_STEP_MAX_D];            // bf16(LayerNorm) / the merged bf16 context, as floats
    __shared__ __attribute__((aligned(16))) float hs[MMT_STEP_MAX_F];            // bf16(relu(hid))
    __shared__ __attribute__((aligned(16))) float qs[MMT_STEP_MAX_HDKP];         // Q', K_t, V_t: [head][dkp], pad columns zero
    __shared__ __attribute__((aligned(16))) float ks[MMT_STEP_MAX_HDKP];
    __shared__ __attribute__((aligned(16))) float vs[MMT_STEP_MAX_HDKP];
    __shared__ float red[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    int t;
    // Where p + 1 goes after the last stage (null: nowhere).  Thread 0 parks the address in LDS and fetches it back itself at the end:
    // held in SGPRs across the whole body, which already spills ~220 of them to VGPR lanes, it cost the kernel a private segment.
    __shared__ int* next;
    if (SLOTS && tid == 0) next = advance != 0 ? pos + b : nullptr;
    if (SLOTS) {
        t = slot_decode(__builtin_amdgcn_readfirstlane(pos[b]), RING ? 0 : P.capacity);      // the one read of pos[b]; uniform, so t lives in an SGPR
        if (t == MMT_SLOT_SKIP) {                                                // idle or full: a zero row and nothing else
            for (int n = tid; n < P.d; n += MMT_STEP_THREADS) P.y[(size_t)b * P.d + n] = 0.f;
            return;
        }
    } else {
        t = P.t;
        if (t < 0 || (RING ? t == INT_MAX : t >= P.capacity)) return;            // the host refuses such a call; never index the cache with it
    }
    // the cached keys of this step: n of them, age i in row `at(i)`; K_t and V_t go to row wrow.  RING: one modulo, on the uniform t
    const int span = P.capacity;
    const int n = RING ? ring_keys(t, span) : t;
    const int r0 = RING ? ring_first_row(t, n, span) : 0;
    const int wrow = RING ? ring_row(r0, n, span) : t;
    auto at = [&](int i) { return RING ? ring_row(r0, i, span) : i; };
    const int d = P.d, h = P.h, f = P.f, dk = P.dk, dkp = P.dkp, nchunk = P.nchunk, KPd = P.KPd, KPf = P.KPf;
    const bool blank = P.mask != nullptr && P.mask[b] == 0.f;

    for (int c = tid; c < d; c += MMT_STEP_THREADS) xs[c] = P.x[(size_t)b * d + c];
    for (int c = d + tid; c < KPd; c += MMT_STEP_THREADS) ns[c] = 0.f;            // the pads of the product inputs: written once, never again
    for (int c = f + tid; c < KPf; c += MMT_STEP_THREADS) hs[c] = 0.f;
    for (int i = tid; i < h * (dkp - dk); i += MMT_STEP_THREADS) {
        const int o = (i / (dkp - dk)) * dkp + dk + i % (dkp - dk);
        qs[o] = 0.f; ks[o] = 0.f; vs[o] = 0.f;
    }
    __syncthreads();

    // lane roles of the attention sweeps
    const int cl = nchunk <= 1 ? 1 : nchunk <= 2 ? 2 : nchunk <= 4 ? 4 : 8;     // lanes per key
    const int KG = 64 / cl, kg = lane / cl;
    const bool chunk_ok = lane % cl < nchunk;                                    // d_k padded to 3, 5, 6 or 7 chunks leaves lanes of a group idle
    const int c = chunk_ok ? lane % cl : 0;                                      // an idle lane forms chunk 0's addresses and loads nothing

    for (int layer = 0; layer < P.N; ++layer) {
        const float* lp = P.params + (size_t)layer * P.pl.layer;
        const bf16* W = P.weights + (size_t)layer * P.w_layer_elems;
        float mean, rstd;

        // 1. LayerNorm 1 -> ns
        step_ln_stats(xs, d, P.eps, red, mean, rstd);
        for (int n = tid; n < d; n += MMT_STEP_THREADS)
            ns[n] = step_bf16_round(lp[P.pl.ln1a + n] * ((xs[n] - mean) * rstd) + lp[P.pl.ln1b + n]);
        __syncthreads();

        // 2. Q', K_t, V_t -> LDS
        step_matvec(W + P.w_off[0], ns, KPd, 3 * d, [&](int n, float acc) {
            const int which = n / d, col = n - which * d;
            const int o = (col / dk) * dkp + col % dk;
            if (which == 0) {
                const float q = step_bf16_round((acc + lp[P.pl.bq + col]) * P.qscale);
                qs[o] = blank ? 0.f : q;
            } else if (which == 1) {
                ks[o] = step_bf16_round(acc + lp[P.pl.bk + col]);
            } else {
                vs[o] = step_bf16_round(acc + lp[P.pl.bv + col]);
            }
        });
        __syncthreads();

        // 3. append K_t, V_t: cache row wrow (t; in a ring t mod span) of every head, 16 bytes per store (bf16 of a bf16-valued float is exact)
        bf16* Kc = P.cache + (size_t)layer * P.cache_layer + (size_t)b * P.cache_seq;
        bf16* Vc = Kc + P.cache_kv;
        for (int i = tid; i < 2 * h * nchunk; i += MMT_STEP_THREADS) {
            const int kv = i / (h * nchunk), r = i - kv * (h * nchunk), head = r / nchunk, ch = r - head * nchunk;
            const float* src = (kv ? vs : ks) + head * dkp + 8 * ch;
            bf16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (bf16)src[e];
            *reinterpret_cast<bf16x8*>((kv ? Vc : Kc) + (size_t)head * P.cache_head + (size_t)wrow * dkp + 8 * ch) = v;
        }

        // 4. attention of the one query over the n cached keys (ages 0 .. n - 1: positions t - n .. t - 1) and key t; key t from LDS
        for (int head = wave; head < h; head += 4) {
            const bf16* Kh = Kc + (size_t)head * P.cache_head;
            const bf16* Vh = Vc + (size_t)head * P.cache_head;
            float q[8], kt[8], vt[8];                                            // chunk c of Q' and of this step's key and value, from LDS
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                q[e] = chunk_ok ? qs[head * dkp + 8 * c + e] : 0.f;
                kt[e] = chunk_ok ? ks[head * dkp + 8 * c + e] : 0.f;
                vt[e] = chunk_ok ? vs[head * dkp + 8 * c + e] : 0.f;
            }
            float st = 0.f;                                                      // the score of key t: every lane has it
#pragma unroll
            for (int e = 0; e < 8; ++e) st = fmaf(q[e], kt[e], st);
            for (int o = 1; o < cl; o <<= 1) st += __shfl_xor(st, o);
            // first sweep over the cached keys, ages j < n: the row's exact maximum.  The loads are unconditional (a lane behind n reads the
            // row of age 0, which is cached inside this loop) so that several are in flight; what such a lane read is dropped by a select.
            float m = st;
            for (int j0 = 0; j0 < n; j0 += MMT_STEP_KEYS_INFLIGHT * KG) {
                bf16x8 kk[MMT_STEP_KEYS_INFLIGHT];
#pragma unroll
                for (int u = 0; u < MMT_STEP_KEYS_INFLIGHT; ++u) {
                    const int j = j0 + u * KG + kg;
                    kk[u] = *reinterpret_cast<const bf16x8*>(Kh + (size_t)at(j < n ? j : 0) * dkp + 8 * c);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < MMT_STEP_KEYS_INFLIGHT; ++u) {
                    const bool valid = j0 + u * KG + kg < n;
                    float part = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) part = fmaf(q[e], (float)kk[u][e], part);
                    part = chunk_ok ? part : 0.f;
                    for (int o = 1; o < cl; o <<= 1) part += __shfl_xor(part, o);
                    m = valid ? fmaxf(m, part) : m;
                }
            }
            for (int o = cl; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
            // second sweep: the score again, P, l and P V
            float l = 0.f, acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
            for (int j0 = 0; j0 < n; j0 += MMT_STEP_KEYS_INFLIGHT * KG) {
                bf16x8 kk[MMT_STEP_KEYS_INFLIGHT], v8[MMT_STEP_KEYS_INFLIGHT];
#pragma unroll
                for (int u = 0; u < MMT_STEP_KEYS_INFLIGHT; ++u) {
                    const int j = j0 + u * KG + kg;
                    const size_t row = (size_t)at(j < n ? j : 0) * dkp + 8 * c;
                    kk[u] = *reinterpret_cast<const bf16x8*>(Kh + row);
                    v8[u] = *reinterpret_cast<const bf16x8*>(Vh + row);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < MMT_STEP_KEYS_INFLIGHT; ++u) {
                    const bool valid = j0 + u * KG + kg < n;
                    float part = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) part = fmaf(q[e], (float)kk[u][e], part);
                    part = chunk_ok ? part : 0.f;
                    for (int o = 1; o < cl; o <<= 1) part += __shfl_xor(part, o);
                    const float p = valid ? fast_exp2(part - m) : 0.f;           // selects: nothing behind n is ever multiplied
                    const float pb = step_bf16_round(p);
                    l += p;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = fmaf(pb, valid && chunk_ok ? (float)v8[u][e] : 0.f, acc[e]);
                }
            }
            {   // key t, counted once: by key group 0
                const float p = kg == 0 ? fast_exp2(st - m) : 0.f;
                const float pb = step_bf16_round(p);
                l += p;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pb, kg == 0 ? vt[e] : 0.f, acc[e]);
            }
            for (int o = cl; o < 64; o <<= 1) {
                l += __shfl_xor(l, o);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], o);
            }
            if (kg == 0 && chunk_ok) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (8 * c + e < dk) ns[head * dk + 8 * c + e] = step_bf16_round(acc[e] / l);       // the merged context
            }
        }
        __syncthreads();

        // 5. output projection + residual
        step_matvec(W + P.w_off[1], ns, KPd, d, [&](int n, float acc) { xs[n] += acc + lp[P.pl.bo + n]; });
        __syncthreads();

        // 6. LayerNorm 2 -> ns
        step_ln_stats(xs, d, P.eps, red, mean, rstd);
        for (int n = tid; n < d; n += MMT_STEP_THREADS)
            ns[n] = step_bf16_round(lp[P.pl.ln2a + n] * ((xs[n] - mean) * rstd) + lp[P.pl.ln2b + n]);
        __syncthreads();

        // 7. FFN + residual
        step_matvec(W + P.w_off[2], ns, KPd, f, [&](int n, float acc) { hs[n] = step_bf16_round(fmaxf(acc + lp[P.pl.b1 + n], 0.f)); });
        __syncthreads();
        step_matvec(W + P.w_off[3], hs, KPf, d, [&](int n, float acc) { xs[n] += acc + lp[P.pl.b2 + n]; });
        __syncthreads();
    }

    float mean, rstd;
    step_ln_stats(xs, d, P.eps, red, mean, rstd);
    const float* fa = P.params + P.pl.final_a;
    const float* fb = P.params + P.pl.final_b;
    for (int n = tid; n < d; n += MMT_STEP_THREADS)
        P.y[(size_t)b * d + n] = fa[n] * ((xs[n] - mean) * rstd) + fb[n];
    if (SLOTS && tid == 0) {
        int* const w = next;
        if (w != nullptr) *w = t + 1;                                            // t < INT_MAX (slot_decode): no overflow.  Read by the next launch only
    }
}

__global__ __launch_bounds__(MMT_STEP_THREADS) void encoder_step_kernel(const EncStepParams P) { encoder_step_body<false, false>(P, nullptr, 0); }

__global__ __launch_bounds__(MMT_STEP_THREADS) void encoder_step_slots_kernel(const EncStepParams P, int* pos, int advance) {
    encoder_step_body<true, false>(P, pos, advance);
}

// The ring forms (step_ring.h): P.capacity is the span, the cache has that many rows, and no position below INT_MAX is refused.
__global__ __launch_bounds__(MMT_STEP_THREADS) void encoder_step_ring_kernel(const EncStepParams P) { encoder_step_body<false, true>(P, nullptr, 0); }

__global__ __launch_bounds__(MMT_STEP_THREADS) void encoder_step_ring_slots_kernel(const EncStepParams P, int* pos, int advance) {
    encoder_step_body<true, true>(P, pos, advance);
}
