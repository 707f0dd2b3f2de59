// A tile of up to 16 consecutive windows of a causal encoder stack per launch: encoder_extend_kernel advances all N layers and the final
// LayerNorm for positions t .. t + c - 1 (1 <= c <= 16) of each sequence, from ANY t, on the stream state of the one-window step
// (encoder_step_plan.h: the prepared weights and the K/V cache, untouched in layout), so a stream mixes step, prefill and extend
// freely.  Its rows are what encoder_step_kernel gives for the same windows one at a time, to fp32 summation order: the rule of
// encoder_step.h per row, which tests/stream_ref.py and tests/ring_stream_ref.py restate.  Index rule and limits: encoder_extend_plan.h.
//
// Shape of the kernel.  Grid = sequences of the call, one workgroup of 256 threads per sequence; workgroups share nothing and never
// communicate (no flag, no spin, no atomic), so a sequence's rows do not depend on the batch it is extended in.  Sixteen windows are
// one MFMA tile: every product (QKV, out-proj, FFN 1 and 2) is mfma_f32_16x16x32_bf16 with fp32 accumulation,
//     D[feature n][window w] = sum_k W[n][k] in[w][k],
// with the prepared weights [k / 8][output row][k % 8] as the A operand exactly as they lie (lane l reads 16 contiguous bytes of output
// row n0 + (l & 15) at k-block 4 kb + (l >> 4); consecutive lanes read consecutive addresses) and the tile's rows, bf16 in LDS, as the B
// operand (lane l: row l & 15, k = 32 kb + 8 (l >> 4) ..).  The accumulator holds features n0 + 4 (l >> 4) + reg of window l & 15.  The
// sixteen-row output tiles of a product are dealt to the four waves; the weights are read once per tile, not once per window.  A
// k-block behind the matrix's padded K, and an output row behind nout, loads a valid address and is replaced by zeros by SELECT.
//
// Numerics, per row, as the step: bf16 at the LayerNorm outputs, Q' = bf16((q + b_q) log2(e) / sqrt(d_k)), K, V, P, the merged context
// and relu(hid); fp32 sums, biases, residuals and LayerNorm statistics.  Softmax around the row's own EXACT maximum in two sweeps over
// its keys, P_j = bf16(2^(S_j - m)), l = the sum of the unrounded values, ctx = bf16((sum_j P_j V_j) / l).  A blanked row (mask == 0) has
// Q' = 0 by select; its K and V are appended like any other.
//
// Attention.  (row, head) pairs are dealt to the four waves, and a wave runs the step's sweep for its pair: `cl` lanes per key, key
// groups side by side, over the n cached keys in age order and then over the tile's own keys from LDS.  Row i (position t + i) attends
// positions 0 .. t + i; in a ring, max(0, t + i - span + 1) .. t + i, masked per element by select (extend_cached_ok, extend_tile_ok).
// A lane behind a bound loads a valid row and drops it by select.  Pad rows of a partial tile (c < 16) are zeros going in, take no part
// in the attention and are never stored.
//
// Cache discipline.  The tile's own K and V take part from LDS; cached positions < t are only read; nothing written in a launch is
// read back in it.  Plain: rows t .. t + c - 1 are written, pad columns as zeros.  Ring: only the last min(c, span) positions, each to
// pos mod span.  In every layer ALL cache reads (the attention) are behind a barrier before the first write: ring row (t + i) mod span
// holds position t + i - span, which an earlier row of the tile still reads.  Every address derived from device data (the table pair
// and pos[dst]) passes extend_decode first, with its limits taken from the launch arguments.
#pragma once
#include "common.h"
#include "encoder_extend_plan.h"
#include "encoder_step.h"         // EncStepParams, MMT_STEP_KEYS_INFLIGHT
#include "step_common.h"          // step_bf16_round

struct EncExtendParams {
    EncStepParams s;              // x (rows, C, d), mask (rows, C) or null, y (rows, C, d); s.t: the position the call started on (host form);
                                  // s.B: sequences of the state; s.capacity: the capacity, or the span
    ExtendLds lds;
    int C, first, last;           // the call's windows; this launch's first row within the call; the call's last launch?
    int HDKP;
    const int* dst;               // slots form: the table, `rows` pairs
    const int* len;
};

#define MMT_EXTEND_KB_INFLIGHT 8       // weight k-blocks (16 bytes a lane) in flight per output tile

// epi(n, w, acc): features n .. n + 3 (n a multiple of 4, all four below nout) of window w = lane & 15.  W: prepared [KP / 8][nout][8];
// in: bf16 [16][ld], zero behind KP up to the next multiple of 32.  Every thread calls it.
template <typename Epi>
__device__ __forceinline__ void extend_product(const bf16* __restrict__ W, const bf16* in, int ld, int KP, int nout, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = lane & 15, g = lane >> 4;
    const int nkc = KP >> 3, nkb = (nkc + 3) >> 2;
    const bf16x8* wp = reinterpret_cast<const bf16x8*>(W);
    const bf16* brow = in + w * ld + 8 * g;
    for (int n0 = 16 * wave; n0 < nout; n0 += 64) {
        const bool row_ok = n0 + w < nout;
        const int row = row_ok ? n0 + w : 0;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb0 = 0; kb0 < nkb; kb0 += MMT_EXTEND_KB_INFLIGHT) {
            bf16x8 a[MMT_EXTEND_KB_INFLIGHT];
#pragma unroll
            for (int u = 0; u < MMT_EXTEND_KB_INFLIGHT; ++u) {
                const int kc = 4 * (kb0 + u) + g;
                a[u] = wp[(size_t)(kc < nkc ? kc : 0) * nout + row];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < MMT_EXTEND_KB_INFLIGHT; ++u) {
                const int kb = kb0 + u, kc = 4 * kb + g;
                if (kb < nkb) {                                                   // uniform
                    const bf16x8 zero = {};
                    const bf16x8 av = row_ok && kc < nkc ? a[u] : zero;
                    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(brow + 32 * kb);
                    acc = mfma16(av, bv, acc);
                }
            }
        }
        const int n = n0 + 4 * g;
        if (n < nout) epi(n, w, acc);
    }
}

// LayerNorm of the reference (unbiased std, eps added to the std) of the 16 rows of xs: sixteen lanes per row.  put(row, col, value)
template <typename Put>
__device__ __forceinline__ void extend_layernorm(const float* xs, int ld, int d, float eps, const float* a, const float* b, Put put) {
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const float* x = xs + row * ld;
    float s = 0.f;
    for (int c = sub; c < d; c += 16) s += x[c];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)d;
    float q = 0.f;
    for (int c = sub; c < d; c += 16) { const float u = x[c] - mean; q += u * u; }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / (sqrtf(q / (float)(d - 1)) + eps);
    for (int c = sub; c < d; c += 16) put(row, c, a[c] * ((x[c] - mean) * rstd) + b[c]);
}

// SLOTS false: sequence blockIdx.x of the state gets the call's C windows from P.s.t.  SLOTS true: row blockIdx.x of the call goes
// where its table pair says, from pos[dst].  RING: P.s.capacity is the span (step_ring.h).
template <bool SLOTS, bool RING>
__device__ __forceinline__ void encoder_extend_body(const EncExtendParams& P, int* pos, int advance) {
    extern __shared__ __attribute__((aligned(16))) char extend_lds[];
    const EncStepParams& S = P.s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;                                                    // the row of x, mask and y
    const int d = S.d, h = S.h, f = S.f, dk = S.dk, dkp = S.dkp, nchunk = S.nchunk, KPd = S.KPd, KPf = S.KPf, HDKP = P.HDKP;
    const int C = P.C, first = P.first, span = S.capacity;
    const int tile_rows = C - first < MMT_EXTEND_ROWS ? C - first : MMT_EXTEND_ROWS;         // rows of y this launch owns

    // the one decision (encoder_extend_plan.h): uniform, so dst, t and c live in SGPRs
    ExtendRun run;
    if (SLOTS) {
        const int dst = __builtin_amdgcn_readfirstlane(P.dst[r]), len = __builtin_amdgcn_readfirstlane(P.len[r]);
        const int p = dst >= 0 && dst < S.B ? __builtin_amdgcn_readfirstlane(pos[dst]) : MMT_SLOT_IDLE;      // the one read of pos[dst]
        run = extend_decode(dst, len, first, p, C, S.B, span, RING);
    } else {
        run = extend_decode(r, C, first, S.t, C, S.B, span, RING);
    }
    float* y = S.y + ((size_t)r * C + first) * d;
    const int c = run.dst == MMT_EXTEND_SKIP ? 0 : run.c;
    for (int i = c * d + tid; i < tile_rows * d; i += MMT_EXTEND_THREADS) y[i] = 0.f;      // rows behind len, or of a skipped slot: zeros
    if (run.dst == MMT_EXTEND_SKIP) return;                                      // nothing of the state, no pos
    // the call's last launch leaves p + len behind, once every thread's read of pos[dst] is over (a barrier); no other workgroup and
    // no earlier launch of the call reads the new value
    auto leave = [&]() { if (SLOTS && P.last && advance != 0 && tid == 0) pos[run.dst] = run.next; };
    if (c == 0) { __syncthreads(); leave(); return; }
    const int b = run.dst, t = run.t;

    float* xs = reinterpret_cast<float*>(extend_lds + P.lds.xs);
    bf16* nb = reinterpret_cast<bf16*>(extend_lds + P.lds.nb);
    bf16* hb = reinterpret_cast<bf16*>(extend_lds + P.lds.hb);
    bf16* qb = reinterpret_cast<bf16*>(extend_lds + P.lds.q);
    bf16* kb = reinterpret_cast<bf16*>(extend_lds + P.lds.k);
    bf16* vb = reinterpret_cast<bf16*>(extend_lds + P.lds.v);
    const int xs_ld = P.lds.xs_ld, nb_ld = P.lds.nb_ld, hb_ld = P.lds.hb_ld;

    // the cached keys of this tile: n of them, age j in row at(j) (encoder_step.h)
    const int n = RING ? ring_keys(t, span) : t;
    const int r0 = RING ? ring_first_row(t, n, span) : 0;
    auto at = [&](int j) { return RING ? ring_row(r0, j, span) : j; };

    // every byte of the LDS the kernel reads is written here or later: the rows of x (pad rows as zeros), zeros everywhere else
    const float* x = S.x + ((size_t)r * C + first) * d;
    for (int i = tid; i < MMT_EXTEND_ROWS * d; i += MMT_EXTEND_THREADS) {
        const int row = i / d, col = i - row * d;
        xs[row * xs_ld + col] = row < c ? x[i] : 0.f;
    }
    for (int i = tid; i < MMT_EXTEND_ROWS * nb_ld; i += MMT_EXTEND_THREADS) nb[i] = (bf16)0.f;
    for (int i = tid; i < MMT_EXTEND_ROWS * hb_ld; i += MMT_EXTEND_THREADS) hb[i] = (bf16)0.f;
    for (int i = tid; i < MMT_EXTEND_ROWS * HDKP; i += MMT_EXTEND_THREADS) { qb[i] = (bf16)0.f; kb[i] = (bf16)0.f; vb[i] = (bf16)0.f; }
    // window lane & 15 of the product epilogues: blanked?
    const int wl = lane & 15;
    const bool blank = S.mask != nullptr && wl < c && S.mask[(size_t)r * C + first + wl] == 0.f;
    __syncthreads();

    // lane roles of the attention sweeps (encoder_step.h)
    const int cl = nchunk <= 1 ? 1 : nchunk <= 2 ? 2 : nchunk <= 4 ? 4 : 8;     // lanes per key
    const int KG = 64 / cl, kg = lane / cl;
    const bool chunk_ok = lane % cl < nchunk;
    const int ch = chunk_ok ? lane % cl : 0;

    for (int layer = 0; layer < S.N; ++layer) {
        const float* lp = S.params + (size_t)layer * S.pl.layer;
        const bf16* W = S.weights + (size_t)layer * S.w_layer_elems;

        // 1. LayerNorm 1 -> nb
        extend_layernorm(xs, xs_ld, d, S.eps, lp + S.pl.ln1a, lp + S.pl.ln1b, [&](int row, int col, float v) { nb[row * nb_ld + col] = (bf16)v; });
        __syncthreads();

        // 2. Q', K, V of the tile -> LDS
        extend_product(W + S.w_off[0], nb, nb_ld, KPd, 3 * d, [&](int n4, int w, f32x4 acc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int nn = n4 + e;
                const int which = nn / d, col = nn - which * d;
                const int o = w * HDKP + (col / dk) * dkp + col % dk;
                if (which == 0) {
                    const float q = (acc[e] + lp[S.pl.bq + col]) * S.qscale;
                    qb[o] = blank ? (bf16)0.f : (bf16)q;
                } else if (which == 1) {
                    kb[o] = (bf16)(acc[e] + lp[S.pl.bk + col]);
                } else {
                    vb[o] = (bf16)(acc[e] + lp[S.pl.bv + col]);
                }
            }
        });
        __syncthreads();

        // 3. attention: (row, head) pairs dealt to the waves; the n cached keys in age order, then the tile's own from LDS
        bf16* Kc = S.cache + (size_t)layer * S.cache_layer + (size_t)b * S.cache_seq;
        bf16* Vc = Kc + S.cache_kv;
        for (int task = wave; task < c * h; task += 4) {
            const int head = task / c, i = task - head * c;
            const bf16* Kh = Kc + (size_t)head * S.cache_head;
            const bf16* Vh = Vc + (size_t)head * S.cache_head;
            const bf16* kt = kb + head * dkp + 8 * ch;                           // + u * HDKP: chunk ch of the tile's key u
            const bf16* vt = vb + head * dkp + 8 * ch;
            float q[8];
            {
                const bf16x8 q8 = *reinterpret_cast<const bf16x8*>(qb + i * HDKP + head * dkp + 8 * ch);
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = chunk_ok ? (float)q8[e] : 0.f;
            }
            auto score = [&](const bf16x8& k8) {
                float part = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) part = fmaf(q[e], (float)k8[e], part);
                part = chunk_ok ? part : 0.f;
                for (int o = 1; o < cl; o <<= 1) part += __shfl_xor(part, o);
                return part;
            };
            // first sweep: the row's exact maximum.  Loads are unconditional (a lane behind a bound reads age 0 / key 0), dropped by select
            float m = -INFINITY;
            for (int j0 = 0; j0 < n; j0 += MMT_STEP_KEYS_INFLIGHT * KG) {
                bf16x8 kk[MMT_STEP_KEYS_INFLIGHT];
#pragma unroll
                for (int u = 0; u < MMT_STEP_KEYS_INFLIGHT; ++u) {
                    const int j = j0 + u * KG + kg;
                    kk[u] = *reinterpret_cast<const bf16x8*>(Kh + (size_t)at(j < n ? j : 0) * dkp + 8 * ch);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < MMT_STEP_KEYS_INFLIGHT; ++u) {
                    const int j = j0 + u * KG + kg;
                    const bool valid = j < n && extend_cached_ok(i, j, n, span, RING);
                    const float part = score(kk[u]);
                    m = valid ? fmaxf(m, part) : m;
                }
            }
            for (int u0 = 0; u0 < MMT_EXTEND_ROWS; u0 += KG) {
                const int u = u0 + kg;
                const bool valid = u < MMT_EXTEND_ROWS && extend_tile_ok(i, u, span, RING);
                const float part = score(*reinterpret_cast<const bf16x8*>(kt + (u < MMT_EXTEND_ROWS ? u : 0) * HDKP));
                m = valid ? fmaxf(m, part) : m;
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
                    const size_t row = (size_t)at(j < n ? j : 0) * dkp + 8 * ch;
                    kk[u] = *reinterpret_cast<const bf16x8*>(Kh + row);
                    v8[u] = *reinterpret_cast<const bf16x8*>(Vh + row);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < MMT_STEP_KEYS_INFLIGHT; ++u) {
                    const int j = j0 + u * KG + kg;
                    const bool valid = j < n && extend_cached_ok(i, j, n, span, RING);
                    const float part = score(kk[u]);
                    const float p = valid ? fast_exp2(part - m) : 0.f;           // selects: nothing behind a bound is ever multiplied
                    const float pb = step_bf16_round(p);
                    l += p;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = fmaf(pb, valid && chunk_ok ? (float)v8[u][e] : 0.f, acc[e]);
                }
            }
            for (int u0 = 0; u0 < MMT_EXTEND_ROWS; u0 += KG) {
                const int u = u0 + kg, uc = u < MMT_EXTEND_ROWS ? u : 0;
                const bool valid = u < MMT_EXTEND_ROWS && extend_tile_ok(i, u, span, RING);
                const float part = score(*reinterpret_cast<const bf16x8*>(kt + uc * HDKP));
                const bf16x8 v8 = *reinterpret_cast<const bf16x8*>(vt + uc * HDKP);
                const float p = valid ? fast_exp2(part - m) : 0.f;
                const float pb = step_bf16_round(p);
                l += p;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pb, valid && chunk_ok ? (float)v8[e] : 0.f, acc[e]);
            }
            for (int o = cl; o < 64; o <<= 1) {
                l += __shfl_xor(l, o);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], o);
            }
            if (kg == 0 && chunk_ok) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (8 * ch + e < dk) nb[i * nb_ld + head * dk + 8 * ch + e] = (bf16)(acc[e] / l);          // the merged context
            }
        }
        // pad rows of a partial tile take no part in the attention: their context is zeros
        for (int i = c * d + tid; i < MMT_EXTEND_ROWS * d; i += MMT_EXTEND_THREADS) nb[(i / d) * nb_ld + i % d] = (bf16)0.f;
        __syncthreads();                                                         // every cache read of this layer is over

        // 4. append K, V of the tile's rows [w0, c): 16 bytes per store, pad columns are the zeros the LDS rows hold
        {
            const int w0 = extend_first_written(c, span, RING);
            const int per = h * nchunk, items = 2 * (c - w0) * per;
            for (int it = tid; it < items; it += MMT_EXTEND_THREADS) {
                const int kv = it / ((c - w0) * per), r1 = it - kv * ((c - w0) * per);
                const int i = w0 + r1 / per, r2 = r1 % per, head = r2 / nchunk, cc = r2 - head * nchunk;
                const bf16x8 v = *reinterpret_cast<const bf16x8*>((kv ? vb : kb) + i * HDKP + head * dkp + 8 * cc);
                const int row = prefill_row(t + i, span, RING);
                *reinterpret_cast<bf16x8*>((kv ? Vc : Kc) + (size_t)head * S.cache_head + (size_t)row * dkp + 8 * cc) = v;
            }
        }

        // 5. output projection + residual
        extend_product(W + S.w_off[1], nb, nb_ld, KPd, d, [&](int n4, int w, f32x4 acc) {
            f32x4* px = reinterpret_cast<f32x4*>(xs + w * xs_ld + n4);
            f32x4 v = *px;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += acc[e] + lp[S.pl.bo + n4 + e];
            *px = v;
        });
        __syncthreads();

        // 6. LayerNorm 2 -> nb
        extend_layernorm(xs, xs_ld, d, S.eps, lp + S.pl.ln2a, lp + S.pl.ln2b, [&](int row, int col, float v) { nb[row * nb_ld + col] = (bf16)v; });
        __syncthreads();

        // 7. FFN + residual
        extend_product(W + S.w_off[2], nb, nb_ld, KPd, f, [&](int n4, int w, f32x4 acc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) hb[w * hb_ld + n4 + e] = (bf16)fmaxf(acc[e] + lp[S.pl.b1 + n4 + e], 0.f);
        });
        __syncthreads();
        extend_product(W + S.w_off[3], hb, hb_ld, KPf, d, [&](int n4, int w, f32x4 acc) {
            f32x4* px = reinterpret_cast<f32x4*>(xs + w * xs_ld + n4);
            f32x4 v = *px;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += acc[e] + lp[S.pl.b2 + n4 + e];
            *px = v;
        });
        __syncthreads();
    }

    extend_layernorm(xs, xs_ld, d, S.eps, S.params + S.pl.final_a, S.params + S.pl.final_b,
                     [&](int row, int col, float v) { if (row < c) y[(size_t)row * d + col] = v; });
    leave();                                                                     // behind the barriers of the layers
}

__global__ __launch_bounds__(MMT_EXTEND_THREADS) void encoder_extend_kernel(const EncExtendParams P) { encoder_extend_body<false, false>(P, nullptr, 0); }

__global__ __launch_bounds__(MMT_EXTEND_THREADS) void encoder_extend_slots_kernel(const EncExtendParams P, int* pos, int advance) {
    encoder_extend_body<true, false>(P, pos, advance);
}

// The ring forms (step_ring.h): P.s.capacity is the span, the cache has that many rows, and no position below INT_MAX is refused.
__global__ __launch_bounds__(MMT_EXTEND_THREADS) void encoder_extend_ring_kernel(const EncExtendParams P) { encoder_extend_body<false, true>(P, nullptr, 0); }

__global__ __launch_bounds__(MMT_EXTEND_THREADS) void encoder_extend_ring_slots_kernel(const EncExtendParams P, int* pos, int advance) {
    encoder_extend_body<true, true>(P, pos, advance);
}
