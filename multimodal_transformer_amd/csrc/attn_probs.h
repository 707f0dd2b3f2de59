// The attention probabilities of every head, materialised on request: P (B,h,T,T) fp32, the post-dropout p_attn the reference
// keeps on the module (transformer/MFT/multiTransformer.py:22-34, self.attn at :59).  A diagnostic beside the attention core, not part
// of it: attn.h never forms a (T x T) tensor and is not touched by this file.
//
// Arithmetic is that of attn.h's forward, so the map is the one the model used: Q' = bf16(q * log2(e)/sqrt(d_k)) (0 for a blanked
// query row, which then soft-maxes to exactly 1/T over all T keys), K = bf16(k), scores on bf16 MFMA with fp32 accumulation in the
// log2 domain, P = 2^(S' - rowmax) * (1 / rowsum) in fp32.  Train mode stores 0 for a dropped element and P / (1 - p) for a kept one,
// normalised by the UNDROPPED row sum; the keep decisions are attn_mask.h's (attn_keep_block of the same (seed, batch*head, tile
// pair)), i.e. bit for bit those mmt_sdpa_forward applies for the same seed.
//
// Shape of the work.  The kernel is bound by its B*h*T^2*4 bytes of stores; the scores are cheap.  Wave w of a workgroup owns query
// tile 4 bx + w of one (batch, head) and sweeps the key tiles twice: sweep 1 keeps a running (max, sum) per LANE and query (a lane sees
// keys r, r + 32, ... of its 16 queries), merged across the 32 lanes of a half once, after the sweep; sweep 2 recomputes the scores
// (same instructions, same operands: bit-identical) and stores.  Nothing T-wide stays in registers or LDS.  The product is oriented
// S = Q' K^T — the KEY on the accumulator's lane column, not attn.h's S^T — so that one store instruction writes two contiguous
// 128-byte runs (one query row per 32-lane half).  Rows are T floats apart and T is usually no multiple of 4: dword stores.
// q and k are read as fp32 straight from the caller's (B,T,d) tensors (head i in columns [i d_k, (i+1) d_k)), 8 consecutive features
// per lane and k-step, and rounded in registers; features >= d_k are zeros (d_k padded to 16/32/64 like the core's fragments).
// The waves of a workgroup share nothing: no LDS staging, no barrier, no inter-workgroup communication, no atomics.
//
// Dropout.  The generator's unit is one lane drawing one 32x32 block (attn_keep_block: W[key] bit query).  At the first tile of every
// 64 key tiles the wave's lanes draw the 64 blocks (q tile, kt0 + lane) and park them in a wave-private LDS patch (33-word rows:
// conflict-free); tile kt then takes word `key r` of block kt - kt0 and lane_word() picks the 16 queries of the lane's half in
// accumulator order — the LK orientation of attn_mask.h.  Every block is drawn exactly once.
//
// Key lengths (attn_probs_keys_kernel; attn.h): both sweeps end after the ceil(len/32) key tiles of the sequence, keys >= len score
// MASKED like keys >= T, and — the output buffer is uninitialised — the columns behind the length are written as exact zeros.
//
// Causal (attn_probs_causal_kernel; attn.h): both sweeps of query tile qt end at key tile qt, where key > query scores MASKED too, and
// the tiles above the diagonal are written as exact zeros.  The diagonal is a select on a wave-uniform flag inside the one tile
// body, still straight-line code: a second instantiation of the body, as attn.h has, doubles the keep-bit generator and brings the
// d_k = 64 train instance to 256 VGPRs with scratch.
//
// Band (attn_probs_band_kernel; attn.h): both sweeps of query tile qt run key tiles band_lo_tile(qt) .. qt, a key outside query-span+1 ..
// query scores MASKED — one select in the one tile body, on every tile of the sweep (the kernel is bound by its stores) — and the
// tiles on BOTH sides of the band are written as exact zeros.  A (lane, query) pair whose first tiles hold no visible key carries
// m = MASKED, which is finite: the first visible score wipes what it had summed (2^(MASKED - s) == 0), and one that never sees a key
// weighs 0 in the merge.  The keep bits of a sweep that starts in the middle of a 64-tile group are drawn at its first tile.
#pragma once
#include "common.h"
#include "attn_mask.h"
#include "attn.h"          // attn_block / attn_grid: the (tile quad, batch*head) decoding of the 1-D grid

#define MMT_PROBS_MASKED (-1.0e30f)        // score of a key >= T: finite (no inf - inf in the running rescale), 2^(it - any real max) == 0
#define MMT_PROBS_PATCH_ROW 33             // uint32 words per parked block

// features e0 .. e0+7 of one window's head slice -> bf16 fragment, scaled by sc before rounding; features >= dk read as 0.
// vec: the slice is 16-byte aligned and dk a multiple of 4, so each group of four is all inside or all outside.
__device__ __forceinline__ bf16x8 probs_frag(const float* __restrict__ row, int e0, int dk, float sc, bool vec) {
    float v[8];
    if (vec) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
            if (e0 + 4 * g < dk) t = *reinterpret_cast<const f32x4*>(row + e0 + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * g + j] = t[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (e0 + j < dk) ? row[e0 + j] : 0.f;
    }
    bf16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (bf16)(v[j] * sc);
    return out;
}

template <int DKP, bool DROP, int MODE>
__device__ __forceinline__ void attn_probs_body(
        const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ rowmask, float* __restrict__ P,
        int h, int T, int nt, int nbh, int d, int dk, float qscale, int vec, DropCfg drop, const int* __restrict__ key_lengths, int span) {
    constexpr bool KEYS = MODE == ATTN_KEYS, CAUSAL = MODE == ATTN_CAUSAL, BAND = MODE == ATTN_BAND;
    constexpr int KS = DKP / 16;
    __shared__ uint32_t patch[DROP ? 4 * 64 * MMT_PROBS_PATCH_ROW : 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const AttnBlock ab = attn_block((nt + 3) >> 2, nbh);
    if (!ab.valid) return;
    const int qt = ab.bx * 4 + wave;
    if (qt >= nt) return;                               // waves share nothing: no barrier below
    const int bh = ab.bh, b = bh / h, head = bh - b * h;
    const int Tk = KEYS ? attn_key_len(key_lengths, b, T) : T;          // keys that exist for this sequence, and their tiles
    const int nk = KEYS ? (Tk + 31) >> 5 : (CAUSAL || BAND) ? qt + 1 : nt;       // causal: up to the diagonal tile
    const int sp = BAND ? min(span, T) : 0;
    const int k0 = BAND ? band_lo_tile(qt, sp) : 0;                    // band: from the tile of the first query's first key

    // A operand: Q' of query r of the tile (a query >= T reads row T-1 and is never stored), features 16 s + 8 hh .. + 7
    bf16x8 qf[KS];
    {
        const int tq = min(qt * 32 + r, T - 1);
        const size_t mq = (size_t)b * T + tq;
        const float sc = (rowmask && rowmask[mq] == 0.0f) ? 0.f : qscale;        // blanked query row: Q' = 0
        const float* qrow = q + mq * d + head * dk;
#pragma unroll
        for (int s = 0; s < KS; ++s) qf[s] = probs_frag(qrow, 16 * s + 8 * hh, dk, sc, vec);
    }
    // B operand: K of key r of tile kt (a key >= T reads row T-1; its score is overwritten)
    const float* kbase = k + (size_t)b * T * d + head * dk;
    auto kfrag = [&](int kt, bf16x8 (&kf)[KS]) {
        const float* krow = kbase + (size_t)min(kt * 32 + r, T - 1) * d;
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[s] = probs_frag(krow, 16 * s + 8 * hh, dk, 1.f, vec);
    };
    // S' tile: register i = query acc32_row(i, hh), lane column = key r.  Straight-line code from the MFMA to the consumers of its result.
    auto scores = [&](const bf16x8 (&kf)[KS], int kt) {
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int ss = 0; ss < KS; ++ss) s = mfma32(qf[ss], kf[ss], s);
        const bool kok = kt * 32 + r < Tk;
        if constexpr (BAND) {                           // key r of the tile is visible to the queries key .. key + span - 1
            const int rel = (qt - kt) * 32 - r;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = (kok && (unsigned)(rel + acc32_row(i, hh)) < (unsigned)sp) ? s[i] : MMT_PROBS_MASKED;
        } else if constexpr (CAUSAL) {                  // on the diagonal tile key r is visible to the queries >= r only
            const bool diag = kt == qt;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = (kok && (!diag || r <= acc32_row(i, hh))) ? s[i] : MMT_PROBS_MASKED;
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = kok ? s[i] : MMT_PROBS_MASKED;
        }
        return s;
    };

    // ---- sweep 1: running max and sum per (lane, query)
    float m[16], l[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { m[i] = MMT_PROBS_MASKED; l[i] = 0.f; }
    bf16x8 kf[KS], kn[KS];
    kfrag(k0, kf);
    for (int kt = k0; kt < nk; ++kt) {
        kfrag(min(kt + 1, nk - 1), kn);                 // next tile in flight behind this tile's arithmetic (the last one re-reads itself)
        const f32x16 s = scores(kf, kt);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float mn = fmaxf(m[i], s[i]);
            l[i] = l[i] * fast_exp2(m[i] - mn) + fast_exp2(s[i] - mn);
            m[i] = mn;
        }
#pragma unroll
        for (int s2 = 0; s2 < KS; ++s2) kf[s2] = kn[s2];
    }
    // merge the 32 lanes of a half: m <- row max, l <- (1/(1-p)) / row sum.  A lane that saw only keys >= T carries m = MASKED and
    // weighs 2^(MASKED - max) = 0; every row has >= 1 real key, so the max is finite.  (Band: a query row >= T of the last tile sees no
    // key at all when span is small; its max is MASKED, which is finite too, its weights are 2^0, and the row is never stored.)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float mx = m[i];
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float li = l[i] * fast_exp2(m[i] - mx);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) li += __shfl_xor(li, o);
        m[i] = mx;
        l[i] = (DROP ? drop.scale : 1.0f) / li;
    }

    // ---- sweep 2: recompute, normalise, drop, store
    DropCfg dc = drop;
    if (DROP) dc = drop_substream(drop, (uint32_t)bh);
    uint32_t* const mine = patch + (DROP ? wave * 64 * MMT_PROBS_PATCH_ROW : 0);
    float* const prow = P + ((size_t)bh * T + (size_t)qt * 32) * T;       // row `query in tile` at + query * T
    const bool qfull = qt * 32 + 32 <= T;
    if (BAND) {                                         // the key tiles below the band: zeros
        for (int kt = 0; kt < k0; ++kt) {
            float* const pk = prow + kt * 32 + r;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (qt * 32 + acc32_row(i, hh) < T) pk[(size_t)acc32_row(i, hh) * T] = 0.f;
        }
    }
    kfrag(k0, kf);
    for (int kt = k0; kt < nk; ++kt) {
        const int kb = BAND ? kt & ~63 : kt;            // first tile of the 64 whose blocks the patch holds
        if (DROP && (BAND ? (kt == kb || kt == k0) : (kt & 63) == 0)) {       // wave-uniform: the keep bits of blocks (qt, kb + lane), one block per lane
            uint32_t W[32];
            attn_keep_block(dc, (uint32_t)(qt * nt + min(kb + lane, nt - 1)), W);      // W[key] bit query
#pragma unroll
            for (int key = 0; key < 32; ++key) mine[lane * MMT_PROBS_PATCH_ROW + key] = W[key];
        }
        kfrag(min(kt + 1, nk - 1), kn);
        f32x16 s = scores(kf, kt);
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = fast_exp2(s[i] - m[i]) * l[i];
        if (DROP) {     // (same wave wrote and reads the patch: program order is enough, no barrier)
            const uint32_t lw = lane_word(mine[(kt & 63) * MMT_PROBS_PATCH_ROW + r], hh);     // bit i: (query acc32_row(i, hh), key r)
            static_for<0, 16>([&](auto ic) { constexpr int i = decltype(ic)::value; s[i] = keep_and<i>(s[i], lw); });
        }
        float* const pk = prow + kt * 32 + r;
        if (qfull && kt * 32 + 32 <= T) {               // wave-uniform: a full tile stores unguarded
#pragma unroll
            for (int i = 0; i < 16; ++i) pk[(size_t)acc32_row(i, hh) * T] = s[i];
        } else {                                        // the last tile of either axis: no element outside (T x T) is written
            const bool kok = kt * 32 + r < T;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (kok && qt * 32 + acc32_row(i, hh) < T) pk[(size_t)acc32_row(i, hh) * T] = s[i];
        }
#pragma unroll
        for (int s2 = 0; s2 < KS; ++s2) kf[s2] = kn[s2];
    }
    if (KEYS || CAUSAL || BAND) {     // the key tiles behind the length / above the diagonal: zeros (the boundary tile's masked entries were stored above, as 2^(MASKED - max) == 0)
        for (int kt = nk; kt < nt; ++kt) {
            float* const pk = prow + kt * 32 + r;
            const bool kok = kt * 32 + r < T;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (kok && qt * 32 + acc32_row(i, hh) < T) pk[(size_t)acc32_row(i, hh) * T] = 0.f;
        }
    }
}
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_probs_kernel(
        const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ rowmask, float* __restrict__ P,
        int h, int T, int nt, int nbh, int d, int dk, float qscale, int vec, DropCfg drop) {
    attn_probs_body<DKP, DROP, ATTN_PLAIN>(q, k, rowmask, P, h, T, nt, nbh, d, dk, qscale, vec, drop, nullptr, 0);
}
// ... with key lengths: columns >= key_lengths[b] are exact zeros
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_probs_keys_kernel(
        const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ rowmask, float* __restrict__ P,
        int h, int T, int nt, int nbh, int d, int dk, float qscale, int vec, DropCfg drop, const int* __restrict__ key_lengths) {
    attn_probs_body<DKP, DROP, ATTN_KEYS>(q, k, rowmask, P, h, T, nt, nbh, d, dk, qscale, vec, drop, key_lengths, 0);
}
// ... causal: entries above the diagonal are exact zeros
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_probs_causal_kernel(
        const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ rowmask, float* __restrict__ P,
        int h, int T, int nt, int nbh, int d, int dk, float qscale, int vec, DropCfg drop) {
    attn_probs_body<DKP, DROP, ATTN_CAUSAL>(q, k, rowmask, P, h, T, nt, nbh, d, dk, qscale, vec, drop, nullptr, 0);
}
// ... band: entries outside keys query-span+1 .. query are exact zeros
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_probs_band_kernel(
        const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ rowmask, float* __restrict__ P,
        int h, int T, int nt, int nbh, int d, int dk, float qscale, int vec, DropCfg drop, int span) {
    attn_probs_body<DKP, DROP, ATTN_BAND>(q, k, rowmask, P, h, T, nt, nbh, d, dk, qscale, vec, drop, nullptr, span);
}
