// Dropout on the attention probabilities (transformer/MFT/multiTransformer.py:32-33) as a stored BIT MASK.
//
// Round 1 evaluated a counter hash per score inside every attention kernel, forward and backward: 13 cycles of SIMD issue per
// hash word plus 6 per decision for the compare-and-select, 40 % of the forward's and a third of the backward's instruction
// stream (tools/valu_micro.hip prices the instructions).  Now one generator launch per forward pass draws every decision of
// every layer once, 32 decisions per instruction, and stores them in the order the consumers hold their scores: a consumer lane
// loads ONE 16-bit word per 32x32 score tile (a tile ahead, with the tile's operand prefetch) and turns bit i into an all-ones /
// zero word with v_bfe_i32, which it ANDs onto accumulator register i: two full-rate instructions per register, no compare, no
// hash, no scalar registers.  (A first version kept the masks as 64-bit lane masks in SGPRs, loaded with s_load_dwordx16 and
// applied with one v_cndmask_b32 per register: fewer vector instructions, but scalar loads share the LDS wait counter, so every
// tile's first LDS wait exposed the whole scalar-load latency: +5 us per forward launch over eval mode instead of +1.  The plain
// d_k = 16 forward has that form again — see "Lane-mask form" below — with the loads placed where no LDS wait follows them until the
// masks are needed.)
//
// Bernoulli words.  A 32-bit word whose bits are independent drops with probability thr16 / 65536 is built from up to 16
// uniform random words, least significant threshold bit first:  D = bit_b ? (D | R_b) : (D & R_b)   (each step halves the
// distance to the target probability).  Threshold bits below the lowest set one leave D = 0 and are skipped (p = 0.1:
// thr16 = 0x199A, 15 words; p = 0.25: 2 words).  R_b = drop_fin(drop_lin(...)) — the counter hash of common.h — of the word
// index ((q tile * nt + k tile) * 32 + key) * 16 + b inside the per-(batch, head) substream, so a mask is still a pure
// function of (seed, layer stream, batch*head, query, key) and mmt_debug_dropout_mask replays it.
//
// Layouts (uint16 words; nt = Tp / 32 tiles per axis).  One generator lane owns one 32x32 block and writes it twice, 128 bytes each:
//   LQ [bh][q tile][k tile][64 lanes]: for kernels that keep the QUERY on the lane (forward, dQ): lane l = 32 hh + q holds, in bit i,
//      the decision for (query q, key (i&3) + 8(i>>2) + 4hh) — accumulator register i of that lane;
//   LK [bh][k tile][q tile][64 lanes]: for kernels that keep the KEY on the lane (dK/dV, the one-kernel backward): lane 32 hh + key,
//      bit j = (query (j&3) + 8(j>>2) + 4hh, key).
// LQ needs the block transposed (bits over keys): a 32x32 bit transpose in registers (5 butterfly stages), 64 blocks per wave.
//
// Lane-mask form of LQ (MaskGenLayer::lanes, chosen by the host per layer with the kernel that reads it; same array, same 128 bytes
// per block, same block order, so a launch writes one form or the other):
//   sixteen 64-bit words per block, word i = the wave's lane mask of accumulator register i: bit r + 32 hh = the decision for
//   (query r, key (i&3) + 8(i>>2) + 4hh).  That is the key-major bit matrix W with its rows in register order — dword 2i + hh =
//   W[acc32_row(i, hh)] — so this form needs no transpose and no lane_word.  Its reader (attn.h, the plain d_k = 16 forward) fetches the
//   128 bytes with wave-uniform scalar loads and applies word i to register i with ONE v_cndmask_b32 (4.2 cycles of SIMD issue where
//   v_bfe_i32 + v_and_b32 take 6.5: profiles/r10_valu_micro.txt).  LK keeps its form: every backward kernel reads the 16-bit words.
#pragma once
#include "common.h"

#define MMT_MASK_BLOCK_WORDS 32

// keep bits of one 32x32 block: W[key] bit q = 1 iff (query q, key) of the block is kept.  CHAINS: independent hash chains in flight
// (keys drawn together); every W[key] is its own function of (dc, blk, key), so the bits do not depend on it.
template <int CHAINS = 32>
__device__ __forceinline__ void attn_keep_block(const DropCfg& dc, uint32_t blk, uint32_t (&W)[32]) {
    static_assert(CHAINS > 0 && 32 % CHAINS == 0, "the keys of a block are drawn in equal groups");
    const uint32_t thr = dc.thr16;
    const int b0 = thr ? __builtin_ctz(thr) : 16;                 // wave-uniform
    // threshold bit outermost (a uniform, rolled loop), the 32 keys unrolled inside: 32 independent hash chains in flight (124 VGPRs,
    // 4 waves per SIMD).  16 or 8 chains at 6 or 8 waves per SIMD (all 6144 waves of configs[3] resident at once) measured the same
    // 58-60 us: the kernel is bound by the total integer instruction issue, not by latency, occupancy or its tail.
    // (CHAINS < 32: the rolled loop runs once per group of CHAINS keys, on the group's own words D — the form that fits beside a row
    // chain's 80 VGPRs, rowgemm.h.  Updating a part of W in a loop instead makes hipcc 7.2 carry W as one 32-register tuple and copy
    // it every trip.)
    const uint32_t x0 = drop_lin(dc.s0, blk * 512u) + (uint32_t)b0 * MMT_DROP_C1;   // word index blk*512 + key*16 + b  (< 2^24 for Tp <= 4096)
#pragma unroll
    for (int k0 = 0; k0 < 32; k0 += CHAINS) {
        uint32_t D[CHAINS];                                       // the drop words; threshold bits below b0 leave them 0
#pragma unroll
        for (int i = 0; i < CHAINS; ++i) D[i] = 0;
        uint32_t x = x0;
#pragma unroll 1
        for (int b = b0; b < 16; ++b) {
            if ((thr >> b) & 1u) {
#pragma unroll
                for (int i = 0; i < CHAINS; ++i) D[i] |= drop_fin(x + (uint32_t)(16 * (k0 + i)) * MMT_DROP_C1, dc.s1);
            } else {
#pragma unroll
                for (int i = 0; i < CHAINS; ++i) D[i] &= drop_fin(x + (uint32_t)(16 * (k0 + i)) * MMT_DROP_C1, dc.s1);
            }
            x += MMT_DROP_C1;
        }
#pragma unroll
        for (int i = 0; i < CHAINS; ++i) W[k0 + i] = ~D[i];
    }
}

// in-register transpose of a 32x32 bit matrix: on return A[i] bit j = old A[j] bit i
__device__ __forceinline__ void transpose32(uint32_t (&A)[32]) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int j = 16 >> s;
        const uint32_t m = (s == 0) ? 0x0000FFFFu : (s == 1) ? 0x00FF00FFu : (s == 2) ? 0x0F0F0F0Fu : (s == 3) ? 0x33333333u : 0x55555555u;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            if (k & j) continue;
            // rows k and k+j exchange the off-diagonal j x j bit blocks
            const uint32_t t = ((A[k] >> j) ^ A[k + j]) & m;
            A[k + j] ^= t;
            A[k] ^= t << j;
        }
    }
}

// the 16 bits a consumer lane of half hh needs out of a 32-bit row: bit i of the result = bit (i&3) + 8(i>>2) + 4hh of x
// (the even / odd nibbles of x, packed)
__device__ __forceinline__ uint32_t lane_word(uint32_t x, int hh) {
    uint32_t y = (x >> (4 * hh)) & 0x0F0F0F0Fu;
    y = (y | (y >> 4)) & 0x00FF00FFu;
    return (y | (y >> 8)) & 0x0000FFFFu;
}

struct MaskGenParams {
    uint16_t* lq; uint16_t* lk;            // layer l at + l * layer_words
    size_t layer_words;
    int nbh, nt, nlayers;
    int lanes;                             // LQ in the lane-mask form (every layer of a launch has the same consumers)
    uint32_t thr16;
    uint32_t s0[16], s1[16];               // stream keys of the layers' attention dropout (make_drop(p, seed, 4l+0))
    const uint64_t* seedword;              // non-null: device-resident seed (common.h drop_resolve); s0[l] then holds the stream id 4l+0
};
// what the generator needs of ONE layer: its two arrays and its stream keys (seedword non-null: s0 is the stream id, as above)
struct MaskGenLayer {
    uint16_t* lq; uint16_t* lk;
    int nbh, nt;
    int lanes;                             // LQ in the lane-mask form
    uint32_t thr16, s0, s1;
    const uint64_t* seedword;
};
__device__ __forceinline__ MaskGenLayer mask_gen_layer(const MaskGenParams& P, int layer) {
    MaskGenLayer G;
    G.lq = P.lq + (size_t)layer * P.layer_words; G.lk = P.lk + (size_t)layer * P.layer_words;
    G.nbh = P.nbh; G.nt = P.nt; G.lanes = P.lanes; G.thr16 = P.thr16; G.s0 = P.s0[layer]; G.s1 = P.s1[layer]; G.seedword = P.seedword;
    return G;
}

// rows[x] = 32 bits over the lane index (x = the register-side index): the 64 lane words of one block, 8 x 16 bytes, into this lane's
// row of the wave's LDS patch
#define MMT_MASK_LDS_ROW 72            // uint16 per patch row: 64 + 8 pad (144-byte rows: conflict-free 16-byte writes)
__device__ __forceinline__ void park_lane_block(uint16_t* row, const uint32_t (&rows)[32]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {          // piece c: lanes 8c .. 8c+7, i.e. half hh = c >> 2, lane-side index 8(c&3) .. +7
        u32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int l0 = 8 * (c & 3) + 2 * e, hh = c >> 2;
            v[e] = lane_word(rows[l0], hh) | (lane_word(rows[l0 + 1], hh) << 16);
        }
        *reinterpret_cast<u32x4_t*>(row + 8 * c) = v;
    }
}

// the lane-mask form of one block into this lane's patch row: piece c = words 2c and 2c+1, i.e. W[acc32_row(i, hh)] for i = 2c, 2c+1
__device__ __forceinline__ void park_lane_masks(uint16_t* row, const uint32_t (&W)[32]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        u32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 2 * c + (e >> 1), hh = e & 1;
            v[e] = W[(i & 3) + 8 * (i >> 2) + 4 * hh];
        }
        *reinterpret_cast<u32x4_t*>(row + 8 * c) = v;
    }
}

// One lane per 32x32 block; the lanes of a wave own 64 consecutive blocks in (bh, q tile, k tile) order.  A block is 128 bytes per
// orientation, so lane-private stores would be 64 separate 16-byte writes per instruction (6.5 M partial-line transactions per launch
// at configs[3]).  The wave parks its 64 blocks in LDS and writes them out with the lanes laid along memory (no change in the
// kernel's own time — it is bound by integer issue — but whole lines reach the fabric): LQ blocks of a wave are contiguous (1 KB per store instruction), LK blocks are
// written as whole 128-byte lines by 8 lanes each.
// `patch`: the workgroup's LDS patches, MMT_MASK_PATCH_WORDS per generator wave (the caller's own static or dynamic LDS); `first`:
// the workgroup's first block; waves >= gen_waves of the workgroup take no part.  CHAINS: attn_keep_block.
#define MMT_MASK_PATCH_WORDS (64 * MMT_MASK_LDS_ROW)
#define MMT_MASK_GEN_WAVES 4           // generator waves per workgroup of the two stand-alone kernels
template <int CHAINS = 32>
__device__ __forceinline__ void attn_mask_gen_block(const MaskGenLayer& P, uint16_t* patch, size_t first, int gen_waves) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (scalar: so is all that follows from it)
    if (wave >= gen_waves) return;
    patch += wave * MMT_MASK_PATCH_WORDS;
    const size_t g0 = first + wave * 64;                                    // first block of the wave
    const size_t per_bh = (size_t)P.nt * P.nt, total = (size_t)P.nbh * per_bh;
    if (g0 >= total) return;                                                // whole wave (no workgroup barrier below)
    const size_t g = g0 + lane;
    const bool live = g < total;
    const size_t gc = live ? g : total - 1;
    const int bh = (int)(gc / per_bh);
    const int rem = (int)(gc - (size_t)bh * per_bh), qt = rem / P.nt, kt = rem - qt * P.nt;
    DropCfg base; base.thr16 = P.thr16; base.scale = 1.f; base.s0 = P.s0; base.s1 = P.s1;
    const DropCfg dc = drop_substream(drop_resolve(base, P.seedword), (uint32_t)bh);
    uint32_t W[32];
    attn_keep_block<CHAINS>(dc, (uint32_t)(qt * P.nt + kt), W);            // W[key] bit query
    uint16_t* const mine = patch + lane * MMT_MASK_LDS_ROW;
    // flush role: in store instruction i this lane moves piece (lane & 7) of the wave's block 8 i + (lane >> 3)
    const int fp = lane & 7;
    const uint16_t* from;
    // (formed after the park, from a lane index the compiler cannot see through: formed above, the address is live across the draw and
    // the park, where the 80-VGPR form has no register for it)
    auto flush_from = [&] { int l = lane; asm volatile("" : "+v"(l)); return patch + (l >> 3) * MMT_MASK_LDS_ROW + 8 * (l & 7); };
    // ---- LK: key on the lane: lane-side index = key, its row = W[key] (bits over the queries = the register side)
    park_lane_block(mine, W);
    from = flush_from();
    {
        // (bh, q tile, k tile) of block lane >> 3 — its owner lane has them — then + 8 blocks per instruction
        size_t gb = g0 + (lane >> 3);
        int bb = __shfl(bh, lane >> 3), qb = __shfl(qt, lane >> 3), kb = __shfl(kt, lane >> 3);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(from + 8 * i * MMT_MASK_LDS_ROW);
            if (gb < total) *reinterpret_cast<u32x4_t*>(P.lk + ((size_t)bb * per_bh + (size_t)kb * P.nt + qb) * 64 + 8 * fp) = v;
            gb += 8; kb += 8;
            while (kb >= P.nt) { kb -= P.nt; if (++qb == P.nt) { qb = 0; ++bb; } }
        }
    }
    // ---- LQ: block index == g: the wave's 64 blocks are contiguous in memory
    // (same wave wrote and read the patch: program order is enough, no barrier)
    if (P.lanes) park_lane_masks(mine, W);                                 // wave-uniform: a kernel argument
    else {
        transpose32(W);                                                    // W[query] bit key
        park_lane_block(mine, W);
    }
    from = flush_from();
    {
        uint16_t* const lq = P.lq + g0 * 64;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(from + 8 * i * MMT_MASK_LDS_ROW);
            if (g0 + 8 * i + (lane >> 3) < total) *reinterpret_cast<u32x4_t*>(lq + (size_t)i * 512 + lane * 8) = v;
        }
    }
}

// grid = (blocks of 256, layers)
__global__ __launch_bounds__(256, 4) void attn_mask_gen_kernel(const MaskGenParams P) {
    __shared__ __attribute__((aligned(16))) uint16_t patch[MMT_MASK_GEN_WAVES * MMT_MASK_PATCH_WORDS];
    attn_mask_gen_block(mask_gen_layer(P, blockIdx.y), patch, (size_t)blockIdx.x * (64 * MMT_MASK_GEN_WAVES), MMT_MASK_GEN_WAVES);
}

__host__ inline size_t attn_mask_layer_words(int nbh, int nt) { return (size_t)nbh * nt * nt * 64; }      // uint16 words per layer and orientation

// ---- consumer side -------------------------------------------------------------------------------------------------
// all-ones where bit I of the lane's tile word is set (kept), zero where it is clear (dropped): ONE v_bfe_i32.  Written as asm with
// the bit index as an immediate: from `(int)w << (31 - i) >> 31` or __builtin_amdgcn_sbfe hipcc 7.2 builds v_and (1 << i) + v_cmp_ne +
// v_cndmask for the AND that follows — three instructions per score where two do (found in the ISA of both attention hot loops).
// (Its source is a word loaded long before and its consumer an ordinary v_and: no MFMA / transcendental hazard is involved.)
template <int I> struct IdxC { static constexpr int value = I; };
template <int B, int E, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) { f(IdxC<B>{}); static_for<B + 1, E>(f); }
}
template <int I> __device__ __forceinline__ uint32_t keep_bits(uint32_t w) {
    uint32_t m;
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(w), "n"(I));
    return m;
}
template <int I> __device__ __forceinline__ float keep_and(float v, uint32_t w) {
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) & keep_bits<I>(w));
}
// the lane-mask form: +0 in the lanes whose bit of the 64-bit mask `m` (wave-uniform: a scalar register pair) is clear — the value
// v & 0 has — by ONE v_cndmask_b32 with the pair as its condition: the inverse ballot makes the scalar the per-lane predicate itself.
// Not asm: its operand comes straight out of v_exp_f32, and hipcc's hazard recognizer puts the wait state a transcendental's reader
// needs on gfx950 only in front of instructions it can see (an asm v_cndmask here read registers the exponential had not written
// yet: NaN gradients at T = 257).
__device__ __forceinline__ float keep_lanes(float v, uint64_t m) {
    return __builtin_amdgcn_inverse_ballot_w64(m) ? v : 0.f;
}
// one block of the lane-mask form: sixteen 64-bit words, fetched through the constant address space so that a wave-uniform address
// gives scalar loads (the arrays are written by an earlier launch and never by the reading kernel).  volatile: the loads stay where
// the caller wrote them — hipcc otherwise sinks them next to their first use, behind LDS reads whose wait then exposes their latency
typedef uint64_t u64x8_t __attribute__((ext_vector_type(8)));
struct LaneMasks { u64x8_t lo, hi; };                   // words 0..7, 8..15
__device__ __forceinline__ LaneMasks load_lane_masks(const uint16_t* block) {
    typedef const volatile u64x8_t __attribute__((address_space(4))) * cptr;
    const cptr p = (cptr)(uintptr_t)block;
    LaneMasks m;
    m.lo = p[0]; m.hi = p[1];
    return m;
}

// ---- test hook: expand the generator's decisions to one byte per (bh, query, key) ------------------------------------
__global__ void attn_mask_expand_kernel(DropCfg base, int nbh, int nt, uint8_t* __restrict__ keep) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per_bh = (size_t)nt * nt;
    const int bh = (int)(g / per_bh);
    if (bh >= nbh) return;
    const int rem = (int)(g - (size_t)bh * per_bh), qt = rem / nt, kt = rem - qt * nt;
    const DropCfg dc = drop_substream(base, (uint32_t)bh);
    uint32_t W[32];
    attn_keep_block(dc, (uint32_t)(qt * nt + kt), W);
    const size_t Tp = (size_t)nt * 32;
#pragma unroll
    for (int key = 0; key < 32; ++key)
#pragma unroll 1
        for (int q = 0; q < 32; ++q)
            keep[((size_t)bh * Tp + qt * 32 + q) * Tp + kt * 32 + key] = (W[key] >> q) & 1u;
}
