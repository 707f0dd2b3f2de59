// Scaled-dot-product attention core for gfx950, forward and backward, over per-(batch,head)
// fragment-layout operands (common.h).  No (T x T) tensor is ever materialised
// (the reference does: transformer/MFT/multiTransformer.py:27-34).
//
// Mask semantics of the reference (query-ROW blanking, keys never masked, :29-31,48-50) are applied
// by the producers/consumers of these operands, not here: a blanked row arrives as Q' = 0, which
// soft-maxes to exactly 1/T over all T keys like the reference's constant -1e9 row, and its dQ is
// zeroed by attn_bwd_dq_kernel (which takes the row mask).  Otherwise only index masking lives here:
// keys/queries >= T in the last tile.
//
// Key lengths (opt-in, the *_keys_kernel entries): sequence b sees keys 0 .. len[b]-1 only.  That IS the tail masking
// with T replaced by len[b]: the key-sweeping kernels run ceil(len/32) tiles and their peeled tail compares against len; the dK/dV
// kernel, whose waves own key tiles, masks the tile on the boundary and stores zeros for the tiles behind it.  Every kernel body
// below is written once, as a __device__ function with a compile-time KEYS flag; the plain kernels instantiate KEYS = false, in which
// every use of the length folds away.  A length is read once per workgroup, clamped into [1, T], and is wave-uniform.
//
// Causal (opt-in, the *_causal_kernel entries): query t sees keys 0 .. t of its sequence.  The flag of the bodies is a
// three-valued compile-time MODE (plain, keys, causal), so keys and causal cannot be combined.  A wave that owns query tile qt sweeps
// key tiles 0 .. qt: the tiles in front of the diagonal run the full body, the diagonal tile a separately instantiated DIAG body
// (key > query, or key >= T, masked by a select), and behind it the wave only keeps staging for the workgroup, whose sweep ends at
// the diagonal of its last query tile.  The dK/dV kernel, whose waves own key tiles, mirrors that: idle in front of the diagonal.
//
// Band (opt-in, the *_band_kernel entries, one more argument `int span` >= 1): query t sees keys max(0, t-span+1) .. t of
// its sequence — causal with a lower edge.  MODE's fourth value.  The visible key tiles of query tile qt are band_lo_tile(qt) .. qt, the
// query tiles that see key tile kt are kt .. band_hi_tile(kt); a workgroup stages from the lowest tile of its first wave to the highest
// of its last, and a wave is idle (staging and the barrier only) outside its own range.  At most three tiles of a wave are partial — the
// diagonal, and the two on the far edge — and they coincide when span <= 32.  Every working tile of a band runs ONE body, EDGE, whose
// select is (unsigned)(query - key) < span, with the query clamped to T-1 in the key-sweeping kernels (key <= query < T then needs no
// test of its own, and a row >= T, never stored, keeps finite values) and `query < T` tested beside it in the dK/dV kernel; in a tile
// between the edges the select passes everything.  Straight-line code behind the MFMA, always a select, never a multiplier.  A second
// instantiation for the tiles between (the full body, chosen per tile in the sweep loop) saves those tiles three vector instructions
// per score but costs the forward 13-40 VGPRs and dK/dV 8-24, a wave per SIMD in 7 of the 18 instances (DESIGN.md 4.10 has both
// tables): the one body was kept, as attn_probs_causal chose for the same reason.
// FIRST-TILE RULE: in a lower-edge tile a row may have no visible key at all (span 64, row 31, key tile qt-2), and the forward's first
// tile sets the running maximum to the tile maximum whatever its sign: -inf there, and the sweep would form -inf - (-inf).  So the band
// forward sweeps its key tiles DOWNWARDS from the diagonal: the first working tile is the one in which every row sees its own key and
// has a finite maximum; a later all-masked row has tile maximum -inf, never moves the reference (fmaxf(-inf, 0) = 0) and contributes
// P = 2^-inf = 0.  The rest of the rule is unchanged.  dQ and dK/dV have no running state and sweep upwards.  The plain, keyed and
// causal kernels keep their ascending sweep and their bits.
//
// Scores are kept in the log2 domain: the producer stores Q' = (x Wq^T + bq) * log2(e)/sqrt(d_k), so
// P = 2^(S' - L) with L = rowmax + log2(rowsum) saved per query for the backward pass.
#pragma once
#include <type_traits>
#include "common.h"
#include "attn_mask.h"

// ------------------------------------------------------------------------------------------------
// d_k = 64 (DKP = 64): the score products contract over all 64 features (KS = 4 k-steps), but a 32x32 MFMA accumulator holds only 32
// feature rows of an output (O^T, dK^T, dV^T, dQ^T): each launch produces ONE 32-feature block `fb` of its outputs and the host
// launches twice — the scores are evaluated twice, which this rarely used head size (no BASELINE config has d_k > 32) can afford.
// All three kernels below: a 1-D grid decoded by attn_block() into (tile quad, batch*head), 4 waves per workgroup, each wave owning one 32-window
// tile of its own and sweeping the other axis.  The swept operand tile (K/V for the forward and dQ kernels,
// Q/dO/L/delta for the dK-dV kernel) is the same for the four waves, so the workgroup stages it into LDS
// cooperatively: 2-3 coalesced 16-byte loads per thread, issued one tile AHEAD into registers while the current
// tile computes, written to the other half of a double buffer, one barrier per tile.  The LDS image keeps the
// global fragment layout (R: lane-linear 16-byte pieces), so a wave's MFMA operand for a product that contracts over
// features is a conflict-free ds_read_b128; operands of products that contract over windows come out of the same
// tiles through transposing reads (common.h tr_frag2; those tiles keep their 8-feature groups 576 bytes apart).
// Register budgets stay near 80-130 VGPRs: 3-5 waves share a SIMD.
template <int NSEG, int MAXL = 3>
struct TileStager {
    // segment i: `pieces[i]` 16-byte pieces per tile, read from base[i] + tile * stride[i] (bf16 elements); thread t moves pieces
    // t, t + 256, ... (MAXL = ceil(total pieces / 256) of them).  In LDS segment i starts at piece lds0[i] and leaves pad[i] pieces
    // free after every 32 (an R-layout tile that is read with transposing reads keeps its 8-feature groups 576 bytes apart:
    // the four groups a 32-lane half touches then fall into the four quarters of the 64 banks).
    const bf16* src[MAXL]; int stride[MAXL]; bool on[MAXL]; int dst[MAXL];
    bf16x8 reg[MAXL];
    __device__ __forceinline__ void init(const bf16* const* base, const int* pieces, const int* strides, const int* lds0, const int* pad, int tid) {
#pragma unroll
        for (int l = 0; l < MAXL; ++l) {
            const int p = tid + MMT_THREADS * l;
            int acc = 0; on[l] = false; src[l] = base[0]; stride[l] = 0; dst[l] = 0;
#pragma unroll
            for (int sg = 0; sg < NSEG; ++sg) {
                if (!on[l] && p >= acc && p < acc + pieces[sg]) {
                    on[l] = true; src[l] = base[sg] + (size_t)(p - acc) * 8; stride[l] = strides[sg];
                    dst[l] = (lds0[sg] + (p - acc) + ((p - acc) >> 5) * pad[sg]) * 8;
                }
                acc += pieces[sg];
            }
        }
    }
    __device__ __forceinline__ void load(int tile) {
#pragma unroll
        for (int l = 0; l < MAXL; ++l) if (on[l]) reg[l] = *reinterpret_cast<const bf16x8*>(src[l] + (size_t)tile * stride[l]);
    }
    __device__ __forceinline__ void store(bf16* lds) const {
#pragma unroll
        for (int l = 0; l < MAXL; ++l) if (on[l]) *reinterpret_cast<bf16x8*>(lds + dst[l]) = reg[l];
    }
};
#define MMT_TR_OCT 36        // pieces between the 8-feature groups of a padded R tile in LDS (32 windows + 4 free)

// all 16 registers = x in eight 64-bit moves (hipcc writes a splat as sixteen v_mov_b32).  The trailing s_nop covers the two
// wait states an MFMA needs after a VALU write of its SrcC: the hazard recognizer does not see through asm statements.
__device__ __forceinline__ void fill16(f32x16& v, float x) {
    const f32x2 xp = {x, x};
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        f32x2 t;
        if (i < 14) asm volatile("v_mov_b64 %0, %1" : "=v"(t) : "v"(xp));       // volatile: eight separate moves, not one plus copies
        else asm volatile("v_mov_b64 %0, %1\n\ts_nop 1" : "=v"(t) : "v"(xp));
        v[i] = t[0]; v[i + 1] = t[1];
    }
}
// ------------------------------------------------------------------------------------------------
// Forward.  S^T = K Q'^T puts the query on the lane column: running max / sum / rescale are lane-local and
// the only cross-lane step is one exchange between the two 32-lane halves.  After the first key tile the
// running max m is preloaded as the accumulator (S' = S - m straight out of the MFMA) and the state is only
// rescaled when some row's tile maximum exceeds m by more than RESCALE_THR (then P <= 2^THR, harmless in
// bf16/fp32): the common path per score is max3 + exp + convert.  P^T (keys in registers) is fed straight
// back as the B operand of O^T += V^T P^T.  For DKP == 16 the idle half of that MFMA also forms the row sums
// (row 16 of V^T is synthesised as ones) unless dropout is on (the normaliser uses the undropped P).
#define MMT_RESCALE_THR 8.0f

// Workgroup -> (tile quad bx, batch*head bh).  The (nt+3)/4 workgroups that sweep the same (batch, head) all stream
// that head's whole K/V (forward) or Q/dO (backward) fragments.  The hardware deals consecutive workgroup ids round-robin
// to the 8 XCDs, each with a private L2, so a plain 2-D grid would put the sharers on different XCDs and fetch the
// operands once per sharer from the fabric (measured with FETCH_SIZE: 2.5-3x the operand bytes).  A 1-D grid of
// nx * 8 * ceil(nbh/8) ids is decoded so that ids congruent mod 8 — same XCD — carry the same head.
// Progress-based wave priority.  The four waves that share a SIMD in these kernels belong to four different workgroups; the SIMD
// arbitrates vector issue by priority, then AGE, so at equal priority the oldest wave runs almost unimpeded and the youngest
// starves: measured wave lifetimes in attn_fwd_kernel spread from 31k to 56k cycles for identical work, and while the last
// waves finish alone the SIMD issues at a fraction of its four-wave rate (a wave by itself issues one vector instruction per
// 6-12 cycles: tools/valu_micro.hip).  Each wave therefore LOWERS its priority as it advances through its sweep (3 in the first
// quarter .. 0 in the last): whoever is behind goes first, the waves of a SIMD finish together, and no tail is left.
__device__ __forceinline__ void progress_prio(int step, int nsteps) {
    const int q1 = (nsteps + 3) >> 2, q2 = (nsteps + 1) >> 1, q3 = (3 * nsteps + 3) >> 2;      // wave-uniform
    if (step == 0) __builtin_amdgcn_s_setprio(3);
    else if (step == q1) __builtin_amdgcn_s_setprio(2);
    else if (step == q2) __builtin_amdgcn_s_setprio(1);
    else if (step == q3) __builtin_amdgcn_s_setprio(0);
}

// keys sequence b attends to: its key length clamped into [1, T] (no value of that tensor moves an access out of bounds), as a scalar
__device__ __forceinline__ int attn_key_len(const int* __restrict__ key_lengths, int b, int T) {
    return __builtin_amdgcn_readfirstlane(min(max(key_lengths[b], 1), T));
}

enum AttnMode { ATTN_PLAIN = 0, ATTN_KEYS = 1, ATTN_CAUSAL = 2, ATTN_BAND = 3 };
// tags of the tile bodies: the hot tile, the tile that holds the tail of the swept axis, the tile on the causal diagonal, a partial tile
// of a band (its diagonal and its far edge; the band kernels run it on every tile)
using TileFull = std::integral_constant<int, 0>;
using TileTail = std::integral_constant<int, 1>;
using TileDiag = std::integral_constant<int, 2>;
using TileEdge = std::integral_constant<int, 3>;
// band: the lowest key tile that a query of tile qt sees, the highest query tile that sees a key of tile kt (span <= T: no overflow)
__device__ __forceinline__ int band_lo_tile(int qt, int span) { return max(0, (32 * qt - span + 1) >> 5); }
__device__ __forceinline__ int band_hi_tile(int kt, int span, int nt) { return min(nt - 1, (32 * kt + 30 + span) >> 5); }

struct AttnBlock { int bx, bh; bool valid; };
__device__ __forceinline__ AttnBlock attn_block(int nx, int nbh) {
    const int L = blockIdx.x, grp = L / (8 * nx), rem = L - grp * 8 * nx;
    AttnBlock a;
    a.bx = rem >> 3;
    a.bh = grp * 8 + (rem & 7);
    a.valid = a.bh < nbh;
    return a;
}
__host__ inline int attn_grid(int nx, int nbh) { return nx * 8 * ((nbh + 7) / 8); }
// Causal: the tile quads of a head sweep 4, 8, .. key tiles (forward, dQ; dK/dV the other way round), and the whole grid of a training
// shape is resident at once, so a launch lasts as long as the CU that holds the most work.  With attn_block's decoding the workgroups
// an XCD receives carry bx = 0, 1, .. nx-1, 0, 1, ..: dealt round-robin to its 32 CUs, every workgroup of a CU has the SAME bx when nx
// divides 32, and the CUs of the last quads set the time (measured: DESIGN.md 4.4).  Rotating bx by one per 32 workgroups of the XCD
// gives each CU every quad in turn; ids congruent mod 8 still carry the same head, and (bx, bh) is still hit exactly once.
__device__ __forceinline__ AttnBlock attn_block_causal(int nx, int nbh) {
    AttnBlock a = attn_block(nx, nbh);
    const int grp = blockIdx.x / (8 * nx);
    a.bx = (a.bx + ((grp * nx) >> 5)) % nx;
    return a;
}

// (`//@ name` comment lines mark the phase boundaries at which tools/make_diag.py inserts cycle stamps into the GENERATED stamped twin of this
// kernel — diagnostic builds only; this file holds no diagnostic code)
// LANES: the keep bits come as 64-bit lane masks, one per accumulator register, in scalar registers (attn_mask.h, the lane-mask form
// of LQ) — the plain d_k = 16 train kernel only; the host gives the generator the same choice.
template <int DKP, bool DROP, int MODE, bool LANES = false>
__device__ __forceinline__ void attn_fwd_body(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        bf16* __restrict__ ctx, float* __restrict__ lse,
        int h, int T, int nt, int nbh, int ldc, const uint16_t* __restrict__ maskQ, float drop_scale, int fb,
        const int* __restrict__ key_lengths, int span) {
    constexpr bool KEYS = MODE == ATTN_KEYS, CAUSAL = MODE == ATTN_CAUSAL, BAND = MODE == ATTN_BAND;
    constexpr int KS = DKP / 16;
    constexpr int DKB = DKP < 32 ? DKP : 32;           // feature rows of this launch's output block
    constexpr bool ONES = (DKP == 16) && !DROP;        // row sums through the MFMA
    static_assert(!LANES || (DROP && DKP == 16 && MODE == ATTN_PLAIN), "lane masks: the plain d_k = 16 train kernel only");
    //@ entry
    // 16-byte pieces per tile: K (R layout, all DKP features) and the 32-feature block `fb` of V — ALSO in the R layout, as the QKV
    // epilogue wrote it: the PV product contracts over keys, its A fragment (8 keys of one feature per lane) comes out of LDS
    // through transposing reads (tr_frag2), so no transposed copy of V exists in memory
    constexpr int PK = DKP * 4, PV = DKB * 4, PVL = (DKB / 8) * MMT_TR_OCT;
    __shared__ __attribute__((aligned(16))) bf16 stage[2][(PK + PVL) * 8];
    __shared__ __attribute__((aligned(16))) bf16 zeros[256];          // what the lanes of the padding feature rows (>= d_k) read
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const AttnBlock ab = CAUSAL ? attn_block_causal((nt + 3) >> 2, nbh) : attn_block((nt + 3) >> 2, nbh);
    if (!ab.valid) return;                              // whole workgroup, before any barrier
    const int qt = ab.bx * 4 + wave;
    const bool live = qt < nt;                          // idle waves still stage and synchronise
    const int qtc = live ? qt : nt - 1;
    const int bh = ab.bh, b = bh / h, head = bh - b * h;
    const int Tp = nt * 32;
    // keys that exist for this sequence and the tiles that hold them: (T, nt), or the sequence's key length and its tiles;
    // causal: the workgroup's sweep ends at the diagonal of its last query tile
    const int Tk = KEYS ? attn_key_len(key_lengths, b, T) : T;
    const int nk = KEYS ? (Tk + 31) >> 5 : (CAUSAL || BAND) ? min(nt, ab.bx * 4 + 4) : nt;
    // band: the workgroup sweeps DOWNWARDS from tile nk-1 to kw0, this wave works in qt .. klo of them; sp: the span, at most T
    const int sp = BAND ? min(span, T) : 0;
    const int kw0 = BAND ? band_lo_tile(ab.bx * 4, sp) : 0, klo = BAND ? band_lo_tile(qtc, sp) : 0;
    const int kfirst = BAND ? nk - 1 : 0;               // the first tile staged
    const int qrel = BAND ? min(qtc * 32 + r, T - 1) : 0;      // band: this lane's query, clamped (a row >= T, never stored, acts as row T-1)
    const bf16* Qb = Qr + (size_t)bh * fragR_elems(Tp, DKP);
    const bf16* Kb = Kr + (size_t)bh * fragR_elems(Tp, DKP);
    const bf16* Vb = Vr + (size_t)bh * fragR_elems(Tp, DKP) + (size_t)fb * 4 * 256;      // feature group 4 fb of tile 0
    // dropout: this lane's 16-bit words of the wave's row of mask blocks (attn_mask.h, LQ layout), one per key tile, fetched a tile ahead
    // (LANES: no per-lane words; the wave's row of blocks starts at block mblk0, a scalar)
    const uint16_t* mrow = maskQ + ((size_t)bh * nt + qtc) * nt * 64 + lane;
    uint32_t mw = (DROP && !LANES) ? mrow[BAND ? (size_t)qtc * 64 : 0] : 0u;      // band: the wave's first working tile is its diagonal one
    const uint32_t mblk0 = LANES ? __builtin_amdgcn_readfirstlane((uint32_t)((bh * nt + qtc) * nt)) : 0u;

    TileStager<2, (PK + PV + MMT_THREADS - 1) / MMT_THREADS> stg;
    {
        const bf16* base[2] = {Kb, Vb};
        const int pieces[2] = {PK, PV}, strides[2] = {32 * DKP, 32 * DKP}, lds0[2] = {0, PK}, pad[2] = {0, MMT_TR_OCT - 32};
        stg.init(base, pieces, strides, lds0, pad, threadIdx.x);
    }
    stg.load(kfirst);
    zeros[threadIdx.x] = (bf16)0.f;
    // transposing-read role of this lane in the V tile: its feature row r = 16 g1 + (lane & 15) is delivered by the hardware; the
    // address it SUPPLIES is that of window q = (lane >> 2) & 3 of a 4-window block, features 16 g1 + 4 pp .. + 3, pp = lane & 3.
    // Key order of the fragment = row order of the P^T accumulator: slot j <-> key 16 s2 + 8 (j >> 2) + 4 hh + (j & 3).
    const int g1 = (lane >> 4) & 1, tq = (lane >> 2) & 3, tpp = lane & 3;
    const int voff = ((2 * g1 + (tpp >> 1)) * MMT_TR_OCT + 4 * hh + tq) * 8 + 4 * (tpp & 1);
    const bool vpad = DKB < 32 && g1;                   // feature rows >= 16 at d_k = 16: zeros (or the ones row, below)
    bf16x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
        qf[s] = *reinterpret_cast<const bf16x8*>(Qb + ((size_t)(qtc * (DKP / 8) + 2 * s + hh) * 32 + r) * 8);
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.0f;
    stg.store(stage[kfirst & 1]);
    __syncthreads();

    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    float mrun = 0.f, lrun = 0.f;
    f32x16 mneg;                                        // -mrun in every register: the accumulator init of the score product
#pragma unroll
    for (int i = 0; i < 16; ++i) mneg[i] = 0.f;

    // The tile body is instantiated twice: TAIL = false for the hot loop (no conditional code between an MFMA and the
    // consumers of its result: hipcc's hazard recognizer counts a skippable block's instructions as MFMA->VALU wait
    // states, which is wrong on the taken path — seen as 27 % wrong dQ in attn_bwd_dq_kernel<32>), TAIL = true for the
    // last key tile, whose index masking is then straight-line code.
    //@ prologue
    auto body = [&](auto tile_tag, int kt) {
        constexpr bool TAIL = (int)decltype(tile_tag)::value == 1, DIAG = (int)decltype(tile_tag)::value == 2;
        constexpr bool EDGE = (int)decltype(tile_tag)::value == 3;
        // the workgroup stages one tile ahead: compile-time off in the last tile of a plain or keyed sweep; causal: the wave's
        // diagonal tile is not the workgroup's last one unless the wave owns the last query tile; band: the next tile is the one below
        const bool more = BAND ? kt > kw0 : CAUSAL ? kt + 1 < nk : !TAIL;
        const int knext = BAND ? kt - 1 : kt + 1;
        //@ loop_top
        progress_prio(BAND ? qt - kt : kt, BAND ? qt - klo + 1 : nk);
        const uint32_t tw = mw;                          // this tile's keep bits
        if (BAND) { if (DROP && kt > klo) mw = mrow[(size_t)(kt - 1) * 64]; }
        else if (DROP && !LANES && !TAIL && !DIAG) mw = mrow[(size_t)(kt + 1) * 64];
        if (more) stg.load(knext);                      // next tile in flight behind this tile's arithmetic
        const bf16* sk = stage[kt & 1];
        const bf16* sv = vpad ? zeros : sk + PK * 8 + voff;
        // S' - m straight out of the MFMA: the accumulator init is a register set that holds -m for the whole sweep and is rewritten
        // only when the reference moves (round 3 splatted -m into the accumulator before every tile: 8 v_mov_b64 of ~100 vector
        // instructions per tile)
        f32x16 s;
        LaneMasks lm;
        if constexpr (KS == 1) {
            // written as asm because hipcc only knows the tied form (vdst = srcC) of an MFMA on VGPRs and would copy mneg into s first;
            // the trailing s_nop are the wait states between an 8-pass MFMA and a vector instruction that reads its result, which the
            // hazard recognizer cannot add for an asm statement
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sk + (hh * 32 + r) * 8);
            if constexpr (LANES) {
                // This tile's sixteen lane masks, 128 bytes at a wave-uniform address: two scalar loads, issued HERE — behind the wait
                // for the tile's only LDS read in front of the mask phase and ahead of the score product — because scalar loads count on
                // the LDS wait counter and return out of order: any LDS wait with one in flight waits for it too.  From here to the mask
                // phase (product, maximum, exp, row sum) the wave waits for no LDS result.  The place is pinned from both sides: the
                // address passes through an empty asm that needs kf, and nothing is scheduled across the barrier behind the loads.
                uint32_t blk = mblk0 + (uint32_t)kt;
                asm volatile("" : "+s"(blk) : "v"(kf));
                lm = load_lane_masks(maskQ + (size_t)blk * 64);
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3\n\ts_nop 11" : "=&v"(s) : "v"(kf), "v"(qf[0]), "v"(mneg));
        } else {
            s = mfma32(*reinterpret_cast<const bf16x8*>(sk + (hh * 32 + r) * 8), qf[0], mneg);
#pragma unroll
            for (int ss = 1; ss < KS; ++ss)
                s = mfma32(*reinterpret_cast<const bf16x8*>(sk + ((2 * ss + hh) * 32 + r) * 8), qf[ss], s);
        }
        if (TAIL) {                                     // keys >= T (>= the key length) do not exist
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = (kt * 32 + acc32_row(i, hh) < Tk) ? s[i] : -INFINITY;
        }
        if (DIAG) {                                     // kt == qt: keys behind the query, and keys >= T, do not exist.  Key 32 kt is
#pragma unroll                                          // visible to every query of the tile, so every row keeps a finite maximum
            for (int i = 0; i < 16; ++i) s[i] = (acc32_row(i, hh) <= r && kt * 32 + acc32_row(i, hh) < T) ? s[i] : -INFINITY;
        }
        if (EDGE) {                                     // band: keys query-span+1 .. query exist.  On the diagonal (the first tile of the
#pragma unroll                                          // downward sweep) every row sees its own key; on the far edge a row may see none
            for (int i = 0; i < 16; ++i) s[i] = ((unsigned)(qrel - kt * 32 - acc32_row(i, hh)) < (unsigned)sp) ? s[i] : -INFINITY;
        }
        // (no inline asm here: hipcc's hazard recognizer does not count an asm statement as a reader of MFMA results)
        float tmax = fmaxf(fmaxf(s[0], s[1]), s[2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2) tmax = fmaxf(fmaxf(tmax, s[i]), s[i + 1]);
        tmax = fmaxf(tmax, s[15]);                      // over this lane's 16 keys; the other half of the wave holds the query's other 16
        //@ qk_max
        const int kone = BAND ? qt : 0;                 // the wave's first working tile
        if (kt == kone || __any(tmax > MMT_RESCALE_THR)) {        // __any looks at both halves: no exchange on the common path
            // move the reference to the new running max (first tile: from 0 to the tile max, with o = l = 0)
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));  // finite: every tile holds >= 1 real key in one of the halves (band: in the first
            const float dlt = (kt == kone) ? tmax : fmaxf(tmax, 0.f);      // tile; -inf in a later one leaves the reference where it is)
            // alpha <= 1: a first tile whose maximum is below -128 would give 2^(-dlt) = inf, and o = l = 0 times inf is NaN
            const float alpha = fast_exp2(-fmaxf(dlt, 0.f));
            mrun += dlt;
            lrun *= alpha;
#pragma unroll
            for (int i = 0; i < 16; ++i) { o[i] *= alpha; s[i] -= dlt; }
            fill16(mneg, -mrun);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = fast_exp2(s[i]);
        if (!ONES) {        // row sum of the tile as ONE chain of plain adds: a wave issues a vector instruction every 6+ cycles
            float a = s[0];             // anyway, so the dependency costs nothing, and a v_add_f32 takes 1.6 cycles of SIMD issue where the
#pragma unroll                          // v_pk_add_f32 that two parallel chains get packed into takes 3.7 (tools/valu_micro.hip)
            for (int i = 1; i < 16; ++i) a += s[i];
            lrun += a;
        }
        //@ exp_sum
        if (DROP) {                                     // zero the dropped probabilities; 1/(1-p) is applied once, to the output row
            if constexpr (LANES) {
#pragma unroll
                for (int i = 0; i < 8; ++i) { s[i] = keep_lanes(s[i], lm.lo[i]); s[8 + i] = keep_lanes(s[8 + i], lm.hi[i]); }
            } else static_for<0, 16>([&](auto ic) { constexpr int i = decltype(ic)::value; s[i] = keep_and<i>(s[i], tw); });
        }
        //@ mask
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 va = tr_frag2(sv + 128 * s2, sv + 128 * s2 + 64);       // keys 16 s2 + 4 hh + {0..3}, then + 8
            if (ONES && r == DKP) va = ones;           // V^T rows >= DKP read zeros; row DKP becomes the ones row
            o = mfma32(va, pack8(s, s2), o);
        }
        //@ pv
        if (more) stg.store(stage[knext & 1]);
        //@ stage_wait
        __syncthreads();        // stage[(kt+1)&1] was last read at tile kt-1, i.e. before the previous barrier
        //@ barrier
    };
    if constexpr (CAUSAL) {
        // three wave-uniform states, each a whole body: in front of the diagonal, on it, behind it (and a wave without a query tile):
        // nothing to compute, but the workgroup stages cooperatively — keep moving pieces and meet the one barrier per tile
        for (int kt = 0; kt < (live ? qt : 0); ++kt) body(TileFull{}, kt);
        if (live) body(TileDiag{}, qt);
        __builtin_amdgcn_s_setprio(0);
        for (int kt = live ? qt + 1 : 0; kt < nk; ++kt) {
            if (kt + 1 < nk) { stg.load(kt + 1); stg.store(stage[(kt + 1) & 1]); }
            __syncthreads();
        }
    } else if constexpr (BAND) {
        // downwards: idle above the wave's diagonal, the EDGE body from it to the wave's lowest tile, idle below
        auto idle = [&](int kt) {
            if (kt > kw0) { stg.load(kt - 1); stg.store(stage[(kt - 1) & 1]); }
            __syncthreads();
        };
        int kt = nk - 1;
        for (; kt > (live ? qt : kw0 - 1); --kt) idle(kt);
        if (live) {
            for (; kt >= klo; --kt) body(TileEdge{}, kt);
            __builtin_amdgcn_s_setprio(0);
            for (; kt >= kw0; --kt) idle(kt);
        }
    } else {
        for (int kt = 0; kt < nk - 1; ++kt) body(TileFull{}, kt);
        body(TileTail{}, nk - 1);
    }
    //@ swept
    if (!live) return;
    float ltot;
    if (ONES) ltot = __shfl(o[8], r);                  // O^T row 16 = (register 8, lower half): the row sums
    else ltot = lrun + __shfl_xor(lrun, 32);
    const float inv = (DROP ? drop_scale : 1.0f) / ltot;    // kept probabilities carry 1/(1-p)
    const int t = qt * 32 + r;
    if (t < T) {
        const size_t m = (size_t)b * T + t;
        if (hh == 0) lse[(size_t)bh * Tp + t] = -(mrun + fast_log2(ltot));   // stored NEGATED: it is the accumulator init of the backward
        // O^T rows (head features) live in registers: e = acc32_row(i, hh); groups of 4 are contiguous
#pragma unroll
        for (int g = 0; g < DKB / 8; ++g) {
            bf16x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (bf16)(o[4 * g + i] * inv);
            const int e0 = 32 * fb + 8 * g + 4 * hh;
            *reinterpret_cast<bf16x4*>(ctx + m * ldc + head * DKP + e0) = v;
        }
    }
    //@ exit
}
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_fwd_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        bf16* __restrict__ ctx, float* __restrict__ lse,
        int h, int T, int nt, int nbh, int ldc, const uint16_t* __restrict__ maskQ, float drop_scale, int fb) {
    attn_fwd_body<DKP, DROP, ATTN_PLAIN>(Qr, Kr, Vr, ctx, lse, h, T, nt, nbh, ldc, maskQ, drop_scale, fb, nullptr, 0);
}
// ... at d_k = 16 in train mode with maskQ in the lane-mask form (DROP: always true — a template so that tools/make_diag.py can twin it)
template <bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_fwd_lanes16_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        bf16* __restrict__ ctx, float* __restrict__ lse,
        int h, int T, int nt, int nbh, int ldc, const uint16_t* __restrict__ maskQ, float drop_scale, int fb) {
    attn_fwd_body<16, DROP, ATTN_PLAIN, true>(Qr, Kr, Vr, ctx, lse, h, T, nt, nbh, ldc, maskQ, drop_scale, fb, nullptr, 0);
}
// ... with key lengths: sequence b attends keys < key_lengths[b]
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_fwd_keys_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        bf16* __restrict__ ctx, float* __restrict__ lse,
        int h, int T, int nt, int nbh, int ldc, const uint16_t* __restrict__ maskQ, float drop_scale, int fb,
        const int* __restrict__ key_lengths) {
    attn_fwd_body<DKP, DROP, ATTN_KEYS>(Qr, Kr, Vr, ctx, lse, h, T, nt, nbh, ldc, maskQ, drop_scale, fb, key_lengths, 0);
}
// ... causal: query t attends keys <= t
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_fwd_causal_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        bf16* __restrict__ ctx, float* __restrict__ lse,
        int h, int T, int nt, int nbh, int ldc, const uint16_t* __restrict__ maskQ, float drop_scale, int fb) {
    attn_fwd_body<DKP, DROP, ATTN_CAUSAL>(Qr, Kr, Vr, ctx, lse, h, T, nt, nbh, ldc, maskQ, drop_scale, fb, nullptr, 0);
}
// ... band: query t attends keys max(0, t - span + 1) .. t
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_fwd_band_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        bf16* __restrict__ ctx, float* __restrict__ lse,
        int h, int T, int nt, int nbh, int ldc, const uint16_t* __restrict__ maskQ, float drop_scale, int fb, int span) {
    attn_fwd_body<DKP, DROP, ATTN_BAND>(Qr, Kr, Vr, ctx, lse, h, T, nt, nbh, ldc, maskQ, drop_scale, fb, nullptr, span);
}

// ------------------------------------------------------------------------------------------------
// Backward, part A: dK, dV.  Wave w owns key tile kt = 4*blockIdx.x + w (the key on the lane column) and
// sweeps all query tiles, keeping dK^T, dV^T in accumulators.  Per query tile:
//     S'  = Q' K^T - L      (-L, stored negated, is the accumulator init: P = 2^S' needs no subtraction)
//     dPc = dO V^T - delta  (same trick with -delta = -rowsum(dO . O))
//     dS  = P * dPc ;  dV^T += dO^T P ;  dK^T += Q'^T dS     (P, dS accumulators ARE the B operands)
template <int DKP, bool DROP, int MODE>
__device__ __forceinline__ void attn_bwd_dkv_body(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr, const bf16* __restrict__ dOr,
        const float* __restrict__ lse, const float* __restrict__ delta,
        bf16* __restrict__ dkv, int lddkv,      // row-major [M][lddkv]; dK at column HD, dV at 2*HD
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskK, float drop_scale, int fb,
        const int* __restrict__ key_lengths, int span) {
    constexpr bool KEYS = MODE == ATTN_KEYS, CAUSAL = MODE == ATTN_CAUSAL, BAND = MODE == ATTN_BAND;
    constexpr int KS = DKP / 16;
    constexpr int DKB = DKP < 32 ? DKP : 32;
    // pieces: R-layout tile (in LDS with its 8-feature groups 576 bytes apart: the products that contract over the queries read
    // their A fragments out of these tiles with transposing reads, like attn_fwd_kernel reads V), 32 fp32 row constants
    constexpr int PR = DKP * 4, PRL = (DKP / 8) * MMT_TR_OCT, PC = 8;
    constexpr int TOTAL = 2 * PR + 2 * PC, TOTAL_LDS = 2 * PRL + 2 * PC;
    __shared__ __attribute__((aligned(16))) bf16 stage[2][TOTAL_LDS * 8];
    __shared__ __attribute__((aligned(16))) bf16 zeros[256];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const AttnBlock ab = CAUSAL ? attn_block_causal((nt + 3) >> 2, nbh) : attn_block((nt + 3) >> 2, nbh);
    if (!ab.valid) return;                              // whole workgroup, before any barrier
    const int kt = ab.bx * 4 + wave;
    const bool live = kt < nt;
    const int ktc = live ? kt : nt - 1;
    const int bh = ab.bh, b = bh / h, head = bh - b * h;
    const int Tp = nt * 32, HD = h * DKP;
    const int Tk = KEYS ? attn_key_len(key_lengths, b, T) : T;          // keys that exist for this sequence
    // dK = dV = 0 for this lane's key (a key that no query attends), 32-feature block fb
    auto store_zeros = [&]() {
        const int t = kt * 32 + r;
        if (!live || t >= T) return;
        const size_t m = (size_t)b * T + t;
        const bf16x4 z = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
#pragma unroll
        for (int g = 0; g < DKB / 8; ++g) {
            const int e0 = head * DKP + 32 * fb + 8 * g + 4 * hh;
            *reinterpret_cast<bf16x4*>(dkv + m * lddkv + HD + e0) = z;
            *reinterpret_cast<bf16x4*>(dkv + m * lddkv + 2 * HD + e0) = z;
        }
    };
    if (KEYS && ab.bx * 128 >= Tk) { store_zeros(); return; }          // all four key tiles behind the length: whole workgroup, before any barrier
    const size_t offR = (size_t)bh * fragR_elems(Tp, DKP);
    const bf16 *Krb = Kr + offR, *Vrb = Vr + offR;
    const uint16_t* mrow = maskK + ((size_t)bh * nt + ktc) * nt * 64 + lane;      // LK layout: this lane's word of one block per query tile
    const int q0 = (CAUSAL || BAND) ? ab.bx * 4 : 0;    // first query tile of the workgroup's sweep (causal: no earlier query sees its keys)
    // band: the wave works in query tiles kt .. qhi, the workgroup's sweep ends behind the last tile of its last live wave (nq == nt otherwise)
    const int sp = BAND ? min(span, T) : 0;
    const int qhi = BAND ? band_hi_tile(ktc, sp, nt) : nt - 1;
    const int nq = BAND ? band_hi_tile(min(nt - 1, ab.bx * 4 + 3), sp, nt) + 1 : nt;
    uint32_t mw = DROP ? mrow[(size_t)((CAUSAL || BAND) ? ktc : 0) * 64] : 0u;      // causal: the wave's first working tile is its diagonal one
    const uint32_t scale_bits = __builtin_bit_cast(uint32_t, drop_scale);

    TileStager<4, (TOTAL + MMT_THREADS - 1) / MMT_THREADS> stg;
    {
        const bf16* base[4] = {Qr + offR, dOr + offR,
                               reinterpret_cast<const bf16*>(lse + (size_t)bh * Tp), reinterpret_cast<const bf16*>(delta + (size_t)bh * Tp)};
        const int pieces[4] = {PR, PR, PC, PC}, strides[4] = {32 * DKP, 32 * DKP, 64, 64};
        const int lds0[4] = {0, PRL, 2 * PRL, 2 * PRL + PC}, pad[4] = {MMT_TR_OCT - 32, MMT_TR_OCT - 32, 0, 0};
        stg.init(base, pieces, strides, lds0, pad, threadIdx.x);
    }
    stg.load(q0);
    zeros[threadIdx.x] = (bf16)0.f;
    bf16x8 kfr[KS], vfr[KS];
#pragma unroll
    for (int ss = 0; ss < KS; ++ss) {
        const size_t off = ((size_t)(ktc * (DKP / 8) + 2 * ss + hh) * 32 + r) * 8;
        kfr[ss] = *reinterpret_cast<const bf16x8*>(Krb + off);
        vfr[ss] = *reinterpret_cast<const bf16x8*>(Vrb + off);
    }
    // DKP == 16: a 32-row A fragment has 16 idle rows, so ONE accumulator serves both products: lanes r < 16 read dO^T (rows 0..15:
    // dV^T) and zeros for Q^T, lanes r >= 16 read Q^T features r - 16 (rows 16..31: dK^T) and zeros for dO^T.  16 VGPRs less
    // puts the kernel at 4 waves per SIMD.  DKP >= 32 keeps two accumulators.
    constexpr bool ONEACC = (DKP == 16);
    f32x16 dKacc, dVacc;
#pragma unroll
    for (int j = 0; j < 16; ++j) { dKacc[j] = 0.f; dVacc[j] = 0.f; }
    // transposing-read role (see attn_fwd_kernel): the lane supplies query tq of a 4-query block, features 4 tpp .. + 3 of its
    // 16-lane group's 16 features, and receives feature row r; slot j <-> query 16 s2 + 8 (j >> 2) + 4 hh + (j & 3)
    const int g1 = (lane >> 4) & 1, tq = (lane >> 2) & 3, tpp = lane & 3;
    const int toff = (((ONEACC ? 0 : 4 * fb + 2 * g1) + (tpp >> 1)) * MMT_TR_OCT + 4 * hh + tq) * 8 + 4 * (tpp & 1);
    // (causal: a key >= T is seen by queries >= T only, which the DIAG body masks)
    const bool key_tail = (CAUSAL || BAND) ? false : KEYS ? (ktc * 32 + 32 > Tk) : (ktc == nt - 1) && (T & 31);
    const bool key_ok = (ktc * 32 + r) < Tk;
    stg.store(stage[0]);                                // (q0 is a multiple of 4: tile qt sits in stage[qt & 1] in every mode)
    __syncthreads();
    if (KEYS && ktc * 32 >= Tk) {
        // a wave whose key tile lies wholly behind the length (wave-uniform; some other wave of the workgroup has visible keys): it has
        // nothing to sweep, but the workgroup stages cooperatively — it keeps moving its pieces and meets the one barrier per tile
        for (int qt = 0; qt < nt; ++qt) {
            if (qt + 1 < nt) { stg.load(qt + 1); stg.store(stage[(qt + 1) & 1]); }
            __syncthreads();
        }
        store_zeros();
        return;
    }

    // Tile body without conditional code (see attn_fwd_kernel): the key-tail mask is a per-lane multiplier that is
    // simply 1 everywhere except in the wave that owns the last key tile, and the query tail is the peeled last tile.
    // (KEYS: a select instead — a key behind the length is a real window, whose 2^(S' - L) may be inf)
    const float kmul = (key_tail && !key_ok) ? 0.f : 1.f;
    auto body = [&](auto tile_tag, int qt) {
        constexpr bool QTAIL = (int)decltype(tile_tag)::value == 1, DIAG = (int)decltype(tile_tag)::value == 2;
        constexpr bool EDGE = (int)decltype(tile_tag)::value == 3;
        const bool more = qt + 1 < nq;                  // scalar, loop-invariant except at the very last tile
        progress_prio(BAND ? qt - kt : qt - q0, BAND ? qhi - kt + 1 : nq - q0);
        const uint32_t tw = mw;
        if (DROP && more) mw = mrow[(size_t)(qt + 1) * 64];
        if (more) stg.load(qt + 1);
        const bf16* sq = stage[qt & 1];
        const bf16* sdo = sq + PRL * 8;
        const float* sl = reinterpret_cast<const float*>(sq + 2 * PRL * 8);
        const float* sd = sl + 32;
        const bf16* ado = (ONEACC && g1) ? zeros : sdo + toff;
        const bf16* aq = (ONEACC && !g1) ? zeros : sq + toff;
        f32x16 s, dp;                   // row constants (4 consecutive queries per register group) as the accumulators
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(sl + 8 * g + 4 * hh);
            f32x4 d4 = {0.f, 0.f, 0.f, 0.f};                                   // DROP: -delta enters after the mask
            if (!DROP) d4 = *reinterpret_cast<const f32x4*>(sd + 8 * g + 4 * hh);
#pragma unroll
            for (int i = 0; i < 4; ++i) { s[4 * g + i] = l4[i]; dp[4 * g + i] = d4[i]; }      // both stored negated
        }
#pragma unroll
        for (int ss = 0; ss < KS; ++ss) {
            const int o8 = ((2 * ss + hh) * MMT_TR_OCT + r) * 8;
            s = mfma32(*reinterpret_cast<const bf16x8*>(sq + o8), kfr[ss], s);
            dp = mfma32(*reinterpret_cast<const bf16x8*>(sdo + o8), vfr[ss], dp);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float pv = fast_exp2(s[j]);
            if (QTAIL) pv = (qt * 32 + acc32_row(j, hh) < T) ? pv : 0.f;      // queries >= T do not exist
            // qt == kt: neither do queries in front of the key (a select: L of such a query is from ITS keys, 2^(S' - L) may be inf)
            if (DIAG) pv = (acc32_row(j, hh) >= r && qt * 32 + acc32_row(j, hh) < T) ? pv : 0.f;
            // band: only queries key .. key+span-1 below T see the key (a select, for the same reason)
            if (EDGE) pv = ((unsigned)((qt - kt) * 32 + acc32_row(j, hh) - r) < (unsigned)sp && qt * 32 + acc32_row(j, hh) < T) ? pv : 0.f;
            s[j] = pv;
        }
        if (key_tail) {                                 // wave-uniform, loop-invariant: only the last key tile's wave pays
#pragma unroll
            for (int j = 0; j < 16; ++j) s[j] = KEYS ? (key_ok ? s[j] : 0.f) : s[j] * kmul;
        }
        if (DROP) {
            // dropped probabilities Pd = P*m/(1-p):  dV^T += dO^T Pd ;  dS = P * ((dO V^T)*m/(1-p) - delta); delta unchanged.
            // m = bit j of the lane's tile word (LK layout: the key on the lane, query acc32_row(j, hh) in register j)
            static_for<0, 4>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(sd + 8 * g + 4 * hh);
                static_for<0, 4>([&](auto ic) {
                    constexpr int i = decltype(ic)::value, j = 4 * g + i;
                    const float ms = __builtin_bit_cast(float, scale_bits & keep_bits<j>(tw));
                    dp[j] = s[j] * fmaf(dp[j], ms, d4[i]);
                    s[j] *= ms;
                });
            });
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) dp[j] *= s[j];
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            dVacc = mfma32(tr_frag2(ado + 128 * s2, ado + 128 * s2 + 64), pack8(s, s2), dVacc);
            if (ONEACC) dVacc = mfma32(tr_frag2(aq + 128 * s2, aq + 128 * s2 + 64), pack8(dp, s2), dVacc);
            else dKacc = mfma32(tr_frag2(aq + 128 * s2, aq + 128 * s2 + 64), pack8(dp, s2), dKacc);
        }
        if (more) stg.store(stage[(qt + 1) & 1]);
        __syncthreads();
    };
    if constexpr (CAUSAL) {
        // wave-uniform states, each a whole body: idle in front of the diagonal (staging and the barrier only; a wave without a key tile
        // stays there), the DIAG body on it, the full body behind it, the peeled query tail last.  No key tile is without queries.
        for (int qt = q0; qt < (live ? kt : nt); ++qt) {
            if (qt + 1 < nt) { stg.load(qt + 1); stg.store(stage[(qt + 1) & 1]); }
            __syncthreads();
        }
        if (live) {
            body(TileDiag{}, kt);                       // (on the last tile it is the query tail's body too)
            for (int qt = kt + 1; qt < nt - 1; ++qt) body(TileFull{}, qt);
            if (kt < nt - 1) { if (T & 31) body(TileTail{}, nt - 1); else body(TileFull{}, nt - 1); }
        }
    } else if constexpr (BAND) {
        // idle in front of the diagonal, the EDGE body from it to the wave's last query tile (it masks the query tail too), idle behind
        // it.  No key tile is without queries.
        auto idle = [&](int qt) {
            if (qt + 1 < nq) { stg.load(qt + 1); stg.store(stage[(qt + 1) & 1]); }
            __syncthreads();
        };
        int qt = q0;
        for (; qt < (live ? kt : nq); ++qt) idle(qt);
        if (live) {
            for (; qt <= qhi; ++qt) body(TileEdge{}, qt);
            __builtin_amdgcn_s_setprio(0);
            for (; qt < nq; ++qt) idle(qt);
        }
    } else {
        for (int qt = 0; qt < nt - 1; ++qt) body(TileFull{}, qt);
        if (T & 31) body(TileTail{}, nt - 1); else body(TileFull{}, nt - 1);
    }
    if (!live) return;
    // dK = ln2 * acc (scores are in the log2 domain), dV = acc; rows e = acc32_row, column key = r
    const float LN2 = 0.6931471805599453f;
    const int t = kt * 32 + r;
    if (t < T) {
        const size_t m = (size_t)b * T + t;
#pragma unroll
        for (int g = 0; g < DKB / 8; ++g) {
            bf16x4 kv, vv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kv[j] = (bf16)((ONEACC ? dVacc[8 + 4 * g + j] : dKacc[4 * g + j]) * LN2);      // ONEACC: rows 16 + e sit in registers 8..15
                vv[j] = (bf16)dVacc[4 * g + j];
            }
            const int e0 = head * DKP + 32 * fb + 8 * g + 4 * hh;
            *reinterpret_cast<bf16x4*>(dkv + m * lddkv + HD + e0) = kv;
            *reinterpret_cast<bf16x4*>(dkv + m * lddkv + 2 * HD + e0) = vv;
        }
    }
}
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, DKP == 16 ? 4 : 2) void attn_bwd_dkv_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr, const bf16* __restrict__ dOr,
        const float* __restrict__ lse, const float* __restrict__ delta,
        bf16* __restrict__ dkv, int lddkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskK, float drop_scale, int fb) {
    attn_bwd_dkv_body<DKP, DROP, ATTN_PLAIN>(Qr, Kr, Vr, dOr, lse, delta, dkv, lddkv, h, T, nt, nbh, maskK, drop_scale, fb, nullptr, 0);
}
// ... with key lengths: dK = dV = 0 for keys >= key_lengths[b]
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, DKP == 16 ? 4 : 2) void attn_bwd_dkv_keys_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr, const bf16* __restrict__ dOr,
        const float* __restrict__ lse, const float* __restrict__ delta,
        bf16* __restrict__ dkv, int lddkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskK, float drop_scale, int fb,
        const int* __restrict__ key_lengths) {
    attn_bwd_dkv_body<DKP, DROP, ATTN_KEYS>(Qr, Kr, Vr, dOr, lse, delta, dkv, lddkv, h, T, nt, nbh, maskK, drop_scale, fb, key_lengths, 0);
}
// ... causal: key t gets dK, dV from queries >= t
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, DKP == 16 ? 4 : 2) void attn_bwd_dkv_causal_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr, const bf16* __restrict__ dOr,
        const float* __restrict__ lse, const float* __restrict__ delta,
        bf16* __restrict__ dkv, int lddkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskK, float drop_scale, int fb) {
    attn_bwd_dkv_body<DKP, DROP, ATTN_CAUSAL>(Qr, Kr, Vr, dOr, lse, delta, dkv, lddkv, h, T, nt, nbh, maskK, drop_scale, fb, nullptr, 0);
}
// ... band: key t gets dK, dV from queries t .. t + span - 1
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, DKP == 16 ? 4 : 2) void attn_bwd_dkv_band_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr, const bf16* __restrict__ dOr,
        const float* __restrict__ lse, const float* __restrict__ delta,
        bf16* __restrict__ dkv, int lddkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskK, float drop_scale, int fb, int span) {
    attn_bwd_dkv_body<DKP, DROP, ATTN_BAND>(Qr, Kr, Vr, dOr, lse, delta, dkv, lddkv, h, T, nt, nbh, maskK, drop_scale, fb, nullptr, span);
}

// ------------------------------------------------------------------------------------------------
// Backward, part B: dQ.  Same orientation as the forward (query on the lane): wave w owns query tile
// qt = 4*blockIdx.x + w and sweeps all key tiles; L and delta are lane constants; the dS^T accumulator
// (keys in registers) is the B operand of dQ^T += K^T dS^T.  The epilogue applies 1/sqrt(d_k) and the
// query-row mask (blanked rows pass no gradient to Q) and writes columns [0,HD) of dQKV in both layouts.
template <int DKP, bool DROP, int MODE>
__device__ __forceinline__ void attn_bwd_dq_body(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        const bf16* __restrict__ dOr, const float* __restrict__ lse, const float* __restrict__ delta,
        const float* __restrict__ rowmask, float scale,
        bf16* __restrict__ dqkv, int lddqkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskQ, float drop_scale, int fb,
        const int* __restrict__ key_lengths, int span) {
    constexpr bool KEYS = MODE == ATTN_KEYS, CAUSAL = MODE == ATTN_CAUSAL, BAND = MODE == ATTN_BAND;
    constexpr int KS = DKP / 16;
    constexpr int DKB = DKP < 32 ? DKP : 32;
    constexpr int PR = DKP * 4, PRL = (DKP / 8) * MMT_TR_OCT;      // K tile padded in LDS: K^T fragments by transposing reads
    __shared__ __attribute__((aligned(16))) bf16 stage[2][(PRL + PR) * 8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const AttnBlock ab = CAUSAL ? attn_block_causal((nt + 3) >> 2, nbh) : attn_block((nt + 3) >> 2, nbh);
    if (!ab.valid) return;                              // whole workgroup, before any barrier
    const int qt = ab.bx * 4 + wave;
    const bool live = qt < nt;
    const int qtc = live ? qt : nt - 1;
    const int bh = ab.bh, b = bh / h, head = bh - b * h;
    const int Tp = nt * 32;
    const int Tk = KEYS ? attn_key_len(key_lengths, b, T) : T;          // keys that exist for this sequence, and their tiles
    const int nk = KEYS ? (Tk + 31) >> 5 : (CAUSAL || BAND) ? min(nt, ab.bx * 4 + 4) : nt;      // causal: up to the diagonal of the last query tile
    // band: the workgroup sweeps upwards from tile k0, this wave works in klo .. qt of them
    const int sp = BAND ? min(span, T) : 0;
    const int k0 = BAND ? band_lo_tile(ab.bx * 4, sp) : 0, klo = BAND ? band_lo_tile(qtc, sp) : 0;
    const int qrel = BAND ? min(qtc * 32 + r, T - 1) : 0;      // band: this lane's query, clamped (attn_fwd_body)
    const size_t offR = (size_t)bh * fragR_elems(Tp, DKP);
    const bf16 *Qrb = Qr + offR, *dOrb = dOr + offR;
    const uint16_t* mrow = maskQ + ((size_t)bh * nt + qtc) * nt * 64 + lane;      // LQ layout
    uint32_t mw = DROP ? mrow[BAND ? (size_t)klo * 64 : 0] : 0u;
    const uint32_t scale_bits = __builtin_bit_cast(uint32_t, drop_scale);

    TileStager<2, (2 * PR + MMT_THREADS - 1) / MMT_THREADS> stg;
    {
        const bf16* base[2] = {Kr + offR, Vr + offR};
        const int pieces[2] = {PR, PR}, strides[2] = {32 * DKP, 32 * DKP}, lds0[2] = {0, PRL}, pad[2] = {MMT_TR_OCT - 32, 0};
        stg.init(base, pieces, strides, lds0, pad, threadIdx.x);
    }
    stg.load(k0);
    // transposing-read role (see attn_fwd_kernel): feature row 32 fb + r of K^T; slot j <-> key 16 s2 + 8 (j >> 2) + 4 hh + (j & 3).
    // d_k = 16: the lanes of rows >= 16 (nobody reads their dQ^T rows) fetch what lanes r - 16 fetch.
    const int g1 = (lane >> 4) & 1, tq = (lane >> 2) & 3, tpp = lane & 3;
    const int toff = (((DKP == 16 ? 0 : 4 * fb + 2 * g1) + (tpp >> 1)) * MMT_TR_OCT + 4 * hh + tq) * 8 + 4 * (tpp & 1);
    bf16x8 qf[KS], dof[KS];
#pragma unroll
    for (int ss = 0; ss < KS; ++ss) {
        const size_t off = ((size_t)(qtc * (DKP / 8) + 2 * ss + hh) * 32 + r) * 8;
        qf[ss] = *reinterpret_cast<const bf16x8*>(Qrb + off);
        dof[ss] = *reinterpret_cast<const bf16x8*>(dOrb + off);
    }
    const float negL = lse[(size_t)bh * Tp + qtc * 32 + r];          // both stored negated by their producers
    const float negD = delta[(size_t)bh * Tp + qtc * 32 + r];
    f32x16 dq;
#pragma unroll
    for (int j = 0; j < 16; ++j) dq[j] = 0.f;
    stg.store(stage[k0 & 1]);
    __syncthreads();

    // Tile body without conditional code between MFMAs and their consumers (see attn_fwd_kernel); key tail peeled.
    auto body = [&](auto tile_tag, int kt) {
        constexpr bool TAIL = (int)decltype(tile_tag)::value == 1, DIAG = (int)decltype(tile_tag)::value == 2;
        constexpr bool EDGE = (int)decltype(tile_tag)::value == 3;
        const bool more = kt + 1 < nk;
        progress_prio(BAND ? kt - klo : kt, BAND ? qt - klo + 1 : nk);
        const uint32_t tw = mw;
        if (BAND) { if (DROP && kt < qt) mw = mrow[(size_t)(kt + 1) * 64]; }
        else if (DROP && more && !DIAG) mw = mrow[(size_t)(kt + 1) * 64];
        if (more) stg.load(kt + 1);
        const bf16* sk = stage[kt & 1];
        const bf16* sv = sk + PRL * 8;
        const bf16* skt = sk + toff;
        f32x16 s, dp;
        fill16(s, negL);
        if (DROP) {                                     // -delta enters after the mask
#pragma unroll
            for (int j = 0; j < 16; ++j) dp[j] = 0.f;
        } else fill16(dp, negD);
#pragma unroll
        for (int ss = 0; ss < KS; ++ss) {
            const int o8 = ((2 * ss + hh) * 32 + r) * 8;
            s = mfma32(*reinterpret_cast<const bf16x8*>(sk + o8 + (2 * ss + hh) * (MMT_TR_OCT - 32) * 8), qf[ss], s);
            dp = mfma32(*reinterpret_cast<const bf16x8*>(sv + o8), dof[ss], dp);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float pv = fast_exp2(s[j]);
            if (TAIL) pv = (kt * 32 + acc32_row(j, hh) < Tk) ? pv : 0.f;      // keys >= T (>= the key length) do not exist
            // kt == qt: neither do keys behind the query (a select: L is from the visible keys, 2^(S' - L) of a later key may be inf)
            if (DIAG) pv = (acc32_row(j, hh) <= r && kt * 32 + acc32_row(j, hh) < T) ? pv : 0.f;
            // band: only keys query-span+1 .. query exist (a select, for the same reason)
            if (EDGE) pv = ((unsigned)(qrel - kt * 32 - acc32_row(j, hh)) < (unsigned)sp) ? pv : 0.f;
            s[j] = pv;
        }
        if (DROP) {
            // dS = P * ((dO V^T) * m/(1-p) - delta)
            static_for<0, 16>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                dp[j] = s[j] * fmaf(dp[j], __builtin_bit_cast(float, scale_bits & keep_bits<j>(tw)), negD);
            });
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) dp[j] *= s[j];
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
            dq = mfma32(tr_frag2(skt + 128 * s2, skt + 128 * s2 + 64), pack8(dp, s2), dq);
        if (more) stg.store(stage[(kt + 1) & 1]);
        __syncthreads();
    };
    if constexpr (CAUSAL) {                             // the three wave-uniform states of attn_fwd_body
        for (int kt = 0; kt < (live ? qt : 0); ++kt) body(TileFull{}, kt);
        if (live) body(TileDiag{}, qt);
        __builtin_amdgcn_s_setprio(0);
        for (int kt = live ? qt + 1 : 0; kt < nk; ++kt) {
            if (kt + 1 < nk) { stg.load(kt + 1); stg.store(stage[(kt + 1) & 1]); }
            __syncthreads();
        }
    } else if constexpr (BAND) {
        // idle below the wave's lowest tile, the EDGE body from it to the diagonal, idle above
        auto idle = [&](int kt) {
            if (kt + 1 < nk) { stg.load(kt + 1); stg.store(stage[(kt + 1) & 1]); }
            __syncthreads();
        };
        int kt = k0;
        for (; kt < (live ? klo : nk); ++kt) idle(kt);
        if (live) {
            for (; kt <= qt; ++kt) body(TileEdge{}, kt);
            __builtin_amdgcn_s_setprio(0);
            for (; kt < nk; ++kt) idle(kt);
        }
    } else {
        for (int kt = 0; kt < nk - 1; ++kt) body(TileFull{}, kt);
        if (Tk & 31) body(TileTail{}, nk - 1); else body(TileFull{}, nk - 1);
    }
    if (!live) return;
    const int t = qt * 32 + r;
    if (t < T) {
        const size_t m = (size_t)b * T + t;
        const float sc = (rowmask && rowmask[m] == 0.0f) ? 0.f : scale;     // blanked query rows pass no gradient to Q
#pragma unroll
        for (int g = 0; g < DKB / 8; ++g) {
            bf16x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (bf16)(dq[4 * g + j] * sc);
            const int e0 = head * DKP + 32 * fb + 8 * g + 4 * hh;
            *reinterpret_cast<bf16x4*>(dqkv + m * lddqkv + e0) = v;
        }
    }
}
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_bwd_dq_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        const bf16* __restrict__ dOr, const float* __restrict__ lse, const float* __restrict__ delta,
        const float* __restrict__ rowmask, float scale,
        bf16* __restrict__ dqkv, int lddqkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskQ, float drop_scale, int fb) {
    attn_bwd_dq_body<DKP, DROP, ATTN_PLAIN>(Qr, Kr, Vr, dOr, lse, delta, rowmask, scale, dqkv, lddqkv, h, T, nt, nbh, maskQ, drop_scale, fb, nullptr, 0);
}
// ... with key lengths: the sweep ends at key_lengths[b]
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_bwd_dq_keys_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        const bf16* __restrict__ dOr, const float* __restrict__ lse, const float* __restrict__ delta,
        const float* __restrict__ rowmask, float scale,
        bf16* __restrict__ dqkv, int lddqkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskQ, float drop_scale, int fb,
        const int* __restrict__ key_lengths) {
    attn_bwd_dq_body<DKP, DROP, ATTN_KEYS>(Qr, Kr, Vr, dOr, lse, delta, rowmask, scale, dqkv, lddqkv, h, T, nt, nbh, maskQ, drop_scale, fb, key_lengths, 0);
}
// ... causal: the sweep of a query tile ends at its diagonal
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_bwd_dq_causal_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        const bf16* __restrict__ dOr, const float* __restrict__ lse, const float* __restrict__ delta,
        const float* __restrict__ rowmask, float scale,
        bf16* __restrict__ dqkv, int lddqkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskQ, float drop_scale, int fb) {
    attn_bwd_dq_body<DKP, DROP, ATTN_CAUSAL>(Qr, Kr, Vr, dOr, lse, delta, rowmask, scale, dqkv, lddqkv, h, T, nt, nbh, maskQ, drop_scale, fb, nullptr, 0);
}
// ... band: the sweep of a query tile runs from its far edge to its diagonal
template <int DKP, bool DROP>
__global__ __launch_bounds__(MMT_THREADS, 2) void attn_bwd_dq_band_kernel(
        const bf16* __restrict__ Qr, const bf16* __restrict__ Kr, const bf16* __restrict__ Vr,
        const bf16* __restrict__ dOr, const float* __restrict__ lse, const float* __restrict__ delta,
        const float* __restrict__ rowmask, float scale,
        bf16* __restrict__ dqkv, int lddqkv,
        int h, int T, int nt, int nbh, const uint16_t* __restrict__ maskQ, float drop_scale, int fb, int span) {
    attn_bwd_dq_body<DKP, DROP, ATTN_BAND>(Qr, Kr, Vr, dOr, lse, delta, rowmask, scale, dqkv, lddqkv, h, T, nt, nbh, maskQ, drop_scale, fb, nullptr, span);
}

// ------------------------------------------------------------------------------------------------
// Key lengths from a mask (B, T): len[b] = 1 + index of the last non-zero entry of row b, 1 for an all-zero row.  One workgroup per
// sequence; a prefix mask (what padding produces) gives its length, holes inside the prefix stay attended.
__global__ __launch_bounds__(MMT_THREADS) void key_lengths_kernel(const float* __restrict__ mask, int* __restrict__ out, int T) {
    __shared__ int part[MMT_THREADS / 64];
    const float* row = mask + (size_t)blockIdx.x * T;
    int last = 0;                                       // 1 + index, 0: none seen
    for (int t = threadIdx.x; t < T; t += MMT_THREADS) if (row[t] != 0.0f) last = t + 1;      // ascending t: the thread's last hit stays
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) last = max(last, __shfl_xor(last, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = last;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = part[0];
#pragma unroll
        for (int w = 1; w < MMT_THREADS / 64; ++w) m = max(m, part[w]);
        out[blockIdx.x] = max(m, 1);
    }
}
