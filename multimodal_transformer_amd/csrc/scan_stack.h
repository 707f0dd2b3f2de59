// Stacked LSTM scan: L = 2..4 coupled layers with the top layer's output fed back into layer 0, the autoregressive decoder of the SFT /
// single-modality models built with n_layers > 1 (nn.LSTM(2d, d, L) called one step at a time on [o_{t-1} ; enc_t],
// transformer/SFT/multiTransformer.py:444-446,463-483; transformer/MFT/multiTransformer.py:335-337,357-376).  With H = d:
//
//   o_{-1} = 0,  h^l_{-1} = h0[l],  c^l_{-1} = c0[l]
//   g^0_t = gx0_t + [o_{t-1} ; h^0_{t-1}] P_0^T                 gx0 = enc W_ih_l0[:, d:]^T + b_0: one batched GEMM before the scan
//   g^l_t = b_l   + [h^{l-1}_t ; h^l_{t-1}] P_l^T               l = 1 .. L-1
//   (h^l_t, c^l_t) = cell(g^l_t, c^l_{t-1}),   o_t = h^{L-1}_t
//
// so every layer-step is one product [x_a ; x_b] (1 x 2H) . P_l^T with a packed P_l (4H, 2H):  P_0 = [W_ih_l0[:, :d] | W_hh_l0],
// P_l = [W_ih_l | W_hh_l].  The layers are coupled inside every step (o_{t-1} enters layer 0), so this cannot be one scan per layer.
//
// The kernels are scan_units.h's form — one or two sequences per workgroup, one hidden unit per lane, the state rows as the MFMA A
// operand, mfma_f32_16x16x32_bf16, bf16 state tiles in LDS, c in fp32 registers, one LDS barrier per layer-step — with
//   * an A operand of two LDS tiles: k-blocks 0..KS-1 read x_a, KS..2KS-1 read x_b;
//   * one double-buffered h tile per layer (h^l_t in tile [l][t & 1]) and a tile of zeros that stands for o_{-1} at step 0, where the
//     top layer's own tile holds h0[L-1]: from step 1 on o_{t-1} IS the top layer's tile of step t-1;
//   * c per layer, the biases of layers >= 1 in registers, the gx0 ring of scan_units.h unchanged;
//   * weights streamed from L2 every layer-step (two k-blocks in flight behind scheduling fences), as scan_units.h does at HPAD = 256:
//     a layer set is L x 4 HP16 x 2 HPAD bf16 (1 MB at L = 4, H = 128) and does not fit the registers.
// One workgroup owns its sequences for the whole scan: no exchange between workgroups, no wait, no error word.
// Limits (scan_stack_plan.h): 2 <= L <= 4, H % 4 == 0, H <= 128 (K = 2 HPAD <= 256), B <= 512.  Gate order i, f, g, o.
#pragma once
#include "scan_common.h"

// P (L, 4H, 2H) fp32 -> forward fragments Pf [L][4][HP16][2 HPAD] (row = gate unit, k = x_a unit | HPAD + x_b unit) and backward
// fragments Pb [L][2][HP16][4 HPAD] (row = unit of x_a / x_b, k = gate * HPAD + gate unit), bf16, pads zero.
__global__ void lstm_stack_prep_kernel(const float* __restrict__ P, bf16* __restrict__ Pf, bf16* __restrict__ Pb,
                                       int H, int HP16, int HPAD, int L) {
    const size_t nfl = (size_t)4 * HP16 * 2 * HPAD, nbl = (size_t)2 * HP16 * 4 * HPAD;
    const size_t nf = nfl * L, nb = nbl * L;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < nf + nb; idx += (size_t)gridDim.x * blockDim.x) {
        if (idx < nf) {
            const int l = (int)(idx / nfl);
            const size_t i = idx - (size_t)l * nfl;
            const int k2 = (int)(i % (2 * HPAD)), j = (int)((i / (2 * HPAD)) % HP16), q = (int)(i / ((size_t)2 * HPAD * HP16));
            const int half = k2 / HPAD, k = k2 - half * HPAD;
            Pf[idx] = (bf16)((j < H && k < H) ? P[(((size_t)l * 4 + q) * H + j) * 2 * H + (size_t)half * H + k] : 0.f);
        } else {
            const size_t ib = idx - nf;
            const int l = (int)(ib / nbl);
            const size_t i = ib - (size_t)l * nbl;
            const int c = (int)(i % (4 * HPAD)), j = (int)((i / (4 * HPAD)) % HP16), half = (int)(i / ((size_t)4 * HPAD * HP16));
            const int q = c / HPAD, jp = c - q * HPAD;
            Pb[ib] = (bf16)((j < H && jp < H) ? P[(((size_t)l * 4 + q) * H + jp) * 2 * H + (size_t)half * H + j] : 0.f);
        }
    }
}

// grid = ceil(B / NR); block = 64 * (HP16/16) <= NT.  HPAD = 32 KS.  Outputs h_all, c_all (L,T,B,H) and acts (L,T,B,4H).
template <int KS, int NT, int PF, int NR, int L>
__global__ __launch_bounds__(NT) void lstm_stack_fwd_kernel(const float* __restrict__ gx0, const bf16* __restrict__ Pf,
                                     const float* __restrict__ bias, const float* __restrict__ h0, const float* __restrict__ c0,
                                     float* __restrict__ h_all, float* __restrict__ c_all, float* __restrict__ acts,
                                     int T, int B, int H, int HP16) {
    constexpr int HPAD = 32 * KS, KP2 = 2 * HPAD, ldh = HPAD + 8, TILE = 16 * ldh;
    __shared__ __attribute__((aligned(16))) bf16 hbuf[(2 * L + 1) * TILE];      // [layer][t & 1][16 rows: sequence r in row r][ldh], then zeros
    const bf16* const zeros = hbuf + 2 * L * TILE;
    const int lane = threadIdx.x & 63, jt = threadIdx.x >> 6, l15 = lane & 15, lq = lane >> 4;
    const int bd0 = blockIdx.x * NR;
    const int nb = (B - bd0) < NR ? (B - bd0) : NR;
    const int ud = jt * 16 + l15, udc = ud < H ? ud : H - 1;
    const bool ulive = (lq == 0) && (ud < H);
    const unsigned uo[4] = {4u * (unsigned)ud, 4u * (unsigned)(ud + H), 4u * (unsigned)(ud + 2 * H), 4u * (unsigned)(ud + 3 * H)};   // byte offsets

    // B fragments: column = unit jt*16 + l15, 8 consecutive k per lane quarter
    const bf16* wrow = Pf + (size_t)(jt * 16 + l15) * KP2 + 8 * lq;     // + l*wl + q*wq + ks*32
    const size_t wq = (size_t)HP16 * KP2, wl = 4 * wq;
    const size_t lstride = (size_t)T * B * H;                           // one layer of h_all / c_all
    lds_clear(hbuf, (2 * L + 1) * TILE);
    float cd[L][NR], bl[L][4];
#pragma unroll
    for (int l = 0; l < L; ++l) {
#pragma unroll
        for (int q = 0; q < 4; ++q) bl[l][q] = l ? bias[(size_t)(l - 1) * 4 * H + (size_t)q * H + udc] : 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            cd[l][r] = 0.f;
            if (ulive && r < nb) {
                const size_t o = ((size_t)l * B + bd0 + r) * H + ud;
                if (c0) cd[l][r] = c0[o];
                if (h0) hbuf[(2 * l + 1) * TILE + r * ldh + ud] = (bf16)h0[o];      // h_{-1} sits where h_1 will
            }
        }
    }
    __syncthreads();

    // this lane's layer-0 gate inputs of the next PF steps (scan_units.h)
    const size_t gstep = (size_t)B * 4 * H;
    const float* gxl = gx0 + (size_t)bd0 * 4 * H + udc;
    struct In { float g[NR][4]; };
    In ring[PF];
    size_t foff = 0;                                            // float offset of the next step to fetch; stops at the last step
    int tf = 0;
    const size_t r1 = (size_t)(nb > 1 ? 1 : 0) * 4 * H;
    auto fetch = [&](In& q) {
        const float* p = gxl + foff;
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) q.g[r][g] = p[(r ? r1 : 0) + (size_t)g * H];
        foff += (tf < T - 1) ? gstep : 0;                       // the tail re-reads the last step (unused)
        ++tf;
    };
#pragma unroll
    for (int d = 0; d < PF; ++d) fetch(ring[d]);
    size_t soff = (size_t)bd0 * H;                              // float offset of (step t, sequence bd0) inside a layer of h_all / c_all
    int cur = 0;                                                // t & 1
    auto step = [&](int t, In& slot) {
        const In in = slot;
        fetch(slot);
#pragma unroll
        for (int l = 0; l < L; ++l) {
            // x_a: o_{t-1} (layer 0; zeros at step 0) or the layer below at this step; x_b: this layer's own previous state
            const bf16* xa = l == 0 ? (t == 0 ? zeros : hbuf + (2 * (L - 1) + (cur ^ 1)) * TILE) : hbuf + (2 * (l - 1) + cur) * TILE;
            const bf16* xb = hbuf + (2 * l + (cur ^ 1)) * TILE;
            const bf16* pa = xa + l15 * ldh + 8 * lq;           // A fragments: row l15 = sequence l15
            const bf16* pb = xb + l15 * ldh + 8 * lq;
            const bf16* wr = wrow + l * wl;
            // the fragment addresses do not change from step to step, and hipcc would otherwise keep the first k-blocks of EVERY layer in
            // registers across the time loop (32 VGPRs per layer and k-block pair: spills at HPAD = 128).  An address it cannot see through
            // keeps each layer-step's loads inside the layer-step.
            asm volatile("" : "+v"(wr));
            f32x4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            // streamed weights: two k-blocks of fragments in flight; the scheduling fences keep hipcc from hoisting every fragment
            // load of the layer-step to its top
            bf16x8 wa[2][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) wa[0][q] = *reinterpret_cast<const bf16x8*>(wr + q * wq);
#pragma unroll
            for (int ks = 0; ks < 2 * KS; ++ks) {
                if (ks + 1 < 2 * KS) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) wa[(ks + 1) & 1][q] = *reinterpret_cast<const bf16x8*>(wr + q * wq + (ks + 1) * 32);
                }
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(ks < KS ? pa + ks * 32 : pb + (ks - KS) * 32);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = mfma16(af, wa[ks & 1][q], acc[q]);
                __builtin_amdgcn_sched_barrier(0);
            }
            float ig[NR], fg[NR], gg[NR], og[NR], hn[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float x0 = l == 0 ? in.g[r][0] : bl[l][0], x1 = l == 0 ? in.g[r][1] : bl[l][1];
                const float x2 = l == 0 ? in.g[r][2] : bl[l][2], x3 = l == 0 ? in.g[r][3] : bl[l][3];
                ig[r] = sigmoid_f(acc[0][r] + x0); fg[r] = sigmoid_f(acc[1][r] + x1);
                gg[r] = tanh_f(acc[2][r] + x2); og[r] = sigmoid_f(acc[3][r] + x3);
                cd[l][r] = fg[r] * cd[l][r] + ig[r] * gg[r];
                hn[r] = og[r] * tanh_f(cd[l][r]);
                // rows >= nb and units >= H of every h tile stay 0 (never written)
                if (ulive && r < nb) hbuf[(2 * l + cur) * TILE + r * ldh + ud] = (bf16)hn[r];
            }
            lds_barrier();                                      // h^l_t visible to every wave; global traffic stays in flight
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (ulive && r < nb) {
                    const size_t o = (size_t)l * lstride + soff + (size_t)r * H;
                    st_uniform(h_all + o, uo[0], hn[r]);
                    st_uniform(c_all + o, uo[0], cd[l][r]);
                    float* ap = acts + o * 4;
                    st_uniform(ap, uo[0], ig[r]); st_uniform(ap, uo[1], fg[r]); st_uniform(ap, uo[2], gg[r]); st_uniform(ap, uo[3], og[r]);
                }
        }
        soff += (size_t)B * H;
        cur ^= 1;
    };
    int t0 = 0;
    for (; t0 + PF <= T; t0 += PF) {
#pragma unroll
        for (int d = 0; d < PF; ++d) step(t0 + d, ring[d]);
    }
#pragma unroll
    for (int d = 0; d < PF; ++d) if (t0 + d < T) step(t0 + d, ring[d]);
}

// Backward through time, t = T-1 .. 0 and inside a step l = L-1 .. 0.  dh^l_t is the sum of the external gradient (top layer only:
// dh_top (T,B,H) or null), the x_a half of layer l+1's product at step t, the x_b half of layer l's product at step t+1 and, for the
// top layer, the x_a half of layer 0's product at step t+1 (the o feedback).  Then the cell backward (scan_common.h), dG^l_t stored to
// dG (L,T,B,4H) — also the operand of the batched weight gradients — and [dx_a ; dx_b] = dG^l_t . P_l, a 4H -> 2H product: both halves
// share the gate-gradient A fragments.  The o feedback gradient of step 0 is dropped (o_{-1} is a constant).  KS4 = 4 HPAD / 32.
// The saved activations of the NEXT layer-step are fetched under the MFMAs of this one.
template <int KS4, int NT, int NR, int L>
__global__ __launch_bounds__(NT) void lstm_stack_bwd_kernel(const float* __restrict__ dh_top, const bf16* __restrict__ Pb,
                                     const float* __restrict__ c0, const float* __restrict__ c_all, const float* __restrict__ acts,
                                     float* __restrict__ dG, float* __restrict__ dh0, float* __restrict__ dc0,
                                     int T, int B, int H, int HP16) {
    constexpr int KP4 = 32 * KS4, HPAD = KP4 / 4, ldg = KP4 + 8;
    __shared__ __attribute__((aligned(16))) bf16 gbuf[2 * 16 * ldg];    // [2][16 rows: sequence r in row r][ldg]: k = gate*HPAD + unit
    const int lane = threadIdx.x & 63, jt = threadIdx.x >> 6, l15 = lane & 15, lq = lane >> 4;
    const int bd0 = blockIdx.x * NR;
    const int nb = (B - bd0) < NR ? (B - bd0) : NR;
    const int ud = jt * 16 + l15, udc = ud < H ? ud : H - 1;
    const bool ulive = (lq == 0) && (ud < H);
    const unsigned uo[4] = {4u * (unsigned)ud, 4u * (unsigned)(ud + H), 4u * (unsigned)(ud + 2 * H), 4u * (unsigned)(ud + 3 * H)};   // byte offsets

    const bf16* wrow = Pb + (size_t)(jt * 16 + l15) * KP4 + 8 * lq;     // B fragments: column = unit jt*16 + l15 of dx_a / dx_b
    const size_t wh = (size_t)HP16 * KP4;                               // + (2 l + half) * wh + ks * 32
    lds_clear(gbuf, 2 * 16 * ldg);

    const size_t ostep = (size_t)B * H, lstride = (size_t)T * ostep;
    size_t bo[NR];                                                      // (sequence, unit) offset inside a step; dead rows read row 0
#pragma unroll
    for (int r = 0; r < NR; ++r) bo[r] = (size_t)(bd0 + (r < nb ? r : 0)) * H + udc;
    const float* const dhp = dh_top ? dh_top : c_all;                   // an absent gradient reads a valid dummy, scaled by 0
    const float dhs = dh_top ? 1.f : 0.f;
    struct In { float ig[NR], fg[NR], gg[NR], og[NR], ct[NR], cp[NR], dhe[NR]; };
    auto fetch = [&](int l, int t) {
        In q;
        const size_t so = (size_t)l * lstride + (size_t)t * ostep;      // (layer l, step t)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float* ap = acts + (so + bo[r] - udc) * 4 + udc;
            q.ig[r] = ap[0]; q.fg[r] = ap[H]; q.gg[r] = ap[2 * H]; q.og[r] = ap[3 * H];
            q.ct[r] = c_all[so + bo[r]];
            const float cprev = c_all[so - (t > 0 ? ostep : 0) + bo[r]];
            const float cinit = c0 ? c0[(size_t)l * ostep + bo[r]] : 0.f;       // c_{-1} = c0[l]
            q.cp[r] = t > 0 ? cprev : cinit;
            q.dhe[r] = dhp[(size_t)t * ostep + bo[r]] * dhs;
        }
        return q;
    };
    float dxb[L][NR], dcd[L][NR], dxa0[NR], dxau[NR];                   // carried: x_b halves and dc per layer, layer 0's x_a half; within a step: the layer above's x_a half
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        dxa0[r] = 0.f; dxau[r] = 0.f;
#pragma unroll
        for (int l = 0; l < L; ++l) { dxb[l][r] = 0.f; dcd[l][r] = 0.f; }
    }
    In nxt = fetch(L - 1, T - 1);
    int cur = 0;
    for (int t = T - 1; t >= 0; --t) {
#pragma unroll
        for (int l = L - 1; l >= 0; --l) {
            const In in = nxt;
            {   // the layer-step after this one: (l-1, t), or (L-1, t-1); past the end re-reads step 0 (unused)
                const int tn = l > 0 ? t : (t > 0 ? t - 1 : 0);
                nxt = fetch(l > 0 ? l - 1 : L - 1, tn);
            }
            float dgi[NR], dgf[NR], dgg[NR], dgo[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const bool lived = ulive && r < nb;
                const float dh = dxb[l][r] + (l == L - 1 ? dxa0[r] : dxau[r]);
                lstm_cell_bwd(lived, in.ig[r], in.fg[r], in.gg[r], in.og[r], in.ct[r], in.cp[r], dh, l == L - 1 ? in.dhe[r] : 0.f, 0.f,
                              dcd[l][r], dgi[r], dgf[r], dgg[r], dgo[r]);
                // rows >= nb and pad units of the gradient tile stay 0 (never written)
                if (lived) {
                    bf16* gw = gbuf + cur * 16 * ldg + r * ldg + ud;
                    gw[0] = (bf16)dgi[r]; gw[HPAD] = (bf16)dgf[r]; gw[2 * HPAD] = (bf16)dgg[r]; gw[3 * HPAD] = (bf16)dgo[r];
                }
            }
            lds_barrier();
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (ulive && r < nb) {
                    float* gp = dG + (((size_t)l * T + t) * B + bd0 + r) * 4 * H;
                    st_uniform(gp, uo[0], dgi[r]); st_uniform(gp, uo[1], dgf[r]); st_uniform(gp, uo[2], dgg[r]); st_uniform(gp, uo[3], dgo[r]);
                }
            const bf16* gb = gbuf + cur * 16 * ldg + l15 * ldg + 8 * lq;        // A fragments: row l15 = sequence l15 (rows >= nb are zero)
            const bf16* wa = wrow + (size_t)(2 * l) * wh;
            const bf16* wb = wa + wh;
            // two independent accumulation chains per half: one chain of KS4 dependent MFMAs would serialise on the accumulator latency
            f32x4 acc[2][2] = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}};
            constexpr int KG = 4;                                       // k-blocks per group: 4 A + 8 weight fragments in flight
#pragma unroll
            for (int k0 = 0; k0 < KS4; k0 += KG) {
                bf16x8 afr[KG], wfa[KG], wfb[KG];
#pragma unroll
                for (int ks = 0; ks < KG; ++ks) {
                    afr[ks] = *reinterpret_cast<const bf16x8*>(gb + (k0 + ks) * 32);
                    wfa[ks] = *reinterpret_cast<const bf16x8*>(wa + (k0 + ks) * 32);
                    wfb[ks] = *reinterpret_cast<const bf16x8*>(wb + (k0 + ks) * 32);
                }
#pragma unroll
                for (int ks = 0; ks < KG; ++ks) {
                    acc[0][ks & 1] = mfma16(afr[ks], wfa[ks], acc[0][ks & 1]);
                    acc[1][ks & 1] = mfma16(afr[ks], wfb[ks], acc[1][ks & 1]);
                }
                __builtin_amdgcn_sched_barrier(0);                      // keep the next group's fragment loads below this point
            }
            const f32x4 da = acc[0][0] + acc[0][1], db = acc[1][0] + acc[1][1];
#pragma unroll
            for (int r = 0; r < NR; ++r) {                              // sequence r, this lane's unit (lanes lq == 0)
                dxb[l][r] = db[r];
                if (l == 0) dxa0[r] = da[r]; else dxau[r] = da[r];
            }
            cur ^= 1;
        }
    }
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (ulive && r < nb) {
                const size_t o = ((size_t)l * B + bd0 + r) * H + ud;
                if (dh0) dh0[o] = dxb[l][r];
                if (dc0) dc0[o] = dcd[l][r];
            }
}
