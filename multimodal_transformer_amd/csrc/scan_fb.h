// LSTM scan with the read-out MLP inside the recurrence: the decoder of the encoder-decoder LSTM (MultiEDLSTM,
// transformer/MFT/models.py:290-305; nn.LSTM(1 + H, H) called one step at a time on [p_{t-1} ; ctx_t], p_t = out(h_t)):
//
//   p_{-1} = p_init,  h_{-1} = h0,  c_{-1} = c0
//   gates_t = gxc_t + p_{t-1} w_p + h_{t-1} W_hh^T         gxc = ctx W_ih[:, 1:]^T + b_ih + b_hh: one batched GEMM before the scan
//   (h_t, c_t) = cell(gates_t, c_{t-1})                    w_p = W_ih[:, 0]
//   u_t = ReLU(W1 h_t + b1)   (E)                          W1 = out.0.weight (E,H)
//   p_t = w2 . u_t + b2       scalar per sequence          w2 = out.2.weight[0]
//
// The value fed back passes through a non-linear read-out of h, so neither lstm_scan (h fed back) nor lstm_stack_scan expresses it.
//
// The kernels are scan_units.h's form — one or two sequences per workgroup, one hidden unit per lane, the state rows as the MFMA A
// operand, mfma_f32_16x16x32_bf16, the bf16 h tile in LDS, c in fp32 registers, W_hh fragments resident in registers, the gxc ring in
// registers — with
//   * the rows of W1 as further 16-row B tiles dealt to the waves (tile s of wave w: rows (s NW + w) 16 ..): the product that reads
//     h_{t-1} for the gates of step t also yields W1 h_{t-1};
//   * p_{t-1}: every wave reduces w2 . u over its rows (fp32, a fixed butterfly over the 16 lanes), the partial sums go to LDS, and every
//     lane adds them in wave order: reruns are bit-identical.  This is a second barrier in the step;
//   * p, w_p, b1, w2, b2 and every sum in fp32; only the MFMA operands (h, W_hh, W1; backward: dG, du) are bf16.
// One workgroup owns its sequences for the whole scan: no exchange between workgroups, no wait, no error word.
// Limits (scan_fb_plan.h): H, E multiples of 4 in [4,128], B <= 512.  Gate order i, f, g, o.
#pragma once
#include "scan_common.h"

// W_hh (4H,H), W1 (E,H) fp32 -> the four bf16 fragment sets of scan_fb_plan.h, pads zero
__global__ void lstm_fb_prep_kernel(const float* __restrict__ Whh, const float* __restrict__ W1, bf16* __restrict__ Wf, bf16* __restrict__ Wb,
                                    bf16* __restrict__ W1f, bf16* __restrict__ W1b, int H, int E, int HP16, int HPAD, int ER, int EK) {
    const size_t nf = (size_t)4 * HP16 * HPAD, nb = (size_t)HP16 * 4 * HPAD, n1f = (size_t)ER * HPAD, n1b = (size_t)HP16 * EK;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < nf + nb + n1f + n1b; idx += (size_t)gridDim.x * blockDim.x) {
        if (idx < nf) {
            const int k = (int)(idx % HPAD), j = (int)((idx / HPAD) % HP16), q = (int)(idx / ((size_t)HPAD * HP16));
            Wf[idx] = (bf16)((j < H && k < H) ? Whh[((size_t)q * H + j) * H + k] : 0.f);
        } else if (idx < nf + nb) {
            const size_t i = idx - nf;
            const int c = (int)(i % (4 * HPAD)), j = (int)(i / (4 * HPAD));
            const int q = c / HPAD, jp = c - q * HPAD;
            Wb[i] = (bf16)((j < H && jp < H) ? Whh[((size_t)q * H + jp) * H + j] : 0.f);
        } else if (idx < nf + nb + n1f) {
            const size_t i = idx - nf - nb;
            const int k = (int)(i % HPAD), e = (int)(i / HPAD);
            W1f[i] = (bf16)((e < E && k < H) ? W1[(size_t)e * H + k] : 0.f);
        } else {
            const size_t i = idx - nf - nb - n1f;
            const int e = (int)(i % EK), j = (int)(i / EK);
            W1b[i] = (bf16)((j < H && e < E) ? W1[(size_t)e * H + j] : 0.f);
        }
    }
}

// sum over the 16 lanes that share lane >> 4, in a fixed order
__device__ __forceinline__ float fb_sum16(float v) {
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    return v;
}

// grid = ceil(B / NR); block = 64 * (HP16/16) <= NT.  HPAD = 32 KS.  ES: MLP row tiles per wave.
// Outputs h_all, c_all (T,B,H), acts (T,B,4H), u_all (T,B,E), p_all (T+1,B): row 0 holds p_init, row t + 1 holds p_t.
template <int KS, int NT, int PF, int NR, int ES>
__global__ __launch_bounds__(NT) void lstm_fb_scan_fwd_kernel(const float* __restrict__ gxc, const bf16* __restrict__ Wf, const bf16* __restrict__ W1f,
                                     const float* __restrict__ w_p, const float* __restrict__ b1, const float* __restrict__ w2,
                                     const float* __restrict__ b2, const float* __restrict__ h0, const float* __restrict__ c0, float p_init,
                                     float* __restrict__ h_all, float* __restrict__ c_all, float* __restrict__ acts,
                                     float* __restrict__ u_all, float* __restrict__ p_all, int T, int B, int H, int E, int HP16) {
    constexpr int KP = 32 * KS, ldh = KP + 8;
    __shared__ __attribute__((aligned(16))) bf16 hbuf[2 * 16 * ldh];            // [2][16 rows: sequence r in row r, the others zero][ldh]
    __shared__ float pbuf[2][8 * NR];                                           // [step parity][wave][sequence]: partial sums of w2 . u
    const int lane = threadIdx.x & 63, jt = threadIdx.x >> 6, l15 = lane & 15, lq = lane >> 4, NW = blockDim.x >> 6;
    const int bd0 = blockIdx.x * NR;
    const int nb = (B - bd0) < NR ? (B - bd0) : NR;
    const int ud = jt * 16 + l15, udc = ud < H ? ud : H - 1;
    const bool ulive = (lq == 0) && (ud < H);
    const unsigned uo[4] = {4u * (unsigned)ud, 4u * (unsigned)(ud + H), 4u * (unsigned)(ud + 2 * H), 4u * (unsigned)(ud + 3 * H)};   // byte offsets

    // B fragments: column = unit jt*16 + l15 (W_hh) / MLP row er[s] (W1), 8 consecutive k per lane quarter
    const bf16* wrow = Wf + (size_t)(jt * 16 + l15) * KP + 8 * lq;      // + q*HP16*KP + ks*32
    const size_t wq = (size_t)HP16 * KP;
    bf16x8 a[4][KS], w1[ES][KS];
#pragma unroll
    for (int q = 0; q < 4; ++q) load_wfrags(a[q], wrow + q * wq);
    int er[ES];
    float b1v[ES], w2v[ES], wpv[4];
#pragma unroll
    for (int s = 0; s < ES; ++s) {
        er[s] = (s * NW + jt) * 16 + l15;                               // < ER = 16 ES NW; rows >= E are zero fragments with b1 = w2 = 0
        load_wfrags(w1[s], W1f + (size_t)er[s] * KP + 8 * lq);
        b1v[s] = er[s] < E ? b1[er[s]] : 0.f;
        w2v[s] = er[s] < E ? w2[er[s]] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) wpv[q] = w_p[(size_t)q * H + udc];
    const float b2v = b2[0];
    lds_zero(hbuf, 2 * 16 * ldh);
    __syncthreads();
    float cd[NR], pcur[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        cd[r] = 0.f; pcur[r] = p_init;
        if (ulive && r < nb) {
            if (c0) cd[r] = c0[(size_t)(bd0 + r) * H + ud];
            if (h0) hbuf[r * ldh + ud] = (bf16)h0[(size_t)(bd0 + r) * H + ud];
        }
    }
    __syncthreads();

    // this lane's gate inputs of the next PF steps (scan_units.h)
    const size_t gstep = (size_t)B * 4 * H;
    const float* gxl = gxc + (size_t)bd0 * 4 * H + udc;
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
    size_t soff = (size_t)bd0 * H;                              // float offset of (step t, sequence bd0) in h_all / c_all
    size_t uoff = (size_t)bd0 * E;                              // ... of the step the next read-out belongs to, in u_all
    size_t poff = (size_t)B + bd0;                              // ... in p_all (row 0: p_init)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < NR; ++r) if (r < nb) p_all[bd0 + r] = p_init;
    }
    int cur = 0;
    // au = W1 h of one step -> u (stored), p (stored, and in pcur for the next step's gates).  One barrier.
    auto readout = [&](const f32x4 (&au)[ES]) {
        float part[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) part[r] = 0.f;
#pragma unroll
        for (int s = 0; s < ES; ++s)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float u = fmaxf(au[s][r] + b1v[s], 0.f);
                part[r] += w2v[s] * u;
                if (lq == 0 && er[s] < E && r < nb) u_all[uoff + (size_t)r * E + er[s]] = u;
            }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            part[r] = fb_sum16(part[r]);                        // lanes 0..15 hold the live rows of D; the other quarters are products of zero rows
            if (lane == 0) pbuf[cur][jt * NR + r] = part[r];
        }
        lds_barrier();
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float p = b2v;
            for (int j = 0; j < NW; ++j) p += pbuf[cur][j * NR + r];    // wave order: the same sum in every lane and every run
            pcur[r] = p;
            if (threadIdx.x == 0 && r < nb) p_all[poff + r] = p;
        }
        uoff += (size_t)B * E;
        poff += (size_t)B;
    };
    auto step = [&](int t, In& slot) {
        const In in = slot;
        fetch(slot);
        f32x4 acc[4], au[ES];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < ES; ++s) au[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bf16* hb = hbuf + cur * 16 * ldh + l15 * ldh + 8 * lq;    // A fragments: row l15 = sequence l15
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 hf = *reinterpret_cast<const bf16x8*>(hb + ks * 32);
#pragma unroll
            for (int s = 0; s < ES; ++s) au[s] = mfma16(hf, w1[s][ks], au[s]);     // the read-out first: the gates wait for it
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = mfma16(hf, a[q][ks], acc[q]);
        }
        if (t > 0) readout(au);                                 // p_{t-1} from h_{t-1}; step 0 feeds p_init back
        float ig[NR], fg[NR], gg[NR], og[NR], hn[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            ig[r] = sigmoid_f(acc[0][r] + in.g[r][0] + pcur[r] * wpv[0]); fg[r] = sigmoid_f(acc[1][r] + in.g[r][1] + pcur[r] * wpv[1]);
            gg[r] = tanh_f(acc[2][r] + in.g[r][2] + pcur[r] * wpv[2]); og[r] = sigmoid_f(acc[3][r] + in.g[r][3] + pcur[r] * wpv[3]);
            cd[r] = fg[r] * cd[r] + ig[r] * gg[r];
            hn[r] = og[r] * tanh_f(cd[r]);
            // rows >= nb and units >= H of the h tile stay 0 (never written)
            if (ulive && r < nb) hbuf[(cur ^ 1) * 16 * ldh + r * ldh + ud] = (bf16)hn[r];
        }
        lds_barrier();                                          // h_t visible to every wave; global traffic stays in flight
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (ulive && r < nb) {
                const size_t o = soff + (size_t)r * H;
                st_uniform(h_all + o, uo[0], hn[r]);
                st_uniform(c_all + o, uo[0], cd[r]);
                float* ap = acts + o * 4;
                st_uniform(ap, uo[0], ig[r]); st_uniform(ap, uo[1], fg[r]); st_uniform(ap, uo[2], gg[r]); st_uniform(ap, uo[3], og[r]);
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
    {   // the read-out of the last step
        f32x4 au[ES];
#pragma unroll
        for (int s = 0; s < ES; ++s) au[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bf16* hb = hbuf + cur * 16 * ldh + l15 * ldh + 8 * lq;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 hf = *reinterpret_cast<const bf16x8*>(hb + ks * 32);
#pragma unroll
            for (int s = 0; s < ES; ++s) au[s] = mfma16(hf, w1[s][ks], au[s]);
        }
        readout(au);
    }
}

// Backward through time, t = T-1 .. 0, carrying dG_{t+1} (a bf16 tile in LDS, fp32 in the lanes that made it) and dc:
//   dp_t = g_t + dG_{t+1} . w_p      (fp32: per-wave butterfly, partial sums through LDS, added in wave order; 0 at t = T-1)
//   du_t = dp_t w2 [u_t > 0]         -> a bf16 tile in LDS, and du (T,B,E)
//   dh_t = [dG_{t+1} | du_t] . [W_hh ; W1]     one contraction of 4 HPAD + EK; its dG part is issued before du_t exists
//   dG_t = cell backward (scan_common.h)       -> dG (T,B,4H), also the gradient of gxc
// Two barriers per step.  dh0 = dG_0 . W_hh (p_{-1} is a constant).  KS4 = 4 HPAD / 32, KE = EK / 32.
template <int KS4, int KE, int NT, int NR>
__global__ __launch_bounds__(NT) void lstm_fb_scan_bwd_kernel(const float* __restrict__ dp_ext, const bf16* __restrict__ Wb, const bf16* __restrict__ W1b,
                                     const float* __restrict__ w_p, const float* __restrict__ w2, const float* __restrict__ c0,
                                     const float* __restrict__ c_all, const float* __restrict__ acts, const float* __restrict__ u_all,
                                     float* __restrict__ dG, float* __restrict__ du, float* __restrict__ dp,
                                     float* __restrict__ dh0, float* __restrict__ dc0, int T, int B, int H, int E, int HP16) {
    constexpr int KP4 = 32 * KS4, HPAD = KP4 / 4, ldg = KP4 + 8, EK = 32 * KE, lde = EK + 8;
    __shared__ __attribute__((aligned(16))) bf16 gbuf[16 * ldg];        // [16 rows: sequence r in row r][ldg]: k = gate*HPAD + unit
    __shared__ __attribute__((aligned(16))) bf16 dubuf[16 * lde];       // [16 rows][lde]: k = MLP row
    __shared__ float pbuf[8 * NR];                                      // [wave][sequence]: partial sums of dG . w_p
    const int lane = threadIdx.x & 63, jt = threadIdx.x >> 6, l15 = lane & 15, lq = lane >> 4, NW = blockDim.x >> 6;
    const int bd0 = blockIdx.x * NR;
    const int nb = (B - bd0) < NR ? (B - bd0) : NR;
    const int ud = jt * 16 + l15, udc = ud < H ? ud : H - 1;
    const bool ulive = (lq == 0) && (ud < H);
    const unsigned uo[4] = {4u * (unsigned)ud, 4u * (unsigned)(ud + H), 4u * (unsigned)(ud + 2 * H), 4u * (unsigned)(ud + 3 * H)};   // byte offsets

    // B fragments: column = unit jt*16 + l15 of dh
    const bf16* wrow = Wb + (size_t)(jt * 16 + l15) * KP4 + 8 * lq;
    bf16x8 a[KS4], a1[KE];
    load_wfrags(a, wrow);
    load_wfrags(a1, W1b + (size_t)(jt * 16 + l15) * EK + 8 * lq);
    float wpv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wpv[q] = w_p[(size_t)q * H + udc];
    // the MLP rows this thread turns into du: e = threadIdx.x and threadIdx.x + blockDim.x (E <= 128 <= 2 * 64)
    int ev[2];
    float w2e[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        ev[i] = (int)threadIdx.x + i * (int)blockDim.x;
        w2e[i] = ev[i] < E ? w2[ev[i]] : 0.f;
    }
    lds_zero(gbuf, 16 * ldg);
    lds_zero(dubuf, 16 * lde);
    if (threadIdx.x < 8 * NR) pbuf[threadIdx.x] = 0.f;
    __syncthreads();

    const size_t ostep = (size_t)B * H;
    size_t bo[NR];                                                      // (sequence, unit) offset inside a step; dead rows read row 0
    int br[NR];                                                         // the sequence a row reads
#pragma unroll
    for (int r = 0; r < NR; ++r) { br[r] = bd0 + (r < nb ? r : 0); bo[r] = (size_t)br[r] * H + udc; }
    struct In { float ig[NR], fg[NR], gg[NR], og[NR], ct[NR], cp[NR], ge[NR], u[2][NR]; };
    auto fetch = [&](int t) {
        In q;
        const size_t so = (size_t)t * ostep;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float* ap = acts + (so + bo[r] - udc) * 4 + udc;
            q.ig[r] = ap[0]; q.fg[r] = ap[H]; q.gg[r] = ap[2 * H]; q.og[r] = ap[3 * H];
            q.ct[r] = c_all[so + bo[r]];
            const float cprev = c_all[so - (t > 0 ? ostep : 0) + bo[r]];
            const float cinit = c0 ? c0[bo[r]] : 0.f;                   // c_{-1} = c0
            q.cp[r] = t > 0 ? cprev : cinit;
            q.ge[r] = dp_ext[(size_t)t * B + br[r]];
#pragma unroll
            for (int i = 0; i < 2; ++i) q.u[i][r] = u_all[((size_t)t * B + br[r]) * E + (ev[i] < E ? ev[i] : E - 1)];
        }
        return q;
    };
    float dcd[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) dcd[r] = 0.f;
    const bf16* gb = gbuf + l15 * ldg + 8 * lq;                         // A fragments: row l15 = sequence l15 (rows >= nb are zero)
    const bf16* db = dubuf + l15 * lde + 8 * lq;
    // dG_{t+1} . W_hh: four independent accumulation chains (a single chain of KS4 dependent MFMAs would serialise on the accumulator latency)
    auto rec_product = [&]() {
        f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < KS4; ++ks) acc[ks & 3] = mfma16(*reinterpret_cast<const bf16x8*>(gb + ks * 32), a[ks], acc[ks & 3]);
        return (acc[0] + acc[1]) + (acc[2] + acc[3]);
    };
    In nxt = fetch(T - 1);
    for (int t = T - 1; t >= 0; --t) {
        const In in = nxt;
        nxt = fetch(t > 0 ? t - 1 : 0);                                 // past the end re-reads step 0 (unused)
        float dpv[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float s = in.ge[r];
            for (int j = 0; j < NW; ++j) s += pbuf[j * NR + r];         // wave order: the same sum in every lane and every run
            dpv[r] = s;
        }
        f32x4 dh = rec_product();                                       // reads dG_{t+1}: before the barrier behind which dG_t is written
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (ev[i] < E) {
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    if (r < nb) {
                        const float d = in.u[i][r] > 0.f ? dpv[r] * w2e[i] : 0.f;
                        du[((size_t)t * B + bd0 + r) * E + ev[i]] = d;
                        dubuf[r * lde + ev[i]] = (bf16)d;               // rows >= nb and columns >= E stay 0 (never written)
                    }
            }
        if (threadIdx.x == 0) {
#pragma unroll
            for (int r = 0; r < NR; ++r) if (r < nb) dp[(size_t)t * B + bd0 + r] = dpv[r];
        }
        lds_barrier();                                                  // du_t visible; every wave has read dG_{t+1} and its partial sums
#pragma unroll
        for (int ks = 0; ks < KE; ++ks) dh = mfma16(*reinterpret_cast<const bf16x8*>(db + ks * 32), a1[ks], dh);
        float dgi[NR], dgf[NR], dgg[NR], dgo[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const bool lived = ulive && r < nb;
            lstm_cell_bwd(lived, in.ig[r], in.fg[r], in.gg[r], in.og[r], in.ct[r], in.cp[r], dh[r], 0.f, 0.f, dcd[r], dgi[r], dgf[r], dgg[r], dgo[r]);
            if (lived) {
                bf16* gw = gbuf + r * ldg + ud;
                gw[0] = (bf16)dgi[r]; gw[HPAD] = (bf16)dgf[r]; gw[2 * HPAD] = (bf16)dgg[r]; gw[3 * HPAD] = (bf16)dgo[r];
            }
            // dead lanes hold zeros (lstm_cell_bwd); lanes 0..15 are the live quarter
            const float part = fb_sum16((dgi[r] * wpv[0] + dgf[r] * wpv[1]) + (dgg[r] * wpv[2] + dgo[r] * wpv[3]));
            if (lane == 0) pbuf[jt * NR + r] = part;
        }
        lds_barrier();                                                  // dG_t and its partial sums visible
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (ulive && r < nb) {
                float* gp = dG + ((size_t)t * B + bd0 + r) * 4 * H;
                st_uniform(gp, uo[0], dgi[r]); st_uniform(gp, uo[1], dgf[r]); st_uniform(gp, uo[2], dgg[r]); st_uniform(gp, uo[3], dgo[r]);
            }
    }
    const f32x4 dhi = rec_product();                                    // dh_{-1} = dG_0 . W_hh
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (ulive && r < nb) {
            if (dh0) dh0[(size_t)(bd0 + r) * H + ud] = dhi[r];
            if (dc0) dc0[(size_t)(bd0 + r) * H + ud] = dcd[r];
        }
}
