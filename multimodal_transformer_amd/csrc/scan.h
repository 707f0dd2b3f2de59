// The general LSTM scans: the T-sequential recurrence as persistent-state kernels for gfx950, 4..16 sequences per workgroup.
// plan_lstm_scan (api.hip) comes here last (LSTM_GENERAL): BT > 2, that is batches above 512 sequences, at HPAD 64 / 128 / 256.
//
// LSTM scan (MFN's per-modality nn.LSTMCell, transformer/MFT/multiTransformer.py:152,208, and the SFT
// decoder's nn.LSTM step, transformer/SFT/multiTransformer.py:471-476).  Only gates += W_rec . h_{t-1} is
// recurrent; the input projection gx[t] = x_t W_ih^T + b_ih + b_hh is batched over all T by the row GEMM.
// One workgroup owns BT <= 16 sequences (columns of the MFMA N dimension; BT is chosen so that the batch
// spreads over up to 256 CUs — the scan is latency-bound, idle MFMA columns cost nothing) for the whole scan;
// wave w owns hidden units [16w, 16w+16) and keeps its slice of W_rec as MFMA A fragments in registers for
// all T steps, the cell state in registers (fp32), and h crosses waves through a double-buffered bf16 LDS
// tile: one barrier per step.  Gate order i, f, g, o (torch).  HPAD <= 128 keeps W_rec in registers; HPAD = 256 re-streams it
// from L2 every step (WREG = false).  The other families: scan_units.h (one / two sequences per workgroup), scan_cluster.h
// (H > 128, four CUs per sequence), scan256.h (H > 128, half-resident weights).  The MFN memory recurrence is mfn_scan.h; what the
// families share is scan_common.h.
#pragma once
#include "scan_common.h"

// W_rec (4H,H) fp32 -> forward operand Wf bf16 [4][HP16][HPAD] (Wf[q][j][k] = W[q*H+j][k]) and
// backward operand Wb bf16 [HP16][4*HPAD] (Wb[j][q*HPAD+j'] = W[q*H+j'][j]); zero padded.
// HPAD = hidden size padded to 64 / 128 / 256: every loop bound in the scans is then a compile-time constant.
__global__ void lstm_prep_kernel(const float* __restrict__ W, bf16* __restrict__ Wf, bf16* __restrict__ Wb,
                                 int H, int HP16, int HPAD) {
    const size_t nf = (size_t)4 * HP16 * HPAD, nb = (size_t)HP16 * 4 * HPAD;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < nf + nb; idx += (size_t)gridDim.x * blockDim.x) {
        if (idx < nf) {
            const int k = (int)(idx % HPAD), j = (int)((idx / HPAD) % HP16), q = (int)(idx / ((size_t)HPAD * HP16));
            Wf[idx] = (bf16)((j < H && k < H) ? W[((size_t)q * H + j) * H + k] : 0.f);
        } else {
            const size_t i = idx - nf;
            const int c = (int)(i % (4 * HPAD)), j = (int)(i / (4 * HPAD));
            const int q = c / HPAD, jp = c - q * HPAD;
            Wb[i] = (bf16)((j < H && jp < H) ? W[((size_t)q * H + jp) * H + j] : 0.f);
        }
    }
}

// grid = ceil(B/BT); block = 64 * (HP16/16) <= NT.  HPAD = 32*KS.  WREG: W_rec fragments stay in registers for the
// whole scan (HPAD <= 128); otherwise (HPAD = 256: 512 KB of bf16 weights exceed one CU's register file) they are
// re-streamed from L2 every step.  The time loop is straight-line code: lanes outside the batch / hidden range
// compute on clamped addresses and simply do not store.  This is the form for 4..16 sequences per workgroup (batches above 512);
// one or two sequences per workgroup run the kernels of scan_units.h.
template <int KS, int NT, bool WREG, int PF>
__global__ __launch_bounds__(NT) void lstm_scan_fwd_kernel(const float* __restrict__ gx, const bf16* __restrict__ Wf,
                                     const float* __restrict__ h0, const float* __restrict__ c0,
                                     float* __restrict__ h_all, float* __restrict__ c_all, float* __restrict__ acts,
                                     int T, int B, int H, int HP16, int BT) {
    constexpr int KP = 32 * KS, ldh = KP + 8;
    __shared__ __attribute__((aligned(16))) bf16 hbuf[2 * 16 * ldh];
    const int lane = threadIdx.x & 63, jt = threadIdx.x >> 6, l15 = lane & 15, lq = lane >> 4;
    // BT <= 16 sequences per workgroup: the scan is latency-bound and its per-step traffic must not funnel through a
    // couple of CUs, so small batches are spread over many workgroups and the unused MFMA columns simply idle.
    const int b = blockIdx.x * BT + l15, j0 = jt * 16 + 4 * lq;
    const bool live = (l15 < BT) && (b < B) && (j0 < H);        // H % 4 == 0: the 4 rows of a lane are all in or all out
    const int bc = b < B ? b : B - 1, jc = j0 < H ? j0 : H - 4; // clamped (always valid) coordinates for loads

    const bf16* wrow = Wf + (size_t)(jt * 16 + l15) * KP + 8 * lq;      // + q*HP16*KP + ks*32
    const size_t wq = (size_t)HP16 * KP;
    bf16x8 a[WREG ? 4 : 1][WREG ? KS : 1];
    if (WREG) {
#pragma unroll
        for (int q = 0; q < 4; ++q) load_wfrags(a[q], wrow + q * wq);
    }
    lds_clear(hbuf, 2 * 16 * ldh);
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        if (c0) c = *reinterpret_cast<const f32x4*>(c0 + (size_t)b * H + j0);
        if (h0) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(h0 + (size_t)b * H + j0);
#pragma unroll
            for (int r = 0; r < 4; ++r) hbuf[l15 * ldh + j0 + r] = (bf16)hv[r];
        }
    }
    __syncthreads();

    const size_t gstep = (size_t)B * 4 * H;
    // input projections of the next PF steps are always in flight (register ring, statically indexed by unrolling)
    f32x4 ring[PF][4];
    const float* gxl = gx + (size_t)bc * 4 * H + jc;            // + t*gstep + q*H
    auto fetch = [&](f32x4 (&r)[4], int t) {
        const int tl = t < T ? t : T - 1;                       // clamped: the tail re-reads the last step (unused)
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = *reinterpret_cast<const f32x4*>(gxl + tl * gstep + (size_t)q * H);
    };
#pragma unroll
    for (int d = 0; d < PF; ++d) fetch(ring[d], d);
    int cur = 0;
    auto step = [&](int t, f32x4 (&in)[4]) {
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = in[q];
        fetch(in, t + PF);
        const bf16* hb = hbuf + cur * 16 * ldh + l15 * ldh + 8 * lq;
        if (WREG) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 bf = *reinterpret_cast<const bf16x8*>(hb + ks * 32);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = mfma16(a[WREG ? q : 0][WREG ? ks : 0], bf, acc[q]);
            }
        } else {
            // streamed weights: two k-blocks of fragments in flight; the scheduling fences keep hipcc from hoisting
            // all 4*KS fragment loads to the top of the step (128 VGPRs at KS = 8: spills)
            bf16x8 wa[2][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) wa[0][q] = *reinterpret_cast<const bf16x8*>(wrow + q * wq);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks + 1 < KS) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) wa[(ks + 1) & 1][q] = *reinterpret_cast<const bf16x8*>(wrow + q * wq + (ks + 1) * 32);
                }
                const bf16x8 bf = *reinterpret_cast<const bf16x8*>(hb + ks * 32);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = mfma16(wa[ks & 1][q], bf, acc[q]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        f32x4 ig, fg, gg, og, hn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ig[r] = sigmoid_f(acc[0][r]); fg[r] = sigmoid_f(acc[1][r]); gg[r] = tanh_f(acc[2][r]); og[r] = sigmoid_f(acc[3][r]);
            c[r] = fg[r] * c[r] + ig[r] * gg[r];
            hn[r] = live ? og[r] * tanh_f(c[r]) : 0.f;      // pad lanes keep h = 0 in LDS
        }
        bf16x4 hb4;
#pragma unroll
        for (int r = 0; r < 4; ++r) hb4[r] = (bf16)hn[r];
        *reinterpret_cast<bf16x4*>(hbuf + (cur ^ 1) * 16 * ldh + l15 * ldh + jt * 16 + 4 * lq) = hb4;
        lds_barrier();                                      // h_t visible to every wave; global traffic stays in flight
        if (live) {
            const size_t o = ((size_t)t * B + b) * H + j0;
            *reinterpret_cast<f32x4*>(h_all + o) = hn;
            *reinterpret_cast<f32x4*>(c_all + o) = c;
            float* ap = acts + ((size_t)t * B + b) * 4 * H + j0;
            *reinterpret_cast<f32x4*>(ap) = ig; *reinterpret_cast<f32x4*>(ap + H) = fg;
            *reinterpret_cast<f32x4*>(ap + 2 * H) = gg; *reinterpret_cast<f32x4*>(ap + 3 * H) = og;
        }
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

// Backward through time.  dG[t] (gate pre-activation gradients, fp32 (T,B,4H)) is also what the batched
// input-projection / weight gradients consume afterwards.  KS4 = 4*HPAD/32.
template <int KS4, int NT, bool WREG, int PF>
__global__ __launch_bounds__(NT) void lstm_scan_bwd_kernel(const float* __restrict__ dh_ext, const float* __restrict__ dc_ext,
                                     const bf16* __restrict__ Wb, const float* __restrict__ c0,
                                     const float* __restrict__ c_all, const float* __restrict__ acts,
                                     float* __restrict__ dG, float* __restrict__ dh0, float* __restrict__ dc0,
                                     int T, int B, int H, int HP16, int BT) {
    constexpr int KP4 = 32 * KS4, HPAD = KP4 / 4, ldg = KP4 + 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* gbuf = reinterpret_cast<bf16*>(smem);                 // [2][16][ldg]
    const int lane = threadIdx.x & 63, jt = threadIdx.x >> 6, l15 = lane & 15, lq = lane >> 4;
    const int b = blockIdx.x * BT + l15, j0 = jt * 16 + 4 * lq;
    const bool live = (l15 < BT) && (b < B) && (j0 < H);
    const int bc = b < B ? b : B - 1, jc = j0 < H ? j0 : H - 4;
    const float lv = live ? 1.f : 0.f;

    const bf16* wrow = Wb + (size_t)(jt * 16 + l15) * KP4 + 8 * lq;
    bf16x8 a[WREG ? KS4 : 1];
    if (WREG) load_wfrags(a, wrow);
    for (int i = threadIdx.x; i < 2 * 16 * ldg; i += blockDim.x) gbuf[i] = (bf16)0.f;
    __syncthreads();

    f32x4 dh_rec = {0.f, 0.f, 0.f, 0.f}, dc = {0.f, 0.f, 0.f, 0.f};
    // saved activations / cell states / external gradients of the next PF steps (going backwards) stay in flight
    struct StepIn { f32x4 ig, fg, gg, og, ct, cp, dhe, dce; };
    const size_t ostep = (size_t)B * H;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    StepIn ring[PF];
    const float* actl = acts + (size_t)bc * 4 * H + jc;
    const float* cl = c_all + (size_t)bc * H + jc;
    f32x4 c0v = zero4;
    if (c0) c0v = *reinterpret_cast<const f32x4*>(c0 + (size_t)bc * H + jc);
    auto fetch = [&](StepIn& r, int t) {
        const int tc = t > 0 ? t : 0;                           // clamped, branch-free
        const float* ap = actl + (size_t)tc * ostep * 4;
        r.ig = *reinterpret_cast<const f32x4*>(ap); r.fg = *reinterpret_cast<const f32x4*>(ap + H);
        r.gg = *reinterpret_cast<const f32x4*>(ap + 2 * H); r.og = *reinterpret_cast<const f32x4*>(ap + 3 * H);
        r.ct = *reinterpret_cast<const f32x4*>(cl + (size_t)tc * ostep);
        r.cp = *reinterpret_cast<const f32x4*>(cl + (size_t)(tc > 0 ? tc - 1 : 0) * ostep);
        if (t <= 0) r.cp = c0v;
        r.dhe = dh_ext ? *reinterpret_cast<const f32x4*>(dh_ext + (size_t)bc * H + jc + (size_t)tc * ostep) : zero4;
        r.dce = dc_ext ? *reinterpret_cast<const f32x4*>(dc_ext + (size_t)bc * H + jc + (size_t)tc * ostep) : zero4;
    };
#pragma unroll
    for (int d = 0; d < PF; ++d) fetch(ring[d], T - 1 - d);
    int cur = 0;
    auto step = [&](int t, StepIn& slot) {
        const StepIn in = slot;
        fetch(slot, t - PF);
        f32x4 dgi, dgf, dgg, dgo;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dh = dh_rec[r] + in.dhe[r];
            const float th = tanh_f(in.ct[r]);
            const float dct = dc[r] + in.dce[r] + dh * in.og[r] * (1.f - th * th);
            dgo[r] = lv * dh * th * in.og[r] * (1.f - in.og[r]);
            dgi[r] = lv * dct * in.gg[r] * in.ig[r] * (1.f - in.ig[r]);
            dgf[r] = lv * dct * in.cp[r] * in.fg[r] * (1.f - in.fg[r]);
            dgg[r] = lv * dct * in.ig[r] * (1.f - in.gg[r] * in.gg[r]);
            dc[r] = dct * in.fg[r];
        }
        bf16* gw = gbuf + cur * 16 * ldg + l15 * ldg + jt * 16 + 4 * lq;
        bf16x4 p0, p1, p2, p3;
#pragma unroll
        for (int r = 0; r < 4; ++r) { p0[r] = (bf16)dgi[r]; p1[r] = (bf16)dgf[r]; p2[r] = (bf16)dgg[r]; p3[r] = (bf16)dgo[r]; }
        *reinterpret_cast<bf16x4*>(gw) = p0; *reinterpret_cast<bf16x4*>(gw + HPAD) = p1;
        *reinterpret_cast<bf16x4*>(gw + 2 * HPAD) = p2; *reinterpret_cast<bf16x4*>(gw + 3 * HPAD) = p3;
        lds_barrier();
        if (live) {
            float* gp = dG + ((size_t)t * B + b) * 4 * H + j0;
            *reinterpret_cast<f32x4*>(gp) = dgi; *reinterpret_cast<f32x4*>(gp + H) = dgf;
            *reinterpret_cast<f32x4*>(gp + 2 * H) = dgg; *reinterpret_cast<f32x4*>(gp + 3 * H) = dgo;
        }
        const bf16* gb = gbuf + cur * 16 * ldg + l15 * ldg + 8 * lq;
        // four independent accumulation chains (one per gate block of the contraction): a single chain of KS4
        // dependent MFMAs would serialise on the accumulator latency
        f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        // the B operand (all 4H gate gradients of a sequence) is the LDS-bandwidth term of a step: 16 KB per wave
        // at H = 128.  Only the BT live MFMA columns are read; the other lanes keep whatever their registers
        // held (a column of D depends on the same column of B only, and dead columns are never stored).
        constexpr int KG = WREG ? KS4 : 8;                      // B fragments fetched per group (register budget)
#pragma unroll
        for (int k0 = 0; k0 < KS4; k0 += KG) {
            bf16x8 bfr[KG];
            if (l15 < BT) {
#pragma unroll
                for (int ks = 0; ks < KG; ++ks) bfr[ks] = *reinterpret_cast<const bf16x8*>(gb + (k0 + ks) * 32);
            }
#pragma unroll
            for (int ks = 0; ks < KG; ++ks) {
                const bf16x8 af = WREG ? a[WREG ? k0 + ks : 0] : *reinterpret_cast<const bf16x8*>(wrow + (k0 + ks) * 32);
                acc[ks & 3] = mfma16(af, bfr[ks], acc[ks & 3]);
            }
            if (!WREG) __builtin_amdgcn_sched_barrier(0);       // keep the next group's fragment loads below this point
        }
        dh_rec = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        cur ^= 1;
    };
    int tb = T - 1;
    for (; tb - PF + 1 >= 0; tb -= PF) {
#pragma unroll
        for (int d = 0; d < PF; ++d) step(tb - d, ring[d]);
    }
#pragma unroll
    for (int d = 0; d < PF; ++d) if (tb - d >= 0) step(tb - d, ring[d]);
    if (live) {
        if (dh0) *reinterpret_cast<f32x4*>(dh0 + (size_t)b * H + j0) = dh_rec;
        if (dc0) *reinterpret_cast<f32x4*>(dc0 + (size_t)b * H + j0) = dc;
    }
}

