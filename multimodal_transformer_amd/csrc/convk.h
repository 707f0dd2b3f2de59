// Window encoder with K taps, 1 <= K <= 5 (K = 2 stays on convpool.h: the product has one k = 2 path): Conv1d(D -> F, kernel K,
// bias) over the W rows of a window, then the global max-pool over the W - K + 1 conv positions (transformer/SFT/models.py:57-79,
// where k reaches nn.Conv1d unchanged).
//     S[n][p][f] = sum_{j<K} sum_d x[n][p+j][d] w[f][d][j]     out[n][f] = max_p S + b[f]     arg = first p of the maximum
//     dW[f][d][j] = sum_n dy[n][f] x[n][arg+j][d]              db[f] = sum_n dy[n][f]
// Numerics as in convpool.h: x and w become bf16 while staging, mfma_f32_32x32x16_bf16 accumulates in fp32, the bias is added after
// the pool in fp32; the backward rounds dy to bf16 for dW and sums the unrounded dy for db.  No atomics: runs repeat bit for bit.
//
// Forward (convk_fwd_kernel<K, CT>): convpool_fwd_kernel's geometry with K taps.  Workgroup = 8 windows x 64*CT channels, 8 waves, a
//   wave = 2 windows x 32*CT channels.  A row tile of 32 conv positions needs the raw rows rt*32 .. rt*32 + 32 + K - 2; they are staged
//   ONCE per 32-column chunk of D and serve all K taps (tap j = row p + j), so x traffic does not grow with K and the accumulator
//   count does not depend on K.  LDS per buffer: 8 (32 + K - 1) raw rows + K * 64 CT weight rows, 80 B each, double buffered:
//       bytes = 2 * (8 (31 + K) + 64 K CT) * 80        K:      1        3        4        5
//                                              CT = 4:   81,920  166,400  208,640  250,880      (the CU has 163,840: K >= 3 does not fit)
//                                              CT = 2:   61,440  104,960  126,720  148,480
//                                              CT = 1:   51,200   74,240   85,760   97,280
//   so every K runs at CT = 2 (128 channels per workgroup), with CT = 1 for a channel remainder of at most 64.  One workgroup per CU at
//   every K >= 3 (two at K = 1), and an A fragment feeds 2 MFMAs where convpool_fwd_kernel<4> feeds 4: that is the price of this geometry.
// Backward (convk_bwd_kernel<ONE_RT>): convpool_bwd_kernel's one-hot GEMM with THE TAP IN THE GRID.  One transposed copy per tap would be
//   K * 40 KB of LDS (the whole CU at K = 4); here a workgroup owns one tap: 256 channels x 128 raw features x tap j for a slice of the
//   windows, 2 * 2 * 128 * 40 bf16 = 40,960 B of LDS at any K and 4 accumulator tiles per wave.  Tap j stages raw row p + j as position
//   p, so the one-hot A operand is the same for every tap.  Cost: the K workgroups of a (feature block, split, channel block) each read
//   the window's rows, dy and argmax again: K-fold reads of x (mostly from L2) where the 2-tap kernel reads them once for both taps.
#pragma once
#include "convpool.h"

#define CK_MAXK 5
#define CK_CT 2                        // channel tiles per wave of the bulk launch: 128 channels per workgroup

__host__ __device__ inline size_t convk_fwd_lds_bytes(int k, int ct) {
    return (size_t)2 * (CP_WIN * (32 + k - 1) * CP_LDX + k * 64 * ct * CP_LDX) * sizeof(bf16);
}
__host__ __device__ inline size_t convk_bwd_lds_bytes() {
    return (size_t)2 * 2 * CP_DB * CP_PS * sizeof(bf16);                   // [buffer][window of the pair][d][position]
}

// weight (F, D, K) fp32 (nn.Conv1d layout) -> Wp bf16 [K][FPAD][DP], zero padded
__global__ void convk_prep_kernel(const float* __restrict__ w, bf16* __restrict__ Wp, int F, int D, int K, int FPAD, int DP) {
    const size_t n = (size_t)K * FPAD * DP;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int d = (int)(idx % DP), f = (int)((idx / DP) % FPAD), tap = (int)(idx / ((size_t)DP * FPAD));
        Wp[idx] = (bf16)((f < F && d < D) ? w[((size_t)f * D + d) * K + tap] : 0.f);
    }
}

// grid (ceil(N/8), channel blocks); block 512.  The workgroup covers CFB = 64*CT channels starting at c_first + blockIdx.y*CFB.
template <int K, int CT>
__global__ __launch_bounds__(512) void convk_fwd_kernel(const float* __restrict__ X, const bf16* __restrict__ Wp,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        int* __restrict__ arg, int N, int W, int D, int DP, int F, int FPAD,
                                                        int c_first) {
    constexpr int CFB = 64 * CT, ROWS = 32 + K - 1;                        // raw rows staged per 32-position row tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Xs = reinterpret_cast<bf16*>(smem);                              // [2][CP_WIN][ROWS][CP_LDX]
    bf16* Bs = Xs + 2 * CP_WIN * ROWS * CP_LDX;                            // [2][K][CFB][CP_LDX]
    constexpr int XS_STAGE = CP_WIN * ROWS * CP_LDX, BS_STAGE = K * CFB * CP_LDX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int wpair = wave >> 1, chalf = wave & 1;
    const int n0 = blockIdx.x * CP_WIN, cblk = c_first + blockIdx.y * CFB;
    const int npos = W - K + 1, nrt = (npos + 31) / 32, nchunk = DP / CP_KC;

    // staging tasks of this thread: X: items tid + 512*i over CP_WIN*ROWS*8 float4;  W: items tid + 512*i over K*CFB*4 pieces of 8 bf16
    constexpr int XITEMS = CP_WIN * ROWS * (CP_KC / 4), XPER = (XITEMS + 511) / 512;
    constexpr int WITEMS = K * CFB * 4, WPER = (WITEMS + 511) / 512;
    f32x4 xr[XPER];
    bf16x8 wr[WPER];

    float best[2][CT];
    int bestp[2][CT];
#pragma unroll
    for (int wi = 0; wi < 2; ++wi)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) { best[wi][ct] = -INFINITY; bestp[wi][ct] = 0; }

    for (int rt = 0; rt < nrt; ++rt) {
        auto load_chunk = [&](int ch) {
            const int kc = ch * CP_KC;
#pragma unroll
            for (int i = 0; i < XPER; ++i) {
                const int item = tid + 512 * i;
                const int win = item / (ROWS * 8), rem = item - win * (ROWS * 8), row = rem >> 3, c4 = rem & 7;
                const int n = n0 + win, p = rt * 32 + row, c = kc + 4 * c4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (item < XITEMS && n < N && p < W && c < D) v = *reinterpret_cast<const f32x4*>(X + ((size_t)n * W + p) * D + c);
                xr[i] = v;
            }
#pragma unroll
            for (int i = 0; i < WPER; ++i) {
                const int item = tid + 512 * i;
                const int tap = item / (CFB * 4), chn = (item >> 2) % CFB, c8 = item & 3;
                bf16x8 v = {};
                if (item < WITEMS) v = *reinterpret_cast<const bf16x8*>(Wp + ((size_t)tap * FPAD + cblk + chn) * DP + kc + 8 * c8);
                wr[i] = v;
            }
        };
        auto store_chunk = [&](int stage) {
            bf16* xs = Xs + stage * XS_STAGE;
            bf16* bs = Bs + stage * BS_STAGE;
#pragma unroll
            for (int i = 0; i < XPER; ++i) {
                const int item = tid + 512 * i;
                if (item < XITEMS) {
                    const int win = item / (ROWS * 8), rem = item - win * (ROWS * 8), row = rem >> 3, c4 = rem & 7;
                    const f32x2 lo = {xr[i][0], xr[i][1]}, hi = {xr[i][2], xr[i][3]};
                    uint2 pk;
                    pk.x = __builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2));
                    pk.y = __builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2));
                    *reinterpret_cast<uint2*>(xs + (win * ROWS + row) * CP_LDX + 4 * c4) = pk;
                }
            }
#pragma unroll
            for (int i = 0; i < WPER; ++i) {
                const int item = tid + 512 * i;
                if (item < WITEMS) {
                    const int tap = item / (CFB * 4), chn = (item >> 2) % CFB, c8 = item & 3;
                    *reinterpret_cast<bf16x8*>(bs + (tap * CFB + chn) * CP_LDX + 8 * c8) = wr[i];
                }
            }
        };

        f32x16 acc[2][CT];
#pragma unroll
        for (int wi = 0; wi < 2; ++wi)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[wi][ct][i] = 0.f;

        __syncthreads();                                                  // previous row tile's readers are done
        load_chunk(0);
        store_chunk(0);
        __syncthreads();
        for (int ch = 0; ch < nchunk; ++ch) {
            const int stage = ch & 1;
            // the next chunk's global loads in flight behind this chunk's MFMAs; branch-free (the last iteration re-fetches its own chunk)
            load_chunk(ch + 1 < nchunk ? ch + 1 : ch);
            const bf16* xs = Xs + stage * XS_STAGE + (2 * wpair * ROWS + r) * CP_LDX + 8 * hh;
            const bf16* bs = Bs + stage * BS_STAGE + (chalf * 32 * CT + r) * CP_LDX + 8 * hh;
#pragma unroll
            for (int tap = 0; tap < K; ++tap) {
#pragma unroll
                for (int ks = 0; ks < CP_KC / 16; ++ks) {
                    bf16x8 a[2];
#pragma unroll
                    for (int wi = 0; wi < 2; ++wi)                        // conv position r, tap j = staged row r + j (at most ROWS - 1)
                        a[wi] = *reinterpret_cast<const bf16x8*>(xs + (wi * ROWS + tap) * CP_LDX + ks * 16);
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        const bf16x8 b = *reinterpret_cast<const bf16x8*>(bs + (tap * CFB + ct * 32) * CP_LDX + ks * 16);
#pragma unroll
                        for (int wi = 0; wi < 2; ++wi) acc[wi][ct] = mfma32(a[wi], b, acc[wi][ct]);
                    }
                }
            }
            store_chunk(stage ^ 1);
            __syncthreads();
        }

        // ---- max-pool epilogue of this row tile: column r of a tile = channel, rows = positions rt*32 + row
        const int plim = npos - rt * 32;                                   // positions >= plim are padding
#pragma unroll
        for (int wi = 0; wi < 2; ++wi)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                float bv = -INFINITY;
                int bp = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = acc32_row(i, hh);
                    const float v = row < plim ? acc[wi][ct][i] : -INFINITY;
                    if (v > bv) { bv = v; bp = row; }                     // rows ascend with i inside a lane: first maximum wins
                }
                const float ov = __shfl_xor(bv, 32);
                const int op = __shfl_xor(bp, 32);
                if (ov > bv || (ov == bv && op < bp)) { bv = ov; bp = op; }
                bp += rt * 32;
                if (bv > best[wi][ct]) { best[wi][ct] = bv; bestp[wi][ct] = bp; }
            }
    }

    if (hh == 0) {
#pragma unroll
        for (int wi = 0; wi < 2; ++wi) {
            const int n = n0 + 2 * wpair + wi;
            if (n >= N) continue;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const int c = cblk + chalf * 32 * CT + ct * 32 + r;
                if (c < F) {
                    out[(size_t)n * F + c] = best[wi][ct] + bias[c];
                    arg[(size_t)n * F + c] = bestp[wi][ct];
                }
            }
        }
    }
}

// grid (K * ceil(D/128), nsplit, FPAD/256); block 512: blockIdx.x = feature block * K + tap.  slab layout [split][tap][FPAD][DPB] with
// DPB = 128 * ceil(D/128).  ONE_RT: at most 32 conv positions (W - K + 1 <= 32): item = window pair, no index divisions in the loop
template <bool ONE_RT>
__global__ __launch_bounds__(512) void convk_bwd_kernel(const float* __restrict__ X, const float* __restrict__ dy,
                                                        const int* __restrict__ arg, float* __restrict__ slab,
                                                        float* __restrict__ dbpart,
                                                        int N, int W, int D, int F, int K, int FPAD, int wins_per_split) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* XT = reinterpret_cast<bf16*>(smem);                              // [2 buffers][2 windows][CP_DB][CP_PS]
    constexpr int XT_WIN = CP_DB * CP_PS, XT_BUF = 2 * XT_WIN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int fq = wave >> 1, dhalf = wave & 1;                            // wave tile: f tiles 2fq, 2fq+1; d tiles 2dhalf, 2dhalf+1
    const int tap = blockIdx.x % K, dblk = blockIdx.x / K;
    const int d0 = dblk * CP_DB, cblk = blockIdx.z * CP_FB;
    const int nbeg = blockIdx.y * wins_per_split, nend = min(N, nbeg + wins_per_split);
    const int DPB = CP_DB * (gridDim.x / K);
    const int npos = W - K + 1, nrt = (npos + 31) / 32;

    // staging role: 4 waves per window slot; lane = g + 8*dd: positions 4g..4g+3 (raw rows + tap), float4 column dd of this wave's 32 columns
    const int swin = wave >> 2, sw4 = wave & 3, g = lane & 7, dd = lane >> 3;
    const int sd = sw4 * 32 + 4 * dd;                                      // first of 4 raw features (within the 128 block)
    f32x4 xr[4];

    f32x16 acc[2][2];                                                      // [f tile][d tile]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    // work items: (window pair, row tile); each item stages two windows and runs 2 x 8 MFMAs per wave
    const int npairs = (nend - nbeg + 1) / 2;
    const int nitems = npairs > 0 ? npairs * nrt : 0;
    float dyn[2][2];                                                       // next item: dy and (arg - row tile base) of this lane's
    int avn[2][2];                                                         // channels, [window of the pair][f tile]
    auto load_rows = [&](int it) {
        const int pr = ONE_RT ? it : it / nrt, rt = ONE_RT ? 0 : it - pr * nrt;
        const int n = nbeg + 2 * pr + swin;
        const bool ok = n < nend && (d0 + sd) < D;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = rt * 32 + 4 * g + i + tap;                       // the raw row that tap `tap` multiplies at position 4g + i
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok && p < W) v = *reinterpret_cast<const f32x4*>(X + ((size_t)n * W + p) * D + d0 + sd);
            xr[i] = v;
        }
    };
    auto load_dy = [&](int it) {
        const int pr = ONE_RT ? it : it / nrt, rt = ONE_RT ? 0 : it - pr * nrt;
#pragma unroll
        for (int w2 = 0; w2 < 2; ++w2)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int nn = nbeg + 2 * pr + w2, f = cblk + (2 * fq + a) * 32 + r;
                const bool okf = nn < nend && f < F;
                dyn[w2][a] = okf ? dy[(size_t)nn * F + f] : 0.f;
                avn[w2][a] = okf ? arg[(size_t)nn * F + f] - rt * 32 : -1;
            }
    };
    auto store_item = [&](int buf) {
        bf16* base = XT + buf * XT_BUF + swin * XT_WIN;
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                      // raw feature sd + c: positions 4g..4g+3
            const f32x2 a0 = {xr[0][c], xr[1][c]}, a1 = {xr[2][c], xr[3][c]};
            uint2 t0;
            t0.x = __builtin_bit_cast(unsigned, __builtin_convertvector(a0, bf16x2));
            t0.y = __builtin_bit_cast(unsigned, __builtin_convertvector(a1, bf16x2));
            *reinterpret_cast<uint2*>(base + (sd + c) * CP_PS + 4 * g) = t0;
        }
    };

    // Pipeline as in convpool_bwd_kernel: rows two items ahead of the MFMAs (registers), transposed into the idle LDS buffer one item
    // ahead; dy / argmax one item ahead.  One barrier per item; the loop body has no skippable blocks (clamped re-fetches).
    float dyc[2][2];
    int avc[2][2];
    float dbacc[2] = {0.f, 0.f};
    if (nitems > 0) {
        load_rows(0);
        load_dy(0);
        store_item(0);
        load_rows(nitems > 1 ? 1 : 0);
#pragma unroll
        for (int w2 = 0; w2 < 2; ++w2)
#pragma unroll
            for (int a = 0; a < 2; ++a) { dyc[w2][a] = dyn[w2][a]; avc[w2][a] = avn[w2][a]; }
    }
    __syncthreads();
    for (int it = 0; it < nitems; ++it) {
        store_item((it + 1) & 1);                                          // rows of item it+1 (readers of that buffer: item it-1, done)
        load_rows(it + 2 < nitems ? it + 2 : nitems - 1);
        load_dy(it + 1 < nitems ? it + 1 : it);
        const bf16* XTb = XT + (it & 1) * XT_BUF;
        const float first_rt = (ONE_RT || it % nrt == 0) ? 1.f : 0.f;      // bias gradient: every (window, channel) once
#pragma unroll
        for (int a = 0; a < 2; ++a) dbacc[a] += first_rt * (dyc[0][a] + dyc[1][a]);
#pragma unroll
        for (int w2 = 0; w2 < 2; ++w2) {
            // one-hot A fragments: lane (r, hh) holds channel f, positions rt*32 + ks*16 + 8hh + j
            const float* dyv = dyc[w2];
            const int* av = avc[w2];
            const bf16* xt = XTb + w2 * XT_WIN + (dhalf * 64 + r) * CP_PS + 8 * hh;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 afr[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int j = av[a] - ks * 16 - 8 * hh;                // element index inside this fragment, or out of range
                    const unsigned bits = (unsigned)__builtin_bit_cast(unsigned short, (bf16)dyv[a]);
                    const unsigned val = bits << ((j & 1) << 4);           // the value in its half of a dword
                    const int e0 = j >> 1;                                 // dword index (arithmetic shift: out of range stays so)
                    u32x4_t q;
#pragma unroll
                    for (int e = 0; e < 4; ++e) q[e] = (e0 == e) ? val : 0u;
                    afr[a] = __builtin_bit_cast(bf16x8, q);
                }
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(xt + b * 32 * CP_PS + ks * 16);
#pragma unroll
                    for (int a = 0; a < 2; ++a) acc[a][b] = mfma32(afr[a], bfr, acc[a][b]);
                }
            }
        }
#pragma unroll
        for (int w2 = 0; w2 < 2; ++w2)
#pragma unroll
            for (int a = 0; a < 2; ++a) { dyc[w2][a] = dyn[w2][a]; avc[w2][a] = avn[w2][a]; }
        __syncthreads();
    }

    if (blockIdx.x == 0 && dhalf == 0 && hh == 0) {                        // tap 0 of feature block 0: one wave per f-tile pair owns the bias partials
#pragma unroll
        for (int a = 0; a < 2; ++a) dbpart[(size_t)blockIdx.y * FPAD + cblk + (2 * fq + a) * 32 + r] = dbacc[a];
    }
    // D tile: column = lane r = raw feature, rows = channels
    float* sl = slab + ((size_t)blockIdx.y * K + tap) * FPAD * DPB;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int f = cblk + (2 * fq + a) * 32 + acc32_row(i, hh);
                const int d = d0 + dhalf * 64 + b * 32 + r;
                sl[(size_t)f * DPB + d] = acc[a][b][i];
            }
}

// dweight (F, D, K) = sum over splits of slab[split][tap][f][d];  dbias[f] = sum over splits of dbpart[split][f]
__global__ void convk_finish_kernel(const float* __restrict__ slab, const float* __restrict__ dbpart, float* __restrict__ dweight,
                                    float* __restrict__ dbias, int nsplit, int D, int F, int K, int FPAD, int DPB) {
    const size_t nw = (size_t)F * D * K;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < nw + F; idx += (size_t)gridDim.x * blockDim.x) {
        if (idx < nw) {
            const int tap = (int)(idx % K), d = (int)((idx / K) % D), f = (int)((idx / K) / D);
            float s = 0.f;
            for (int sp = 0; sp < nsplit; ++sp) s += slab[(((size_t)sp * K + tap) * FPAD + f) * DPB + d];
            dweight[idx] = s;
        } else {
            const int f = (int)(idx - nw);
            float s = 0.f;
            for (int sp = 0; sp < nsplit; ++sp) s += dbpart[(size_t)sp * FPAD + f];
            dbias[f] = s;
        }
    }
}
