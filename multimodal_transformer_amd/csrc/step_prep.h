// The preparation of a stream state whose parameters arrive as separate tensors (mmt_mfn_stream_prepare, mmt_decoder_stream_prepare): ONE
// launch of step_prep_kernel runs a table of jobs, blockIdx.y = job.
//   A matrix job lays the `rows` x K block at column col0 of a row-major fp32 source (leading dimension ld; plus the block at column
//   col2 of a second source, leading dimension ld2, where one is given: summed in fp32, rounded once) into `rows` rows of a prepared
//   [KP / 8][nout][8] bf16 matrix, k padded to KP by zeros.  `dst` is the byte offset of the first of those rows in the state: a job
//   that fills rows row0 .. of a matrix at byte offset `off` has dst = off + row0 * 8 * sizeof(bf16).
//   A vector job copies n floats (the sum of two sources where a second is given) to byte offset `dst`.
// The tables are built beside the plans (mfn_step_plan.h, decoder_step_plan.h).  Everything above the __HIPCC__ line is plain C++ for
// the host and the device: step_prep_at is the ONE place where a job and a linear index become a destination, so that a stand-alone
// program can walk every byte the kernel writes (tools/mfn_step_plan_check.cpp, tools/decoder_step_plan_check.cpp).
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MMT_PREP_HD __host__ __device__
#else
#define MMT_PREP_HD
#endif

#define MMT_STEP_PREP_MATS 20             // the MFN's: 2 per modality and 12 of the gate
#define MMT_STEP_PREP_VECS 14             // 1 per modality and 10 of the gate

struct StepPrepMat { const float* src; const float* src2; size_t dst; int ld, col0, ld2, col2, rows, K, KP, nout; };
struct StepPrepVec { const float* a; const float* b; size_t dst; int n; };
struct StepPrepParams {
    char* state;
    int nmat, nvec;
    StepPrepMat mat[MMT_STEP_PREP_MATS];
    StepPrepVec vec[MMT_STEP_PREP_VECS];
};
static_assert(sizeof(StepPrepParams) <= 4096, "the table travels as a kernel argument");

// element i < rows * KP of a matrix job: the source row n and column k (k >= K: padding, a zero) and the bf16 element behind J.dst
struct StepPrepAt { int n, k; size_t dst; };
MMT_PREP_HD static inline StepPrepAt step_prep_at(const StepPrepMat& J, size_t i) {
    const int j = (int)(i & 7);
    const size_t r = i >> 3;
    const int n = (int)(r % J.rows), k = (int)(r / J.rows) * 8 + j;
    return {n, k, ((size_t)(k >> 3) * J.nout + n) * 8 + j};
}

// append a job; `most`: the largest number of elements of any matrix job so far (the grid's x)
static inline void step_prep_mat(StepPrepParams& P, size_t& most, const float* src, int ld, int col0, const float* src2, int ld2, int col2,
                                 size_t dst, int rows, int K, int nout) {
    StepPrepMat& J = P.mat[P.nmat++];
    J.src = src; J.src2 = src2; J.dst = dst; J.ld = ld; J.col0 = col0; J.ld2 = ld2; J.col2 = col2;
    J.rows = rows; J.K = K; J.KP = (K + 7) / 8 * 8; J.nout = nout;
    if ((size_t)rows * J.KP > most) most = (size_t)rows * J.KP;
}
static inline void step_prep_vec(StepPrepParams& P, const float* a, const float* b, size_t dst, int n) {
    StepPrepVec& J = P.vec[P.nvec++];
    J.a = a; J.b = b; J.dst = dst; J.n = n;
}

#if defined(__HIPCC__)
#include "common.h"

// Grid-stride over the destination; grid = min(grid_for(most), 64) x (nmat + nvec), 256 threads.
__global__ __launch_bounds__(256) void step_prep_kernel(const StepPrepParams P) {
    const int job = blockIdx.y;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (job < P.nmat) {
        const StepPrepMat& J = P.mat[job];
        bf16* dst = reinterpret_cast<bf16*>(P.state + J.dst);
        const size_t total = (size_t)J.rows * J.KP;
        for (size_t i = first; i < total; i += stride) {
            const StepPrepAt at = step_prep_at(J, i);
            float v = 0.f;
            if (at.k < J.K) {
                v = J.src[(size_t)at.n * J.ld + J.col0 + at.k];
                if (J.src2) v += J.src2[(size_t)at.n * J.ld2 + J.col2 + at.k];
            }
            dst[at.dst] = (bf16)v;
        }
    } else if (job - P.nmat < P.nvec) {
        const StepPrepVec& J = P.vec[job - P.nmat];
        float* dst = reinterpret_cast<float*>(P.state + J.dst);
        for (size_t i = first; i < (size_t)J.n; i += stride) dst[i] = J.b ? J.a[i] + J.b[i] : J.a[i];
    }
}
#endif
