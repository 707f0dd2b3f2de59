// Building blocks shared by the scan kernels: the general LSTM scans (scan.h), the units form (scan_units.h), the half-resident and
// four-CU scans for H > 128 (scan256.h, scan_cluster.h) and the MFN memory scans (mfn_scan.h).
//
// Every helper is forced inline, and a kernel calls one only where it then compiles to exactly the gfx950 instructions it has with the
// text written out: the scans are latency-bound instruction streams, and hipcc's block layout and schedule of these
// kernels move with where a loop or a barrier is written.  That is why the ring loop, the cell forward, the recurrent MFMA loops and the
// cooperative loaders are still written out per kernel, and why a few kernels keep a prologue loop that their siblings take from here.
// Gate order i, f, g, o (torch) everywhere.
#pragma once
#include "common.h"

__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + fast_exp2(-1.4426950408889634f * x)); }
__device__ __forceinline__ float tanh_f(float x) { return 2.0f * sigmoid_f(2.0f * x) - 1.0f; }
// store to a wave-uniform base plus a 32-bit BYTE offset per lane as ONE instruction (`global_store_dword voff, vdata, s[base]`).
// hipcc forms the 64-bit address in vector registers instead (a v_lshl_add_u64 per store: 6 of a forward step's ~120 instructions, and
// a wave of these scans issues roughly one instruction per 10 cycles).  The stored values are many instructions old (the stores sit
// behind the step's barrier), so no hazard the assembler statement would hide from the compiler applies.
__device__ __forceinline__ void st_uniform(float* base, unsigned byte_off, float v) {
    asm volatile("global_store_dword %0, %1, %2" :: "v"(byte_off), "v"(v), "s"(base) : "memory");
}

// ---- prologue fragments
// a[k] = the 8 bf16 at p + 32 k: one lane's MFMA fragments of consecutive k-blocks of a weight row
template <int N>
__device__ __forceinline__ void load_wfrags(bf16x8 (&a)[N], const bf16* p) {
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = *reinterpret_cast<const bf16x8*>(p + k * 32);
}
// zero an LDS tile with the whole workgroup (no barrier) / and wait for it
__device__ __forceinline__ void lds_zero(bf16* buf, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) buf[i] = (bf16)0.f;
}
__device__ __forceinline__ void lds_clear(bf16* buf, int n) {
    lds_zero(buf, n);
    __syncthreads();
}

// ---- LSTM cell, backward, one unit per lane (scan256.h, scan_cluster.h).
// Backward of one unit at one step: dh_rec / dc carried from step t + 1, dhe / dce the external gradients; gate pre-activation
// gradients out, dc updated.  Selects, not products with 0: a dead lane's dh comes from rows that are not weights and may hold anything.
__device__ __forceinline__ void lstm_cell_bwd(bool lived, float ig, float fg, float gg, float og, float ct, float cp, float dh_rec, float dhe,
                                              float dce, float& dc, float& dgi, float& dgf, float& dgg, float& dgo) {
    const float dh = dh_rec + dhe;
    const float th = tanh_f(ct);
    const float dct = dc + dce + dh * og * (1.f - th * th);
    dgo = lived ? dh * th * og * (1.f - og) : 0.f;
    dgi = lived ? dct * gg * ig * (1.f - ig) : 0.f;
    dgf = lived ? dct * cp * fg * (1.f - fg) : 0.f;
    dgg = lived ? dct * ig * (1.f - gg * gg) : 0.f;
    dc = lived ? dct * fg : 0.f;
}
