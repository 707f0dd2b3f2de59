// Limits, padding and workspace layout of the stacked LSTM scan (scan_stack.h): plain host C++ with no HIP in it, so that a stand-alone
// program can exercise it (tools/stack_plan_check.cpp) and api.hip only adds the base pointer to the offsets computed here.
#pragma once
#include <stddef.h>

#define MMT_STACK_MIN_L 2
#define MMT_STACK_MAX_L 4
#define MMT_STACK_MAX_H 128
#define MMT_STACK_MAX_B 512

struct StackPlan {
    int HP16, HPAD, NR;             // units padded to MFMA tiles / to the k-block granule of a half; sequences per workgroup
    int grid, block;
    size_t pf_off, pf_elems;        // forward fragments  [L][4 gates][HP16 units][2 HPAD: x_a half | x_b half]   (bf16 elements)
    size_t pb_off, pb_elems;        // backward fragments [L][2 halves][HP16 units][4 HPAD: gate-major]
    size_t bytes;
};

// Shape limits only (T and B may be 0 for the workspace query).  why: a static string naming the limit that was exceeded.
static inline bool stack_limits_ok(int H, int L, const char** why) {
    if (L < MMT_STACK_MIN_L || L > MMT_STACK_MAX_L) { *why = "stacked LSTM scan: layers not in [2,4]"; return false; }
    if (H <= 0 || H > MMT_STACK_MAX_H) { *why = "stacked LSTM scan: hidden size not in [4,128]"; return false; }
    if (H % 4) { *why = "stacked LSTM scan: hidden size must be a multiple of 4"; return false; }
    return true;
}

static inline size_t stack_align256(size_t n) { return (n + 255) / 256 * 256; }

// B == 0: the workspace query (layout only).  Returns false with *why set when the shape is outside the limits.
static inline bool stack_plan(StackPlan& P, int T, int B, int H, int L, bool query, const char** why) {
    if (!stack_limits_ok(H, L, why)) return false;
    if (!query) {
        if (T <= 0 || B <= 0) { *why = "stacked LSTM scan: non-positive T or B"; return false; }
        if (B > MMT_STACK_MAX_B) { *why = "stacked LSTM scan: batch > 512"; return false; }
    }
    P.HP16 = (H + 15) / 16 * 16;
    P.HPAD = P.HP16 <= 64 ? 64 : 128;
    P.NR = B > 256 ? 2 : 1;                                     // one sequence per workgroup up to 256 workgroups, else two
    P.grid = query ? 0 : (B + P.NR - 1) / P.NR;
    P.block = 64 * (P.HP16 / 16);
    P.pf_elems = (size_t)L * 4 * P.HP16 * 2 * P.HPAD;
    P.pb_elems = (size_t)L * 2 * P.HP16 * 4 * P.HPAD;
    P.pf_off = 0;
    P.pb_off = stack_align256(P.pf_elems * 2);
    P.bytes = P.pb_off + stack_align256(P.pb_elems * 2);
    return true;
}
