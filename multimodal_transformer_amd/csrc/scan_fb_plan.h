// Limits, padding and workspace layout of the LSTM scan with the read-out MLP in its recurrence (scan_fb.h): plain host C++ with no HIP
// in it, so that a stand-alone program can exercise it (tools/fb_plan_check.cpp) and api.hip only adds the base pointer to the offsets
// computed here.
#pragma once
#include <stddef.h>

#define MMT_FB_MAX_H 128
#define MMT_FB_MAX_E 128
#define MMT_FB_MAX_B 512

struct FbPlan {
    int HP16, HPAD, NW;             // units padded to MFMA tiles / to the k-block granule; waves of a workgroup (one 16-unit tile each)
    int ES, ER;                     // MLP row tiles per wave (1, 2, 4 or 8; tile s of wave w holds rows (s NW + w) 16 ..), rows of the W1 fragments = 16 ES NW >= E
    int EK, KE;                     // E rounded up to the backward's k-block (32), and EK / 32
    int NR, grid, block;            // sequences per workgroup
    size_t wf_off, wf_elems;        // forward  W_hh fragments [4 gates][HP16 units][HPAD]      (bf16 elements)
    size_t wb_off, wb_elems;        // backward W_hh fragments [HP16 units][4 HPAD: gate-major]
    size_t w1f_off, w1f_elems;      // forward  W1 fragments   [ER MLP rows][HPAD]
    size_t w1b_off, w1b_elems;      // backward W1 fragments   [HP16 units][EK]
    size_t bytes;
};

// Shape limits only.  why: a static string naming the limit that was exceeded.
static inline bool fb_limits_ok(int H, int E, const char** why) {
    if (H < 4 || H > MMT_FB_MAX_H) { *why = "feedback LSTM scan: hidden size not in [4,128]"; return false; }
    if (H % 4) { *why = "feedback LSTM scan: hidden size must be a multiple of 4"; return false; }
    if (E < 4 || E > MMT_FB_MAX_E) { *why = "feedback LSTM scan: read-out width not in [4,128]"; return false; }
    if (E % 4) { *why = "feedback LSTM scan: read-out width must be a multiple of 4"; return false; }
    return true;
}

static inline size_t fb_align256(size_t n) { return (n + 255) / 256 * 256; }

// query: the workspace query (layout only; T and B are not looked at).  Returns false with *why set when the shape is outside the limits.
static inline bool fb_plan(FbPlan& P, int T, int B, int H, int E, bool query, const char** why) {
    if (!fb_limits_ok(H, E, why)) return false;
    if (!query) {
        if (T <= 0 || B <= 0) { *why = "feedback LSTM scan: non-positive T or B"; return false; }
        if (B > MMT_FB_MAX_B) { *why = "feedback LSTM scan: batch > 512"; return false; }
    }
    P.HP16 = (H + 15) / 16 * 16;
    P.HPAD = P.HP16 <= 64 ? 64 : 128;
    P.NW = P.HP16 / 16;
    const int tiles = (E + 15) / 16, per_wave = (tiles + P.NW - 1) / P.NW;
    P.ES = 1;
    while (P.ES < per_wave) P.ES *= 2;
    P.ER = 16 * P.ES * P.NW;
    P.EK = (E + 31) / 32 * 32;
    P.KE = P.EK / 32;
    P.NR = (!query && B > 256) ? 2 : 1;                         // one sequence per workgroup up to 256 workgroups, else two
    P.grid = query ? 0 : (B + P.NR - 1) / P.NR;
    P.block = 64 * P.NW;
    P.wf_elems = (size_t)4 * P.HP16 * P.HPAD;
    P.wb_elems = (size_t)P.HP16 * 4 * P.HPAD;
    P.w1f_elems = (size_t)P.ER * P.HPAD;
    P.w1b_elems = (size_t)P.HP16 * P.EK;
    P.wf_off = 0;
    P.wb_off = P.wf_off + fb_align256(P.wf_elems * 2);
    P.w1f_off = P.wb_off + fb_align256(P.wb_elems * 2);
    P.w1b_off = P.w1f_off + fb_align256(P.w1f_elems * 2);
    P.bytes = P.w1b_off + fb_align256(P.w1b_elems * 2);
    return true;
}
