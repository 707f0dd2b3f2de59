// Stand-alone host check of the one-window MFN gate step's limits and state layout (csrc/mfn_step_plan.h): no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -o tools/bin/mfn_step_plan_check tools/mfn_step_plan_check.cpp && tools/bin/mfn_step_plan_check
// Walks the limits and their refused neighbours; for accepted shapes checks that the regions of the state are aligned, do not overlap
// and sum to the reported size, and, on a host buffer of exactly that size, walks the job table that mmt_mfn_stream_prepare launches
// (mfn_step_prep_table, through step_prep_walk.h: every weight and bias byte written exactly once, none elsewhere) and touches every word of
// the carried state a step can address, so that an offset or size mistake is a failed check or an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../multimodal_transformer_amd/csrc/mfn_step_plan.h"
#include "step_prep_walk.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static bool accepted(int B, int nm, const int* D, const int* H, int od) {
    if (B <= 0 || nm <= 0 || od <= 0) return false;
    if (nm > 4 || od > 256) return false;
    int sh = 0;
    for (int m = 0; m < nm; ++m) {
        if (D[m] <= 0 || H[m] <= 0 || D[m] % 4 || H[m] % 4 || D[m] > 512) return false;
        sh += H[m];
    }
    return sh <= 256;
}

typedef PrepRegion Region;

static void check_layout(int B, int nm, const int* D, const int* H, int od, bool touch) {
    MfnStepPlan P; const char* why = nullptr;
    EXPECT(mfn_step_plan(P, B, nm, D, H, od, &why) == MMT_MFN_STEP_OK);
    int sh = 0;
    for (int m = 0; m < nm; ++m) {
        EXPECT(P.D[m] == D[m] && P.H[m] == H[m] && P.hoff[m] == sh);
        EXPECT(P.KPD[m] >= D[m] && P.KPD[m] % 8 == 0 && P.KPD[m] - D[m] < 8 && P.KPH[m] >= H[m] && P.KPH[m] % 8 == 0 && P.KPH[m] - H[m] < 8);
        EXPECT(P.xoff[m] % 8 == 0 && P.hpoff[m] % 8 == 0);
        sh += H[m];
    }
    for (int m = nm; m < MMT_MFN_STEP_MAX_MODS; ++m) EXPECT(P.D[m] == 0 && P.H[m] == 0 && P.KPD[m] == 0 && P.KPH[m] == 0);
    EXPECT(P.nm == nm && P.SH == sh && P.A == 2 * sh && P.KL == sh + 128 && P.KPL >= P.KL && P.KPL % 8 == 0 && P.KPL - P.KL < 8 && P.OD == od);
    // the kernel's LDS rows: xs, hs, pre, cs, last (mfn_step.h)
    EXPECT(P.xoff[nm] <= MMT_MFN_STEP_MAX_MODS * MMT_MFN_STEP_MAX_IN && P.hpoff[nm] <= MMT_MFN_STEP_MAX_SH + 8 * MMT_MFN_STEP_MAX_MODS);
    EXPECT(4 * P.SH <= 4 * MMT_MFN_STEP_MAX_SH && P.A <= 2 * MMT_MFN_STEP_MAX_SH && P.KPL <= MMT_MFN_STEP_MAX_SH + MMT_MFN_STEP_MD + 8);
    EXPECT(P.w_k[MFN_W_A11] == P.A && P.w_rows[MFN_W_A12] == P.A && P.w_k[MFN_W_O1] == P.KL && P.w_kp[MFN_W_O1] == P.KPL && P.w_rows[MFN_W_O2] == od);
    // every region, in bytes
    std::vector<Region> R;
    for (int m = 0; m < nm; ++m) {
        R.push_back({P.wih[m], (size_t)4 * H[m] * P.KPD[m] * 2});
        R.push_back({P.whh[m], (size_t)4 * H[m] * P.KPH[m] * 2});
        R.push_back({P.blstm[m], (size_t)4 * H[m] * 4});
    }
    for (int i = 0; i < MFN_W_COUNT; ++i) {
        EXPECT(P.w_kp[i] >= P.w_k[i] && P.w_kp[i] % 8 == 0 && P.w_kp[i] - P.w_k[i] < 8);
        R.push_back({P.w[i], (size_t)P.w_rows[i] * P.w_kp[i] * 2});
    }
    for (int i = 0; i < MFN_B_COUNT; ++i) R.push_back({P.b[i], (size_t)P.b_n[i] * 4});
    EXPECT(P.seq_floats == (size_t)2 * sh + 128 && P.dyn_floats == (size_t)2 * B * P.seq_floats);
    R.push_back({P.dyn_off, P.dyn_floats * 4});
    std::sort(R.begin(), R.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
    size_t end = 0, used = 0;
    for (const Region& r : R) {
        EXPECT(r.off % 256 == 0 && r.off >= end && r.len > 0);                 // aligned, disjoint
        EXPECT(r.off - end < 256);                                             // and nothing but alignment between two of them
        end = r.off + r.len;
        used += (r.len + 255) / 256 * 256;
    }
    EXPECT(R.front().off == 0 && used == P.bytes && P.bytes >= end && P.bytes - end < 256);       // they sum to the size
    if (!touch) return;
    std::vector<unsigned char> st(P.bytes);                                    // exactly the queried size: counts the writes of a byte
    // what the preparation writes: the table the entry launches, with sources that are never dereferenced
    static const float some = 0.f;
    const float* lp[4 * MMT_MFN_STEP_MAX_MODS]; const float* gp[20];
    for (const float*& q : lp) q = &some;
    for (const float*& q : gp) q = &some;
    StepPrepParams T; size_t most = 0;
    mfn_step_prep_table(P, lp, gp, T, most);
    EXPECT(T.nmat == 2 * nm + 12 && T.nvec == nm + 10);
    R.pop_back();                                                              // the carried state: the last region, never prepared
    fails += step_prep_walk(T, most, R, P.dyn_off, st.data());
    for (size_t i = P.dyn_off; i < P.bytes; ++i) EXPECT(st[i] == 0);
    // every word of either copy of the carried state
    float* dyn = reinterpret_cast<float*>(st.data() + P.dyn_off);
    for (int t : {0, 1, 2, 2147483647}) for (int b : {0, B - 1}) {
        float* in = dyn + ((size_t)(t & 1) * B + b) * P.seq_floats;
        float* out = dyn + ((size_t)((t & 1) ^ 1) * B + b) * P.seq_floats;
        EXPECT(in != out);
        for (size_t i = 0; i < P.seq_floats; ++i) { in[i] = 1.f; out[i] = 2.f; }
    }
}

int main() {
    const char* why = nullptr;
    MfnStepPlan P;
    const int D2[2] = {16, 16}, H2[2] = {48, 16};
    // the limits and their neighbours, one dimension at a time around an accepted shape
    for (int d = -4; d <= 520; ++d) { const int D[2] = {d, 16}; EXPECT((mfn_step_plan(P, 2, 2, D, H2, 1, &why) == MMT_MFN_STEP_OK) == accepted(2, 2, D, H2, 1)); }
    for (int h = -4; h <= 260; ++h) {
        const int H[2] = {h, 16};
        const int rc = mfn_step_plan(P, 2, 2, D2, H, 1, &why);
        EXPECT((rc == MMT_MFN_STEP_OK) == accepted(2, 2, D2, H, 1));
        if (rc) EXPECT(why && strstr(why, "mfn stream"));
        else check_layout(2, 2, D2, H, 1, false);
    }
    for (int h = 56; h <= 72; ++h) {                                            // the sum of four: 3 x 64 + h against 256
        const int D[4] = {16, 16, 16, 16}, H[4] = {64, 64, 64, h};
        EXPECT((mfn_step_plan(P, 2, 4, D, H, 1, &why) == MMT_MFN_STEP_OK) == accepted(2, 4, D, H, 1));
    }
    for (int od = -1; od <= 260; ++od) EXPECT((mfn_step_plan(P, 2, 2, D2, H2, od, &why) == MMT_MFN_STEP_OK) == accepted(2, 2, D2, H2, od));
    for (int nm = -1; nm <= 6; ++nm) {
        const int D[6] = {16, 16, 16, 16, 16, 16}, H[6] = {16, 16, 16, 16, 16, 16};
        EXPECT((mfn_step_plan(P, 2, nm, D, H, 1, &why) == MMT_MFN_STEP_OK) == accepted(2, nm, D, H, 1));
    }
    for (int B : {-1, 0, 1, 3, 1024}) EXPECT((mfn_step_plan(P, B, 2, D2, H2, 1, &why) == MMT_MFN_STEP_OK) == accepted(B, 2, D2, H2, 1));
    // the error class and the named limit
    EXPECT(mfn_step_plan(P, 0, 2, D2, H2, 1, &why) == MMT_MFN_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(mfn_step_plan(P, 2, 2, nullptr, H2, 1, &why) == MMT_MFN_STEP_EINVAL && strstr(why, "null"));
    EXPECT(mfn_step_plan(P, 2, 5, D2, H2, 1, &why) == MMT_MFN_STEP_EUNSUPPORTED && strstr(why, "4 modalities"));
    EXPECT(mfn_step_plan(P, 2, 2, D2, H2, 257, &why) == MMT_MFN_STEP_EUNSUPPORTED && strstr(why, "output_dim > 256"));
    { const int D[2] = {18, 16}; EXPECT(mfn_step_plan(P, 2, 2, D, H2, 1, &why) == MMT_MFN_STEP_EUNSUPPORTED && strstr(why, "input widths must be multiples of 4")); }
    { const int D[2] = {516, 16}; EXPECT(mfn_step_plan(P, 2, 2, D, H2, 1, &why) == MMT_MFN_STEP_EUNSUPPORTED && strstr(why, "input width > 512")); }
    { const int H[2] = {50, 16}; EXPECT(mfn_step_plan(P, 2, 2, D2, H, 1, &why) == MMT_MFN_STEP_EUNSUPPORTED && strstr(why, "hidden sizes must be multiples of 4")); }
    { const int H[2] = {244, 16}; EXPECT(mfn_step_plan(P, 2, 2, D2, H, 1, &why) == MMT_MFN_STEP_EUNSUPPORTED && strstr(why, "hidden sizes > 256")); }
    { const int D[2] = {0, 16}; EXPECT(mfn_step_plan(P, 2, 2, D, H2, 1, &why) == MMT_MFN_STEP_EINVAL && strstr(why, "non-positive")); }
    // layouts with every element touched: the test shapes, padded widths (12, 20: no multiples of 8), the small and far corners
    { const int D[1] = {8}, H[1] = {16}; check_layout(1, 1, D, H, 1, true); }
    { const int D[2] = {12, 16}, H[2] = {48, 16}; check_layout(3, 2, D, H, 1, true); }
    { const int D[3] = {40, 24, 32}, H[3] = {88, 48, 88}; check_layout(3, 3, D, H, 1, true); }
    { const int D[4] = {256, 16, 256, 256}, H[4] = {88, 16, 48, 88}; check_layout(2, 4, D, H, 1, true); check_layout(32, 4, D, H, 1, true); }
    { const int D[2] = {16, 16}, H[2] = {48, 16}; check_layout(33, 2, D, H, 1, true); }
    { const int D[2] = {20, 4}, H[2] = {4, 12}; check_layout(2, 2, D, H, 3, true); }
    { const int D[4] = {512, 512, 512, 512}, H[4] = {64, 64, 64, 64}; check_layout(4096, 4, D, H, 256, true); }
    { const int D[1] = {512}, H[1] = {256}; check_layout(1, 1, D, H, 256, true); }
    printf(fails ? "%d checks FAILED\n" : "mfn_step_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
