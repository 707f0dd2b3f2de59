// Stand-alone host check of the one-window decoder step's limits and state layout (csrc/decoder_step_plan.h): no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -o tools/bin/decoder_step_plan_check tools/decoder_step_plan_check.cpp && tools/bin/decoder_step_plan_check
// Walks the limits and their refused neighbours; for accepted shapes checks that the regions of the state are aligned, do not overlap
// and sum to the reported size, and, on a host buffer of exactly that size, walks the job table that mmt_decoder_stream_prepare launches
// (decoder_step_prep_table, through step_prep_walk.h: every weight and vector byte written exactly once, none elsewhere) and touches both
// copies of the carried state for the first and last (b, layer), at the positions slot_decode lets through, so that an offset or size
// mistake is a failed check or an AddressSanitizer report.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../multimodal_transformer_amd/csrc/decoder_step_plan.h"
#include "../multimodal_transformer_amd/csrc/step_slots.h"
#include "step_prep_walk.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static bool accepted(int B, int d, int hd, int L) {
    return B >= 1 && d >= 4 && d <= 512 && d % 4 == 0 && hd >= 1 && hd <= 512 && L >= 0 && L <= 4;
}

typedef PrepRegion Region;

static void check_layout(int B, int d, int hd, int L, bool touch) {
    DecStepPlan P; const char* why = nullptr;
    EXPECT(decoder_step_plan(P, B, d, hd, L, &why) == MMT_DEC_STEP_OK);
    EXPECT(P.d == d && P.hdim == hd && P.L == L);
    EXPECT(P.KPd >= d && P.KPd % 8 == 0 && P.KPd - d < 8 && P.KPh >= hd && P.KPh % 8 == 0 && P.KPh - hd < 8);
    // the kernel's LDS rows: es, hp, hc, pre, hid (decoder_step.h)
    EXPECT(P.KPd <= MMT_DEC_STEP_MAX_D && P.KPh <= MMT_DEC_STEP_MAX_HDIM && L <= MMT_DEC_STEP_MAX_L);
    // every region, in bytes; the matrices first, with their rows and padded k
    struct Mat { size_t off; int rows, kp; };
    std::vector<Mat> M;
    if (L) M.push_back({P.wx, 4 * d, P.KPd});
    for (int l = 0; l < L; ++l) { M.push_back({P.wa[l], 4 * d, P.KPd}); M.push_back({P.wb[l], 4 * d, P.KPd}); }
    M.push_back({P.w1, hd, P.KPd});
    M.push_back({P.w2, 1, P.KPh});
    std::vector<Region> R;
    for (const Mat& m : M) R.push_back({m.off, (size_t)m.rows * m.kp * 2});
    for (int l = 0; l < L; ++l) R.push_back({P.bl[l], (size_t)4 * d * 4});
    R.push_back({P.b1, (size_t)hd * 4});
    R.push_back({P.b2, 4});
    if (L) { R.push_back({P.h0, (size_t)L * d * 4}); R.push_back({P.c0, (size_t)L * d * 4}); }
    EXPECT(P.seq_floats == (size_t)2 * L * d && P.dyn_floats == (size_t)2 * B * P.seq_floats);
    if (L) R.push_back({P.dyn_off, P.dyn_floats * 4});
    std::sort(R.begin(), R.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
    size_t end = 0, used = 0;
    for (const Region& r : R) {
        EXPECT(r.off % 256 == 0 && r.off >= end && r.len > 0);                 // aligned, disjoint
        EXPECT(r.off - end < 256);                                             // and nothing but alignment between two of them
        end = r.off + r.len;
        used += (r.len + 255) / 256 * 256;
    }
    EXPECT(R.front().off == 0 && used == P.bytes && P.bytes >= end && P.bytes - end < 256);       // they sum to the size
    EXPECT(P.dyn_off % 256 == 0 && P.dyn_off + P.dyn_floats * 4 <= P.bytes);
    if (!touch) return;
    std::vector<unsigned char> st(P.bytes);                                    // exactly the queried size: counts the writes of a byte
    // what the preparation writes: the table the entry launches, with sources that are never dereferenced
    static const float some = 0.f;
    const float* lp[4 * MMT_DEC_STEP_MAX_L];
    for (const float*& q : lp) q = &some;
    StepPrepParams T; size_t most = 0;
    decoder_step_prep_table(P, lp, &some, &some, &some, &some, &some, &some, T, most);
    EXPECT(T.nmat == (L ? 3 + 2 * L : 2) && T.nvec == (L ? 4 + L : 2));
    if (L) R.pop_back();                                                       // the carried state: the last region, never prepared
    fails += step_prep_walk(T, most, R, P.dyn_off, st.data());
    for (size_t i = P.dyn_off; i < P.bytes; ++i) EXPECT(st[i] == 0);
    // both copies of the carried state for the first and last (b, layer), at every position slot_decode lets through
    float* dyn = reinterpret_cast<float*>(st.data() + P.dyn_off);
    for (int p : {0, 1, 2, INT_MAX - 1, INT_MAX, -1, INT_MIN}) {
        const int t = slot_decode(p, 0);
        if (t == MMT_SLOT_SKIP) continue;
        for (int b : {0, B - 1}) for (int l : {0, L - 1}) {
            if (L == 0) continue;                                              // no carried state at all
            float* in = dyn + ((size_t)(t & 1) * B + b) * P.seq_floats + (size_t)l * 2 * d;
            float* out = dyn + ((size_t)((t & 1) ^ 1) * B + b) * P.seq_floats + (size_t)l * 2 * d;
            EXPECT(in != out);
            for (int i = 0; i < 2 * d; ++i) { in[i] = 1.f; out[i] = 2.f; }     // h (d) | c (d)
        }
    }
}

int main() {
    const char* why = nullptr;
    DecStepPlan P;
    // the limits and their neighbours, one dimension at a time around an accepted shape
    for (int d = -4; d <= 520; ++d) {
        const int rc = decoder_step_plan(P, 2, d, 128, 1, &why);
        EXPECT((rc == MMT_DEC_STEP_OK) == accepted(2, d, 128, 1));
        if (rc) EXPECT(why && strstr(why, "decoder stream"));
        else check_layout(2, d, 128, 2, false);
    }
    for (int hd = -1; hd <= 516; ++hd) {
        const int rc = decoder_step_plan(P, 2, 40, hd, 1, &why);
        EXPECT((rc == MMT_DEC_STEP_OK) == accepted(2, 40, hd, 1));
        if (!rc) check_layout(2, 40, hd, 1, false);
    }
    for (int L = -1; L <= 6; ++L) EXPECT((decoder_step_plan(P, 2, 40, 32, L, &why) == MMT_DEC_STEP_OK) == accepted(2, 40, 32, L));
    for (int B : {-1, 0, 1, 3, 1024}) EXPECT((decoder_step_plan(P, B, 40, 32, 1, &why) == MMT_DEC_STEP_OK) == accepted(B, 40, 32, 1));
    // the error class and the named limit
    EXPECT(decoder_step_plan(P, 0, 40, 32, 1, &why) == MMT_DEC_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(decoder_step_plan(P, 2, 0, 32, 1, &why) == MMT_DEC_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(decoder_step_plan(P, 2, 40, 0, 1, &why) == MMT_DEC_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(decoder_step_plan(P, 2, 40, 32, -1, &why) == MMT_DEC_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(decoder_step_plan(P, 2, 40, 32, 5, &why) == MMT_DEC_STEP_EUNSUPPORTED && strstr(why, "n_layers > 4"));
    EXPECT(decoder_step_plan(P, 2, 42, 32, 1, &why) == MMT_DEC_STEP_EUNSUPPORTED && strstr(why, "multiple of 4"));
    EXPECT(decoder_step_plan(P, 2, 516, 32, 1, &why) == MMT_DEC_STEP_EUNSUPPORTED && strstr(why, "embed_dim > 512"));
    EXPECT(decoder_step_plan(P, 2, 40, 513, 1, &why) == MMT_DEC_STEP_EUNSUPPORTED && strstr(why, "h_dim > 512"));
    // layouts with every element touched: the test shapes (12, 20: no multiples of 8), the small and far corners
    check_layout(1, 8, 4, 1, true);
    check_layout(3, 12, 20, 1, true);
    check_layout(3, 40, 128, 1, true);
    check_layout(2, 128, 128, 2, true);
    check_layout(2, 64, 32, 4, true);
    check_layout(2, 256, 128, 1, true);
    check_layout(1, 512, 512, 1, true);
    check_layout(2, 16, 8, 0, true);
    check_layout(33, 16, 8, 1, true);
    check_layout(1, 4, 1, 0, true);
    check_layout(1, 4, 1, 4, true);
    check_layout(256, 512, 512, 4, true);
    check_layout(32, 128, 128, 1, true);
    printf(fails ? "%d checks FAILED\n" : "decoder_step_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
