// Stand-alone host check of the one-window encoder step's limits and state layout (csrc/encoder_step_plan.h): no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -o tools/bin/step_plan_check tools/step_plan_check.cpp && tools/bin/step_plan_check
// Walks the limits and their refused neighbours; for accepted shapes checks that the regions of the state are aligned, do not overlap
// and sum to the reported size, and, on a host buffer of exactly that size, touches every element the preparation kernel writes and
// the first and last cache elements a step can address, so that an offset or size mistake is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../multimodal_transformer_amd/csrc/encoder_step_plan.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static bool accepted(int B, int cap, int d, int h, int f, int N) {
    if (B <= 0 || cap <= 0 || d <= 0 || h <= 0 || f <= 0 || N <= 0) return false;
    if (N > 16 || d % h || d % 4 || f % 4 || d / h > 64 || d > 512 || f > 2048 || cap > 4096) return false;
    return h * ((d / h + 7) / 8 * 8) <= 2048;
}

// the element index the step kernel forms for (layer, K or V, b, head, position j, column e): encoder_step.h
static size_t cache_index(const StepPlan& P, int layer, int kv, int b, int head, int j, int e) {
    return (size_t)layer * P.cache_layer + (size_t)kv * P.cache_kv + (size_t)b * P.cache_seq + (size_t)head * P.cache_head + (size_t)j * P.dkp + e;
}

static void check_layout(int B, int cap, int d, int h, int f, int N, bool touch) {
    StepPlan P; const char* why = nullptr;
    EXPECT(step_plan(P, B, cap, d, h, f, N, &why) == MMT_STEP_OK);
    EXPECT(P.dk * h == d && P.dkp >= P.dk && P.dkp % 8 == 0 && P.dkp - P.dk < 8 && P.nchunk * 8 == P.dkp && P.nchunk <= 8);
    EXPECT(P.KPd >= d && P.KPd % 8 == 0 && P.KPd - d < 8 && P.KPf >= f && P.KPf % 8 == 0 && P.KPf - f < 8);
    EXPECT(P.HDKP == h * P.dkp && P.HDKP <= MMT_STEP_MAX_HDKP);
    const size_t rows[4] = {(size_t)3 * d, (size_t)d, (size_t)f, (size_t)d}, cols[4] = {(size_t)P.KPd, (size_t)P.KPd, (size_t)P.KPd, (size_t)P.KPf};
    size_t end = 0;
    for (int i = 0; i < 4; ++i) {
        EXPECT(P.w_elems[i] == rows[i] * cols[i]);
        EXPECT(P.w_off[i] >= end && (P.w_off[i] * 2) % 256 == 0);             // no overlap with the matrix before; 16-byte loads are aligned
        end = P.w_off[i] + P.w_elems[i];
    }
    EXPECT(P.w_layer_elems >= end && (P.w_layer_elems * 2) % 256 == 0);
    EXPECT(P.cache_off >= (size_t)N * P.w_layer_elems * 2 && P.cache_off % 256 == 0);
    EXPECT(P.cache_head == (size_t)cap * P.dkp && P.cache_seq == h * P.cache_head && P.cache_kv == B * P.cache_seq);
    EXPECT(P.cache_layer == 2 * P.cache_kv && P.cache_elems == (size_t)N * P.cache_layer);
    EXPECT(P.bytes >= P.cache_off + P.cache_elems * 2 && P.bytes - (P.cache_off + P.cache_elems * 2) < 256);
    EXPECT((P.dkp * 2) % 16 == 0);                                             // a cache row is whole 16-byte chunks
    EXPECT(cache_index(P, N - 1, 1, B - 1, h - 1, cap - 1, P.dkp - 1) == P.cache_elems - 1);
    const StepParamLayout L = step_param_layout(d, f, N);
    EXPECT(L.layer == (size_t)4 * ((size_t)d * d + d) + 2 * (size_t)f * d + f + d + 4 * (size_t)d && L.final_b == (size_t)N * L.layer + d);
    if (!touch) return;
    std::vector<unsigned short> st(P.bytes / 2);                               // bf16 elements: exactly the queried size
    EXPECT(st.size() * 2 == P.bytes);
    unsigned short* cache = st.data() + P.cache_off / 2;
    for (int layer = 0; layer < N; ++layer)                                    // what the preparation kernel writes: every weight element once
        for (int m = 0; m < 4; ++m) {
            unsigned short* w = st.data() + (size_t)layer * P.w_layer_elems + P.w_off[m];
            for (size_t i = 0; i < P.w_elems[m]; ++i) w[i] += 1;
        }
    for (int layer = 0; layer < N; ++layer)
        for (int m = 0; m < 4; ++m) {
            const unsigned short* w = st.data() + (size_t)layer * P.w_layer_elems + P.w_off[m];
            bool once = true;
            for (size_t i = 0; i < P.w_elems[m]; ++i) once = once && w[i] == 1;
            EXPECT(once);                                                      // an overlap of two matrices would read 2
        }
    for (int layer : {0, N - 1}) for (int kv : {0, 1}) for (int b : {0, B - 1}) for (int head : {0, h - 1}) for (int j : {0, cap - 1})
        for (int e : {0, P.dkp - 1}) cache[cache_index(P, layer, kv, b, head, j, e)] += 2;
    bool apart = true;                                                         // the cache does not reach back into the weights
    for (size_t i = 0; i < (size_t)N * P.w_layer_elems; ++i) apart = apart && st[i] <= 1;
    EXPECT(apart);
}

int main() {
    const char* why = nullptr;
    StepPlan P;
    // the limits and their neighbours, one dimension at a time around an accepted shape
    for (int d = -4; d <= 520; ++d)
        for (int h : {1, 2, 3, 4, 8, 16, 64, 128, 256, 512}) {
            const int rc = step_plan(P, 2, 16, d, h, 128, 2, &why);
            EXPECT((rc == MMT_STEP_OK) == accepted(2, 16, d, h, 128, 2));
            if (rc) EXPECT(why && strstr(why, "encoder stream"));
            else check_layout(2, 16, d, h, 128, 2, false);
        }
    for (int f = -4; f <= 2056; ++f) EXPECT((step_plan(P, 2, 16, 128, 8, f, 2, &why) == MMT_STEP_OK) == accepted(2, 16, 128, 8, f, 2));
    for (int N = -1; N <= 18; ++N) EXPECT((step_plan(P, 2, 16, 128, 8, 128, N, &why) == MMT_STEP_OK) == accepted(2, 16, 128, 8, 128, N));
    for (int cap : {-1, 0, 1, 2, 4095, 4096, 4097}) EXPECT((step_plan(P, 2, cap, 128, 8, 128, 2, &why) == MMT_STEP_OK) == accepted(2, cap, 128, 8, 128, 2));
    for (int B : {-1, 0, 1, 3, 1024}) EXPECT((step_plan(P, B, 16, 128, 8, 128, 2, &why) == MMT_STEP_OK) == accepted(B, 16, 128, 8, 128, 2));
    // the error class and the named limit
    EXPECT(step_plan(P, 0, 16, 128, 8, 128, 2, &why) == MMT_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(step_plan(P, 2, 4097, 128, 8, 128, 2, &why) == MMT_STEP_EUNSUPPORTED && strstr(why, "capacity > 4096"));
    EXPECT(step_plan(P, 2, 16, 256, 2, 128, 2, &why) == MMT_STEP_EUNSUPPORTED && strstr(why, "d_k > 64"));
    EXPECT(step_plan(P, 2, 16, 130, 8, 128, 2, &why) == MMT_STEP_EUNSUPPORTED && strstr(why, "divisible"));
    EXPECT(step_plan(P, 2, 16, 516, 129, 128, 2, &why) == MMT_STEP_EUNSUPPORTED && strstr(why, "512"));
    EXPECT(step_plan(P, 2, 16, 128, 8, 2052, 2, &why) == MMT_STEP_EUNSUPPORTED && strstr(why, "2048"));
    EXPECT(step_plan(P, 2, 16, 128, 8, 128, 17, &why) == MMT_STEP_EUNSUPPORTED && strstr(why, "n_layers"));
    EXPECT(step_plan(P, 2, 16, 512, 512, 128, 2, &why) == MMT_STEP_EUNSUPPORTED && strstr(why, "padded to 8"));
    // layouts with every element touched: the test shapes, padded widths (d = 36, f = 20: no multiples of 8), the small and far corners
    check_layout(1, 1, 32, 2, 128, 1, true);
    check_layout(3, 45, 40, 4, 128, 2, true);
    check_layout(3, 70, 128, 8, 128, 2, true);
    check_layout(3, 130, 64, 2, 128, 3, true);
    check_layout(2, 33, 256, 4, 128, 1, true);
    check_layout(1, 3, 512, 8, 128, 1, true);
    check_layout(2, 5, 36, 3, 20, 2, true);
    check_layout(2, 4096, 512, 256, 2048, 2, true);
    check_layout(32, 512, 128, 8, 128, 6, true);
    check_layout(4, 4096, 512, 8, 2048, 16, false);                            // the far corner: sizes only (0.3 GB of weights and 1 GB of cache)
    printf(fails ? "%d checks FAILED\n" : "step_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
