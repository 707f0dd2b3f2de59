// Stand-alone host check of the ring rule (csrc/step_ring.h) of the banded stream: no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/bin/ring_plan_check tools/ring_plan_check.cpp && tools/bin/ring_plan_check
// The ring step kernels address a cache of `span` rows with values computed from the position t, which has no upper limit below
// INT_MAX.  This program walks the rule as encoder_step.h applies it, for every span in 1..70 and the two largest (4095, 4096), over
// three ranges of t: the first 3 span + 2 steps, the steps around 4096 (the plain stream's last capacity), and the last 3 span
// positions below INT_MAX.  It keeps one tag per row, the position whose K/V the row holds, exactly as the steps before t left it, and
// checks for each step that
//   * every row the sweep reads (age i = 0 .. n - 1) holds position t - n + i, and is below span;
//   * the rows read are distinct;
//   * the row written is none of them, is below span, and is t mod span;
//   * no intermediate overflows: the arithmetic is that of the header, on int, under -fsanitize=undefined, and r0 + i < 2 span;
//   * the slots form's p + 1 is INT_MAX at most, a value slot_decode never runs;
//   * a buffer of exactly mmt_encoder_stream_bytes(B, span, ...) holds the rows touched (AddressSanitizer).
#include <limits.h>
#include <stdio.h>
#include <vector>
#include "../multimodal_transformer_amd/csrc/step_ring.h"
#include "../multimodal_transformer_amd/csrc/encoder_step_plan.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { if (fails < 20) printf("FAILED %s (line %d; span %d, t %d)\n", #c, __LINE__, g_span, g_t); ++fails; } } while (0)
static int g_span = 0, g_t = 0;

// the tags as the steps before t left them: row r holds the largest position j < t with j mod span == r, or -1
static void tags_before(std::vector<long long>& tag, int t, int span) {
    for (int r = 0; r < span; ++r) tag[r] = -1;
    const long long first = (long long)t - span < 0 ? 0 : (long long)t - span;
    for (long long j = first; j < t; ++j) tag[(size_t)(j % span)] = j;
}

// one step, as encoder_step_body<*, true> forms its rows; then the write
static void step(std::vector<long long>& tag, std::vector<int>& seen, int t, int span) {
    g_t = t;
    EXPECT(slot_decode(t, 0) == t);                                            // a ring has no limit: every 0 <= t < INT_MAX runs
    const int n = ring_keys(t, span);
    EXPECT(n >= 0 && n <= span - 1 && n <= t && (n == t || n == span - 1));
    const int r0 = ring_first_row(t, n, span);
    EXPECT(r0 >= 0 && r0 < span);
    for (int i = 0; i < n; ++i) {
        EXPECT(r0 + i < 2 * span && 2 * span <= 2 * MMT_STEP_MAX_CAPACITY);
        const int row = ring_row(r0, i, span);
        EXPECT(row >= 0 && row < span);
        if (row < 0 || row >= span) continue;
        EXPECT(tag[row] == (long long)t - n + i);                              // age i is position t - n + i
        EXPECT(seen[row] != t);                                                // distinct
        seen[row] = t;
    }
    const int wrow = ring_row(r0, n, span);
    EXPECT(wrow >= 0 && wrow < span && wrow == t % span);
    if (wrow < 0 || wrow >= span) return;
    EXPECT(seen[wrow] != t);                                                   // never among the rows read in this step
    EXPECT(n < span - 1 || tag[wrow] == (long long)t - span || span == 1);     // it held the position that left the band
    tag[wrow] = t;
    const int next = t + 1;                                                    // what the slots kernel stores; signed, checked
    EXPECT(next > 0 && (next < INT_MAX || slot_decode(next, 0) == MMT_SLOT_SKIP));
}

static void walk(int span, long long from, long long to) {                     // t in [from, to]
    if (from < 0) from = 0;
    if (to > (long long)INT_MAX - 1) to = (long long)INT_MAX - 1;
    std::vector<long long> tag(span);
    std::vector<int> seen(span, -1);
    tags_before(tag, (int)from, span);
    for (long long t = from; t <= to; ++t) step(tag, seen, (int)t, span);
}

// the rows of a step inside a state of exactly the queried size
static void check_state(int span, int t) {
    StepPlan P; const char* why = nullptr;
    const int B = 2, d = 40, h = 4, f = 128, N = 2;
    EXPECT(step_plan(P, B, span, d, h, f, N, &why) == MMT_STEP_OK);
    std::vector<unsigned short> st(P.bytes / 2);
    unsigned short* cache = st.data() + P.cache_off / 2;
    const int n = ring_keys(t, span), r0 = ring_first_row(t, n, span);
    for (int i = 0; i <= n; ++i)
        for (int layer : {0, N - 1}) for (int kv : {0, 1}) for (int b : {0, B - 1}) for (int head : {0, h - 1}) {
            unsigned short* row = cache + (size_t)layer * P.cache_layer + (size_t)kv * P.cache_kv + (size_t)b * P.cache_seq
                                  + (size_t)head * P.cache_head + (size_t)ring_row(r0, i, span) * P.dkp;
            row[0] += 1; row[P.dkp - 1] += 1;
            EXPECT((size_t)(row - cache) + P.dkp <= P.cache_elems);
        }
    bool apart = true;                                                         // nothing landed in the weights
    for (size_t i = 0; i < P.cache_off / 2; ++i) apart = apart && st[i] == 0;
    EXPECT(apart);
}

int main() {
    std::vector<int> spans;
    for (int s = 1; s <= 70; ++s) spans.push_back(s);
    spans.push_back(MMT_STEP_MAX_CAPACITY - 1);
    spans.push_back(MMT_STEP_MAX_CAPACITY);
    for (int span : spans) {
        g_span = span;
        walk(span, 0, 3LL * span + 2);
        walk(span, 4096 - 2LL * span - 2, 4096 + 2LL * span + 2);
        walk(span, (long long)INT_MAX - 3LL * span, (long long)INT_MAX - 1);
        for (int t : {0, span - 1, span, 4096, INT_MAX - 1}) check_state(span, t);
    }
    {   // a span above the limit is refused with the capacity's message
        StepPlan P; const char* why = "";
        g_span = MMT_STEP_MAX_CAPACITY + 1;
        EXPECT(step_plan(P, 1, MMT_STEP_MAX_CAPACITY + 1, 40, 4, 128, 2, &why) == MMT_STEP_EUNSUPPORTED);
    }
    printf(fails ? "%d checks FAILED\n" : "ring_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
