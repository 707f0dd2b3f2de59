// Stand-alone host check of the slot decode (csrc/step_slots.h) against the state layouts of both step kernels: no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -o tools/bin/slot_pos_check tools/slot_pos_check.cpp && tools/bin/slot_pos_check
// The positioned step kernels form addresses from a value they read from device memory.  slot_decode is the one gate such a value
// passes, so this program walks it over the edge values of an int around every limit and, on host buffers of exactly the queried
// state sizes, touches what a kernel would address with a position the decode let through: the first and last element of cache row
// t of every (layer, K | V, b, head) for the encoder, the copy t & 1 of the carried state for the gate.  A position that should have
// been refused is then an AddressSanitizer report, and p + 1 that overflows an UndefinedBehaviorSanitizer report.
#include <limits.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../multimodal_transformer_amd/csrc/step_slots.h"
#include "../multimodal_transformer_amd/csrc/encoder_step_plan.h"
#include "../multimodal_transformer_amd/csrc/mfn_step_plan.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

// what the kernels do after the last stage when advance is set: signed addition, checked by -fsanitize=undefined
static int advanced(int t) { return t + 1; }

static std::vector<int> edge_values(int limit) {
    std::vector<int> v = {INT_MIN, INT_MIN + 1, -2, -1, 0, 1, INT_MAX - 1, INT_MAX};
    if (limit > 0) for (int p : {limit - 1, limit, limit < INT_MAX ? limit + 1 : limit}) v.push_back(p);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

// the decode itself: skip exactly for p < 0, p >= limit (limit > 0) and p == INT_MAX; otherwise the identity
static void check_decode(int limit) {
    for (int p : edge_values(limit)) {
        const int t = slot_decode(p, limit);
        const bool skip = p < 0 || p == INT_MAX || (limit > 0 && p >= limit);
        EXPECT((t == MMT_SLOT_SKIP) == skip);
        if (t == MMT_SLOT_SKIP) continue;
        EXPECT(t == p && t >= 0 && t < INT_MAX && (limit <= 0 || t < limit));
        const int n = advanced(t);
        EXPECT(n == t + 1 && n > 0);                                           // INT_MAX at most: a value the next launch skips
        EXPECT(n < INT_MAX || slot_decode(n, limit) == MMT_SLOT_SKIP);
    }
}

// the encoder: cache row t of every (layer, K | V, b, head), formed as encoder_step.h forms it, on a buffer of the queried size
static void check_encoder(int B, int cap, int d, int h, int f, int N) {
    StepPlan P; const char* why = nullptr;
    EXPECT(step_plan(P, B, cap, d, h, f, N, &why) == MMT_STEP_OK);
    std::vector<unsigned short> st(P.bytes / 2);                               // bf16 elements: exactly the queried size
    EXPECT(st.size() * 2 == P.bytes);
    unsigned short* cache = st.data() + P.cache_off / 2;
    int ran = 0;
    for (int p : edge_values(cap)) {
        const int t = slot_decode(p, cap);                                     // the encoder's limit is its capacity
        if (t == MMT_SLOT_SKIP) continue;
        ++ran;
        for (int layer : {0, N - 1}) for (int kv : {0, 1}) for (int b : {0, B - 1}) for (int head : {0, h - 1}) {
            unsigned short* row = cache + (size_t)layer * P.cache_layer + (size_t)kv * P.cache_kv + (size_t)b * P.cache_seq
                                  + (size_t)head * P.cache_head + (size_t)t * P.dkp;
            row[0] += 1; row[P.dkp - 1] += 1;                                  // what step t writes; the sweeps read rows j < t of the same head
            EXPECT(row + P.dkp <= st.data() + st.size());
            EXPECT((size_t)(row - cache) + P.dkp <= P.cache_elems);
        }
        (void)advanced(t);
    }
    EXPECT(ran == (cap == 1 ? 1 : cap == 2 ? 2 : 3));                          // 0, 1 and cap - 1, as far as they are distinct and < cap
    bool apart = true;                                                         // nothing landed in the weights
    for (size_t i = 0; i < P.cache_off / 2; ++i) apart = apart && st[i] == 0;
    EXPECT(apart);
}

// the gate: copy t & 1 of the carried state is read, the other written, for sequence b, on a buffer of the queried size
static void check_gate(int B, int limit) {
    const int D[3] = {40, 24, 32}, H[3] = {88, 48, 88};
    MfnStepPlan P; const char* why = nullptr;
    EXPECT(mfn_step_plan(P, B, 3, D, H, 1, &why) == MMT_MFN_STEP_OK);
    std::vector<float> st(P.bytes / 4);
    EXPECT(st.size() * 4 == P.bytes);
    float* dyn = st.data() + P.dyn_off / 4;
    for (int p : edge_values(limit)) {
        const int t = slot_decode(p, limit);
        if (t == MMT_SLOT_SKIP) continue;
        for (int b : {0, B - 1}) {
            float* in = dyn + ((size_t)(t & 1) * B + b) * P.seq_floats;
            float* out = dyn + ((size_t)((t & 1) ^ 1) * B + b) * P.seq_floats;
            EXPECT(in != out);
            in[0] += 1; in[P.seq_floats - 1] += 1; out[0] += 1; out[P.seq_floats - 1] += 1;
            EXPECT(in + P.seq_floats <= st.data() + st.size() && out + P.seq_floats <= st.data() + st.size());
        }
        (void)advanced(t);
    }
}

int main() {
    for (int limit : {INT_MIN, -1, 0, 1, 2, 3, 45, 4096, INT_MAX - 1, INT_MAX}) check_decode(limit);
    // capacity at both ends of the domain of the plan (1 and MMT_STEP_MAX_CAPACITY), small and wide heads, one and several sequences
    for (int cap : {1, 2, 4, 130, MMT_STEP_MAX_CAPACITY}) {
        check_encoder(1, cap, 32, 2, 128, 1);
        check_encoder(3, cap, 40, 4, 128, 2);
        check_encoder(4, cap, 64, 2, 128, 3);
    }
    check_encoder(2, MMT_STEP_MAX_CAPACITY, 512, 8, 2048, 2);
    for (int limit : {0, -1, 1, 4, 12, MMT_STEP_MAX_CAPACITY}) { check_gate(1, limit); check_gate(3, limit); }
    printf(fails ? "%d checks FAILED\n" : "slot_pos_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
