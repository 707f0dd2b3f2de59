// Stand-alone host check of the one-window LSTM-baseline step's limits and state layout (csrc/lstm_step_plan.h): no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -o tools/bin/lstm_step_plan_check tools/lstm_step_plan_check.cpp && tools/bin/lstm_step_plan_check
// Walks the limits and their refused neighbours; for accepted shapes checks that the regions of the state are aligned, do not overlap
// and sum to the reported size, and, on a host buffer of exactly that size, walks the job table that mmt_lstm_stream_prepare launches
// (lstm_step_prep_table, through step_prep_walk.h: every weight and vector byte written exactly once, none elsewhere) and forms every
// address a step can form, with the kernel's own expressions: both copies of (h, c) for every (b, layer), and the ring slot written and
// the ring slots read at the positions slot_decode lets through, so that an offset or size mistake is a failed check or an
// AddressSanitizer report.  It also holds the state discipline: the slot a step writes is none of the slots it reads, and a slot it
// reads was written by an earlier step of the recording.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../multimodal_transformer_amd/csrc/lstm_step_plan.h"
#include "../multimodal_transformer_amd/csrc/step_slots.h"
#include "step_prep_walk.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static bool accepted(int B, int in, int E, int H, int NL, int L) {
    return B >= 1 && in >= 1 && in <= 2048 && E >= 1 && E <= 512 && H >= 1 && H <= 512 && NL >= 1 && NL <= 4 && L >= 1 && L <= 16;
}

typedef PrepRegion Region;

static void check_layout(int B, int in, int E, int H, int NL, int L, bool touch) {
    LstmStepPlan P; const char* why = nullptr;
    EXPECT(lstm_step_plan(P, B, in, E, H, NL, L, &why) == MMT_LSTM_STEP_OK);
    EXPECT(P.in == in && P.E == E && P.H == H && P.NL == NL && P.L == L);
    EXPECT(P.KPin >= in && P.KPin % 8 == 0 && P.KPin - in < 8 && P.KPe >= E && P.KPe % 8 == 0 && P.KPe - E < 8 &&
           P.KPh >= H && P.KPh % 8 == 0 && P.KPh - H < 8);
    // the kernel's LDS rows: xs, emb, hid, hp, hc, pre, htop, zs (lstm_step.h)
    EXPECT(P.KPin <= MMT_LSTM_STEP_MAX_IN && P.KPe <= MMT_LSTM_STEP_MAX_E && P.KPh <= MMT_LSTM_STEP_MAX_H &&
           NL <= MMT_LSTM_STEP_MAX_LAYERS && L <= MMT_LSTM_STEP_MAX_TAPS);
    // every region, in bytes; the matrices first, with their rows and padded k
    struct Mat { size_t off; int rows, kp; };
    std::vector<Mat> M;
    M.push_back({P.we, E, P.KPin});
    M.push_back({P.wa0, E, P.KPe});
    M.push_back({P.wa2, L, P.KPe});
    for (int l = 0; l < NL; ++l) { M.push_back({P.wih[l], 4 * H, l == 0 ? P.KPe : P.KPh}); M.push_back({P.whh[l], 4 * H, P.KPh}); }
    M.push_back({P.wd0, E, P.KPh});
    M.push_back({P.wd2, 1, P.KPe});
    std::vector<Region> R;
    for (const Mat& m : M) R.push_back({m.off, (size_t)m.rows * m.kp * 2});
    R.push_back({P.be, (size_t)E * 4});
    R.push_back({P.ba0, (size_t)E * 4});
    R.push_back({P.ba2, (size_t)L * 4});
    for (int l = 0; l < NL; ++l) R.push_back({P.bl[l], (size_t)4 * H * 4});
    R.push_back({P.bd0, (size_t)E * 4});
    R.push_back({P.bd2, 4});
    EXPECT(P.seq_floats == (size_t)2 * NL * H && P.dyn_floats == (size_t)2 * B * P.seq_floats);
    EXPECT(P.ring_seq_floats == (size_t)L * H && P.ring_floats == (size_t)B * P.ring_seq_floats);
    R.push_back({P.dyn_off, P.dyn_floats * 4});
    R.push_back({P.ring_off, P.ring_floats * 4});
    std::sort(R.begin(), R.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
    size_t end = 0, used = 0;
    for (const Region& r : R) {
        EXPECT(r.off % 256 == 0 && r.off >= end && r.len > 0);                 // aligned, disjoint
        EXPECT(r.off - end < 256);                                             // and nothing but alignment between two of them
        end = r.off + r.len;
        used += (r.len + 255) / 256 * 256;
    }
    EXPECT(R.front().off == 0 && used == P.bytes && P.bytes >= end && P.bytes - end < 256);       // they sum to the size
    EXPECT(P.dyn_off % 256 == 0 && P.dyn_off + P.dyn_floats * 4 <= P.ring_off && P.ring_off + P.ring_floats * 4 <= P.bytes);
    EXPECT(R[R.size() - 2].off == P.dyn_off && R.back().off == P.ring_off);    // the dynamic part lies behind everything prepared
    if (!touch) return;
    std::vector<unsigned char> st(P.bytes);                                    // exactly the queried size: counts the writes of a byte
    // what the preparation writes: the table the entry launches, with sources that are never dereferenced
    static const float some = 0.f;
    const float* pp[MMT_LSTM_STEP_NPARAMS(MMT_LSTM_STEP_MAX_LAYERS)];
    for (const float*& q : pp) q = &some;
    StepPrepParams T; size_t most = 0;
    lstm_step_prep_table(P, pp, T, most);
    EXPECT(T.nmat == 5 + 2 * NL && T.nvec == 5 + NL);
    R.pop_back(); R.pop_back();                                                // (h, c) and the ring: never prepared
    fails += step_prep_walk(T, most, R, P.dyn_off, st.data());
    for (size_t i = P.dyn_off; i < P.bytes; ++i) EXPECT(st[i] == 0);
    // every address of the dynamic part a step can form, with the kernel's expressions, at the positions slot_decode lets through
    float* dyn = reinterpret_cast<float*>(st.data() + P.dyn_off);
    float* rings = reinterpret_cast<float*>(st.data() + P.ring_off);
    for (int p : {0, 1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, INT_MAX - 1, INT_MAX, -1, INT_MIN}) {
        const int t = slot_decode(p, 0);
        if (t == MMT_SLOT_SKIP) continue;
        for (int b : {0, B / 2, B - 1}) {
            for (int l = 0; l < NL; ++l) {
                float* in_ = dyn + ((size_t)(t & 1) * B + b) * P.seq_floats + (size_t)l * 2 * H;
                float* out = dyn + ((size_t)((t & 1) ^ 1) * B + b) * P.seq_floats + (size_t)l * 2 * H;
                EXPECT(in_ != out);
                for (int i = 0; i < 2 * H; ++i) { in_[i] = 1.f; out[i] = 2.f; }     // h (H) | c (H)
            }
            float* ring = rings + (size_t)b * P.ring_seq_floats;
            const int taps = t < L - 1 ? t : L - 1, wr = t % L;
            EXPECT(wr >= 0 && wr < L);
            for (int i = 1; i <= taps; ++i) {
                const int rd = (t - i) % L;
                EXPECT(rd >= 0 && rd < L && rd != wr && t - i >= 0);           // an earlier step's slot, never the one written
                for (int j = 0; j < H; ++j) ring[(size_t)rd * H + j] += 1.f;
            }
            for (int j = 0; j < H; ++j) ring[(size_t)wr * H + j] = 3.f;
        }
    }
    // a recording from position 0: every slot read was written by an earlier step of it (0 marks a slot never written)
    std::vector<int> written(L, 0);
    for (int t = 0; t < 3 * L + 2; ++t) {
        const int taps = t < L - 1 ? t : L - 1;
        for (int i = 1; i <= taps; ++i) EXPECT(written[(t - i) % L] == t - i + 1);
        written[t % L] = t + 1;
    }
}

int main() {
    const char* why = nullptr;
    LstmStepPlan P;
    // the limits and their neighbours, one dimension at a time around an accepted shape
    for (int in = -2; in <= 2056; ++in) {
        const int rc = lstm_step_plan(P, 2, in, 16, 8, 1, 3, &why);
        EXPECT((rc == MMT_LSTM_STEP_OK) == accepted(2, in, 16, 8, 1, 3));
        if (rc) EXPECT(why && strstr(why, "lstm stream"));
        else if (in % 97 == 0 || in < 20 || in > 2040) check_layout(2, in, 16, 8, 1, 3, false);
    }
    for (int E = -1; E <= 516; ++E) {
        const int rc = lstm_step_plan(P, 2, 12, E, 8, 1, 3, &why);
        EXPECT((rc == MMT_LSTM_STEP_OK) == accepted(2, 12, E, 8, 1, 3));
        if (!rc) check_layout(2, 12, E, 8, 2, 3, false);
    }
    for (int H = -1; H <= 516; ++H) {
        const int rc = lstm_step_plan(P, 2, 12, 16, H, 1, 3, &why);
        EXPECT((rc == MMT_LSTM_STEP_OK) == accepted(2, 12, 16, H, 1, 3));
        if (!rc) check_layout(2, 12, 16, H, 2, 3, false);
    }
    for (int NL = -1; NL <= 6; ++NL) EXPECT((lstm_step_plan(P, 2, 12, 16, 8, NL, 3, &why) == MMT_LSTM_STEP_OK) == accepted(2, 12, 16, 8, NL, 3));
    for (int L = -1; L <= 18; ++L) EXPECT((lstm_step_plan(P, 2, 12, 16, 8, 1, L, &why) == MMT_LSTM_STEP_OK) == accepted(2, 12, 16, 8, 1, L));
    for (int B : {-1, 0, 1, 3, 1024}) EXPECT((lstm_step_plan(P, B, 12, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_OK) == accepted(B, 12, 16, 8, 1, 3));
    // the error class and the named limit
    EXPECT(lstm_step_plan(P, 0, 12, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(lstm_step_plan(P, 2, 0, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(lstm_step_plan(P, 2, 12, 0, 8, 1, 3, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(lstm_step_plan(P, 2, 12, 16, 0, 1, 3, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(lstm_step_plan(P, 2, 12, 16, 8, 0, 3, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(lstm_step_plan(P, 2, 12, 16, 8, 1, 0, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "non-positive"));
    EXPECT(lstm_step_plan(P, 2, 2049, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "input width > 2048"));
    EXPECT(lstm_step_plan(P, 2, 12, 513, 8, 1, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "embed_dim > 512"));
    EXPECT(lstm_step_plan(P, 2, 12, 16, 513, 1, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "h_dim > 512"));
    EXPECT(lstm_step_plan(P, 2, 12, 16, 8, 5, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "n_layers > 4"));
    EXPECT(lstm_step_plan(P, 2, 12, 16, 8, 1, 17, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "attn_len > 16"));
    // layouts with every element touched: the GPU test's shapes, ragged sizes, the small and far corners
    check_layout(1, 8, 8, 4, 1, 1, true);
    check_layout(3, 12, 12, 20, 1, 3, true);
    check_layout(3, 300, 128, 256, 1, 5, true);
    check_layout(2, 40, 64, 32, 4, 16, true);
    check_layout(2, 1556, 512, 256, 1, 5, true);
    check_layout(1, 2048, 512, 512, 1, 16, true);
    check_layout(33, 16, 8, 8, 2, 3, true);
    check_layout(1, 1, 1, 1, 1, 1, true);
    check_layout(5, 7, 3, 5, 4, 2, true);
    check_layout(3, 2047, 511, 509, 3, 15, true);
    check_layout(64, 2048, 512, 512, 4, 16, true);
    check_layout(32, 300, 128, 256, 1, 5, true);
    printf(fails ? "%d checks FAILED\n" : "lstm_step_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
