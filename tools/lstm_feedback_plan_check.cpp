// Stand-alone host check of the limits and state layout of the LSTM-baseline steps with a tail (csrc/lstm_feedback_step_plan.h): no HIP,
// no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -o tools/bin/lstm_feedback_plan_check tools/lstm_feedback_plan_check.cpp && tools/bin/lstm_feedback_plan_check
// Walks the limits and their refused neighbours for both tails; for accepted shapes checks that the front is lstm_step_plan's own plan,
// that the tail's pieces are aligned, lie behind it, do not overlap and sum to the reported size, and, on a host buffer of exactly that
// size, walks the job table that mmt_lstm_feedback_stream_prepare launches (lstm_feedback_prep_table, through step_prep_walk.h: every
// prepared byte written exactly once, no byte of a carried block or ring) and forms every address of the tail's dynamic part that a
// step at positions 0, 1, K - 1, K, K + 1 and a large t forms, with the kernel's own expressions, so that an offset or size mistake is
// a failed check or an AddressSanitizer report.  It holds the state discipline: the two copies of (hd, cd, q) are distinct, the
// history slot a step writes is none of the slots it reads, and a slot it reads was written by the step it names.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../multimodal_transformer_amd/csrc/lstm_feedback_step_plan.h"
#include "../multimodal_transformer_amd/csrc/step_slots.h"
#include "step_prep_walk.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static const int FB = MMT_LSTM_TAIL_FB, AR = MMT_LSTM_TAIL_AR;

static bool accepted(int tail, int K, int B, int in, int E, int H, int NL, int L) {
    const bool front = B >= 1 && in >= 1 && in <= 2048 && E >= 1 && E <= 512 && H >= 1 && H <= 512 && NL >= 1 && NL <= 4 && L >= 1 && L <= 16;
    return front && (tail == FB ? NL == 1 : tail == AR && K >= 1 && K <= 16);
}

static int plan(LstmFeedbackPlan& P, int tail, int K, int B, int in, int E, int H, int NL, int L, const char** why) {
    return lstm_feedback_plan(P, tail, K, B, in, E, H, NL, L, why);
}

typedef PrepRegion Region;

static void check_layout(int tail, int K, int B, int in, int E, int H, int NL, int L, bool touch) {
    LstmFeedbackPlan P; const char* why = nullptr;
    EXPECT(plan(P, tail, K, B, in, E, H, NL, L, &why) == MMT_LSTM_STEP_OK);
    const LstmStepPlan& S = P.front;
    LstmStepPlan Q;
    EXPECT(lstm_step_plan(Q, B, in, E, H, NL, L, &why) == MMT_LSTM_STEP_OK && memcmp(&Q.bytes, &S.bytes, sizeof(size_t)) == 0);
    EXPECT(Q.we == S.we && Q.wd0 == S.wd0 && Q.wd2 == S.wd2 && Q.bd0 == S.bd0 && Q.bd2 == S.bd2 && Q.dyn_off == S.dyn_off && Q.ring_off == S.ring_off &&
           Q.KPin == S.KPin && Q.KPe == S.KPe && Q.KPh == S.KPh && Q.seq_floats == S.seq_floats && Q.ring_seq_floats == S.ring_seq_floats);
    const bool fb = tail == FB;
    EXPECT(P.tail == tail && P.K == (fb ? 0 : K) && P.K <= MMT_LSTM_FEEDBACK_MAX_AR);
    // the tail's pieces, in bytes: prepared ones first, then the carried block or the ring
    std::vector<Region> R;
    if (fb) {
        R.push_back({P.wc, (size_t)4 * H * S.KPh * 2});
        R.push_back({P.whd, (size_t)4 * H * S.KPh * 2});
        R.push_back({P.wp, (size_t)4 * H * 4});
        R.push_back({P.bdec, (size_t)4 * H * 4});
        R.push_back({P.w2, (size_t)E * 4});
        for (size_t off : {P.enc_h0, P.enc_c0, P.dec_h0, P.dec_c0}) R.push_back({off, (size_t)H * 4});
        EXPECT(P.fb_seq_floats >= (size_t)2 * H + 1 && P.fb_seq_floats % 4 == 0 && P.fb_seq_floats - (2 * H + 1) < 4);
        EXPECT(P.fb_floats == (size_t)2 * B * P.fb_seq_floats && P.hist_floats == 0 && P.hist_seq_floats == 0);
        R.push_back({P.fb_off, P.fb_floats * 4});
    } else {
        R.push_back({P.wa, (size_t)K * S.KPh * 2});
        R.push_back({P.ba, (size_t)K * 4});
        EXPECT(P.hist_seq_floats == (size_t)K + 1 && P.hist_floats == (size_t)B * (K + 1) && P.fb_floats == 0 && P.fb_seq_floats == 0);
        R.push_back({P.hist_off, P.hist_floats * 4});
    }
    const size_t dyn = R.back().off;                                            // the tail's dynamic part lies behind everything prepared
    size_t end = S.bytes, used = S.bytes;
    EXPECT(S.bytes % 256 == 0);
    for (const Region& r : R) {
        EXPECT(r.off % 256 == 0 && r.off >= end && r.len > 0);                 // aligned, disjoint, behind the front
        EXPECT(r.off - end < 256);                                             // and nothing but alignment between two of them
        end = r.off + r.len;
        used += (r.len + 255) / 256 * 256;
    }
    EXPECT(R.front().off == S.bytes && used == P.bytes && P.bytes >= end && P.bytes - end < 256);
    if (!touch) return;
    std::vector<unsigned char> st(P.bytes);                                    // exactly the queried size: counts the writes of a byte
    // what the preparation writes: the table the entry launches, with sources that are never dereferenced
    static const float some = 0.f;
    const float* pp[MMT_LSTM_STEP_NPARAMS(MMT_LSTM_STEP_MAX_LAYERS) + 9];
    for (const float*& q : pp) q = &some;
    StepPrepParams T; size_t most = 0;
    lstm_feedback_prep_table(P, pp, T, most);
    EXPECT(T.nmat == 5 + 2 * NL + (fb ? 2 : 1) && T.nvec == 5 + NL + (fb ? 7 : 1));
    EXPECT(MMT_LSTM_FEEDBACK_NPARAMS(tail, NL) == 10 + 4 * NL + (fb ? 9 : 2));
    if (fb) {                                                                  // W_c: the columns behind the first of a (4H, 1 + H) matrix
        const StepPrepMat& J = T.mat[T.nmat - 2];
        EXPECT(J.dst == P.wc && J.col0 == 1 && J.ld == 1 + H && J.rows == 4 * H && J.K == H && J.nout == 4 * H);
    }
    std::vector<Region> prepared;                                              // the front's prepared regions, then the tail's
    {
        struct Mat { size_t off; int rows, kp; };
        std::vector<Mat> M;
        M.push_back({S.we, E, S.KPin}); M.push_back({S.wa0, E, S.KPe}); M.push_back({S.wa2, L, S.KPe});
        for (int l = 0; l < NL; ++l) { M.push_back({S.wih[l], 4 * H, l == 0 ? S.KPe : S.KPh}); M.push_back({S.whh[l], 4 * H, S.KPh}); }
        M.push_back({S.wd0, E, S.KPh}); M.push_back({S.wd2, 1, S.KPe});
        for (const Mat& m : M) prepared.push_back({m.off, (size_t)m.rows * m.kp * 2});
        prepared.push_back({S.be, (size_t)E * 4}); prepared.push_back({S.ba0, (size_t)E * 4}); prepared.push_back({S.ba2, (size_t)L * 4});
        for (int l = 0; l < NL; ++l) prepared.push_back({S.bl[l], (size_t)4 * H * 4});
        prepared.push_back({S.bd0, (size_t)E * 4}); prepared.push_back({S.bd2, 4});
    }
    for (size_t i = 0; i + 1 < R.size(); ++i) prepared.push_back(R[i]);
    // step_prep_walk holds every write below its `dyn_off`: the front's carried state lies between prepared pieces here, so the walk
    // runs with the end of the tail's prepared part and the front's dynamic bytes are checked for zero writes below
    fails += step_prep_walk(T, most, prepared, dyn, st.data());
    for (size_t i = S.dyn_off; i < S.bytes; ++i) EXPECT(st[i] == 0);           // (h, c) and the ring of the front: never prepared
    for (size_t i = dyn; i < P.bytes; ++i) EXPECT(st[i] == 0);                 // the tail's carried block or ring: never prepared
    // every address of the tail's dynamic part a step can form, with the kernel's expressions
    const int Kp = fb ? 1 : K;
    for (int p : {0, 1, Kp - 1, Kp, Kp + 1, 2 * Kp + 3, INT_MAX - 1, INT_MAX, -1, INT_MIN}) {
        const int t = slot_decode(p, 0);
        if (t == MMT_SLOT_SKIP) continue;
        for (int b : {0, B / 2, B - 1}) {
            if (fb) {
                float* blk = reinterpret_cast<float*>(st.data() + P.fb_off);
                float* in_ = blk + ((size_t)(t & 1) * B + b) * P.fb_seq_floats;
                float* out = blk + ((size_t)((t & 1) ^ 1) * B + b) * P.fb_seq_floats;
                EXPECT(in_ != out);
                if (t > 0) for (int i = 0; i <= 2 * H; ++i) in_[i] += 1.f;      // hd (H) | cd (H) | q; position 0 reads none of it
                for (int i = 0; i <= 2 * H; ++i) out[i] = 2.f;
                const float* rows[] = {reinterpret_cast<float*>(st.data() + P.enc_h0), reinterpret_cast<float*>(st.data() + P.enc_c0),
                                       reinterpret_cast<float*>(st.data() + P.dec_h0), reinterpret_cast<float*>(st.data() + P.dec_c0)};
                float sum = 0.f;
                for (const float* r : rows) for (int i = 0; i < H; ++i) sum += r[i];
                EXPECT(sum == sum);
            } else {
                float* hist = reinterpret_cast<float*>(st.data() + P.hist_off) + (size_t)b * P.hist_seq_floats;
                const int wr = t % (K + 1);
                EXPECT(wr >= 0 && wr <= K);
                for (int k = 0; k < K; ++k) {
                    const int s = t - K + k;
                    if (s < 0) continue;                                       // p_init stands in
                    const int rd = s % (K + 1);
                    EXPECT(rd >= 0 && rd <= K && rd != wr);                    // an earlier step's slot, never the one written
                    hist[rd] += 1.f;
                }
                hist[wr] = 3.f;
            }
        }
    }
    if (!fb) {                                                                 // a recording from position 0: every slot read holds the step it names
        std::vector<int> written(K + 1, 0);
        for (int t = 0; t < 3 * (K + 1) + 2; ++t) {
            for (int k = 0; k < K; ++k) if (t - K + k >= 0) EXPECT(written[(t - K + k) % (K + 1)] == t - K + k + 1);
            written[t % (K + 1)] = t + 1;
        }
    }
}

int main() {
    const char* why = nullptr;
    LstmFeedbackPlan P;
    // the limits and their neighbours, one dimension at a time around an accepted shape, for both tails
    for (int tail : {FB, AR}) {
        const int K = tail == AR ? 3 : 0, NL = 1;
        for (int in = -2; in <= 2056; ++in) {
            const int rc = plan(P, tail, K, 2, in, 16, 8, NL, 3, &why);
            EXPECT((rc == MMT_LSTM_STEP_OK) == accepted(tail, K, 2, in, 16, 8, NL, 3));
            if (rc) EXPECT(why && strstr(why, "lstm"));
            else if (in % 97 == 0 || in < 20 || in > 2040) check_layout(tail, K, 2, in, 16, 8, NL, 3, false);
        }
        for (int E = -1; E <= 516; ++E) {
            const int rc = plan(P, tail, K, 2, 12, E, 8, NL, 3, &why);
            EXPECT((rc == MMT_LSTM_STEP_OK) == accepted(tail, K, 2, 12, E, 8, NL, 3));
            if (!rc) check_layout(tail, K, 2, 12, E, 8, NL, 3, false);
        }
        for (int H = -1; H <= 516; ++H) {
            const int rc = plan(P, tail, K, 2, 12, 16, H, NL, 3, &why);
            EXPECT((rc == MMT_LSTM_STEP_OK) == accepted(tail, K, 2, 12, 16, H, NL, 3));
            if (!rc) check_layout(tail, K, 2, 12, 16, H, NL, 3, false);
        }
        for (int n = -1; n <= 6; ++n) EXPECT((plan(P, tail, K, 2, 12, 16, 8, n, 3, &why) == MMT_LSTM_STEP_OK) == accepted(tail, K, 2, 12, 16, 8, n, 3));
        for (int L = -1; L <= 18; ++L) EXPECT((plan(P, tail, K, 2, 12, 16, 8, NL, L, &why) == MMT_LSTM_STEP_OK) == accepted(tail, K, 2, 12, 16, 8, NL, L));
        for (int B : {-1, 0, 1, 3, 1024}) EXPECT((plan(P, tail, K, B, 12, 16, 8, NL, 3, &why) == MMT_LSTM_STEP_OK) == accepted(tail, K, B, 12, 16, 8, NL, 3));
    }
    for (int K = -2; K <= 18; ++K) {
        EXPECT((plan(P, AR, K, 2, 12, 16, 8, 2, 3, &why) == MMT_LSTM_STEP_OK) == accepted(AR, K, 2, 12, 16, 8, 2, 3));
        EXPECT(plan(P, FB, K, 2, 12, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_OK);          // ar_order is not looked at
    }
    for (int tail : {-1, 0, 3}) EXPECT(plan(P, tail, 1, 2, 12, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "tail"));
    // the error class and the named limit
    EXPECT(plan(P, AR, 0, 2, 12, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "ar_order < 1"));
    EXPECT(plan(P, AR, 17, 2, 12, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "ar_order > 16"));
    EXPECT(plan(P, FB, 0, 2, 12, 16, 8, 2, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "n_layers == 1"));
    EXPECT(plan(P, AR, 1, 2, 12, 16, 8, 5, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "n_layers > 4"));
    EXPECT(plan(P, FB, 0, 2, 2049, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "input width > 2048"));
    EXPECT(plan(P, FB, 0, 2, 12, 513, 8, 1, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "embed_dim > 512"));
    EXPECT(plan(P, AR, 1, 2, 12, 16, 513, 1, 3, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "h_dim > 512"));
    EXPECT(plan(P, AR, 1, 2, 12, 16, 8, 1, 17, &why) == MMT_LSTM_STEP_EUNSUPPORTED && strstr(why, "attn_len > 16"));
    EXPECT(plan(P, FB, 0, 0, 12, 16, 8, 1, 3, &why) == MMT_LSTM_STEP_EINVAL && strstr(why, "non-positive"));
    // layouts with every element touched: the GPU test's shapes, ragged sizes, the small and far corners
    check_layout(FB, 0, 1, 8, 8, 4, 1, 1, true);
    check_layout(FB, 0, 3, 12, 12, 20, 1, 3, true);
    check_layout(FB, 0, 3, 300, 128, 128, 1, 3, true);
    check_layout(FB, 0, 2, 64, 128, 512, 1, 7, true);
    check_layout(FB, 0, 33, 16, 8, 8, 1, 3, true);
    check_layout(FB, 0, 1, 1, 1, 1, 1, 1, true);
    check_layout(FB, 0, 5, 7, 3, 5, 1, 2, true);
    check_layout(FB, 0, 3, 2047, 511, 509, 1, 15, true);
    check_layout(FB, 0, 32, 2048, 512, 512, 1, 16, true);
    check_layout(AR, 1, 1, 8, 8, 4, 1, 1, true);
    check_layout(AR, 3, 3, 12, 12, 20, 1, 3, true);
    check_layout(AR, 16, 2, 40, 64, 32, 4, 16, true);
    check_layout(AR, 1, 3, 300, 128, 256, 1, 7, true);
    check_layout(AR, 1, 2, 64, 128, 512, 1, 7, true);
    check_layout(AR, 2, 33, 16, 8, 8, 2, 3, true);
    check_layout(AR, 1, 1, 1, 1, 1, 1, 1, true);
    check_layout(AR, 7, 5, 7, 3, 5, 4, 2, true);
    check_layout(AR, 15, 3, 2047, 511, 509, 3, 15, true);
    check_layout(AR, 16, 32, 2048, 512, 512, 4, 16, true);
    printf(fails ? "%d checks FAILED\n" : "lstm_feedback_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
