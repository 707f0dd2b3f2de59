// Stand-alone host check of the prefill rule (csrc/step_prefill_plan.h): no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/bin/prefill_plan_check tools/prefill_plan_check.cpp && tools/bin/prefill_plan_check
// The prefill kernels (csrc/step_prefill.h) move K and V of a batch forward's workspace into a stream's K/V cache and the last state
// of the decoder's scan into its carried state, every address formed by the functions of the plan header.  This program walks those
// functions exactly as the kernels do, on host buffers of exactly the queried sizes (AddressSanitizer holds the edges), for
//   d_k in {8, 10, 16, 32, 40, 64};  P in {1, 31, 32, 33, capacity};  ragged lengths;  a ring with P <, =, > span, span = 1 and
//   P = 2 span + 3;  a permuted, partial dst;  and (dst, len) pairs outside their ranges, which must be skipped.
// It checks that
//   * every written element lies inside the cache / carried-state region of sequence dst[b], and nothing else of the state changes:
//     no prepared weight, no other sequence, no row >= len[b] of a plain cache;
//   * every cache row that a step at t = len[b] reads (plain: rows < len; ring: the ages of step_ring.h) was written, with the
//     elements of its position, and the pad columns d_k <= e < dkp are zeros;
//   * no two source elements share a destination;
//   * the source index stays inside a head's Tp x DKP block of the workspace.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../multimodal_transformer_amd/csrc/step_prefill_plan.h"
#include "../multimodal_transformer_amd/csrc/step_ring.h"

static int fails = 0;
static const char* g_case = "";
#define EXPECT(c) do { if (!(c)) { if (fails < 20) printf("FAILED %s (line %d; %s)\n", #c, __LINE__, g_case); ++fails; } } while (0)

// a value that names its source: (layer, kv, b, head, pos, e) in 16 bits would not fit, so sources are numbered instead
struct Walk {
    StepPlan S; PrefillGeom G;
    std::vector<uint32_t> src[2];         // K | V of ONE layer's workspace region, exactly B_src * h * Tp * DKP elements; value = 1 + index
    std::vector<uint32_t> state;          // one word per bf16 element of the state, exactly S.bytes / 2; 0 = untouched
    std::vector<uint8_t> written;         // per state element
};

static void encoder_case(int d, int h, int N, int B_src, int P, int B_state, int rows, int ring, const std::vector<int>& dst, const std::vector<int>& len,
                         bool expect_all_valid) {
    static char name[160];
    snprintf(name, sizeof(name), "d=%d h=%d N=%d B_src=%d P=%d B_state=%d rows=%d ring=%d", d, h, N, B_src, P, B_state, rows, ring);
    g_case = name;
    Walk W; const char* why = "";
    EXPECT(step_plan(W.S, B_state, rows, d, h, 4 * ((d + 3) / 4), N, &why) == MMT_STEP_OK);
    prefill_geom(W.G, W.S, B_src, P, B_state, rows, ring, h, N);
    const PrefillGeom& G = W.G;
    EXPECT(G.DKP >= G.dkp && G.DKP % 8 == 0 && G.Tp >= P && G.Tp % 32 == 0 && G.nchunk * 8 == G.dkp);
    const size_t src_elems = (size_t)B_src * h * G.src_head;
    const size_t cache0 = W.S.cache_off / 2;
    W.state.assign(W.S.bytes / 2, 0);
    W.written.assign(W.S.bytes / 2, 0);
    uint32_t* cache = W.state.data() + cache0;
    for (int layer = 0; layer < N; ++layer) {
        for (int kv = 0; kv < 2; ++kv) {
            // this (layer, kv)'s source: every element, pads included, carries a value that is not zero
            W.src[kv].assign(src_elems, 0);
            for (size_t i = 0; i < src_elems; ++i) W.src[kv][i] = (uint32_t)(1 + i % 0x7fffffff);
            for (int b = 0; b < B_src; ++b) {
                const PrefillSeq q = prefill_seq(dst[b], len[b], P, B_state, rows, ring);
                if (q.dst == MMT_PREFILL_SKIP) { EXPECT(!expect_all_valid); continue; }
                EXPECT(q.dst == dst[b] && q.len == len[b] && q.first >= 0 && q.first < q.len);
                EXPECT(ring ? q.len - q.first == (len[b] < rows ? len[b] : rows) : q.first == 0);
                const size_t total = prefill_items(G, q);
                EXPECT(total == (size_t)h * (q.len - q.first) * G.nchunk);
                for (size_t i = 0; i < total; ++i) {
                    const PrefillItem it = prefill_item(G, q, i);
                    EXPECT(it.head >= 0 && it.head < h && it.pos >= q.first && it.pos < q.len && it.c >= 0 && it.c < G.nchunk);
                    const PrefillAt at = prefill_at(G, layer, kv, b, q.dst, it.head, it.pos, it.c);
                    // the source chunk: inside this head's block, 16-byte aligned, and the element fragR_index names
                    const size_t head0 = ((size_t)b * h + it.head) * G.src_head;
                    EXPECT(at.src >= head0 && at.src + 8 <= head0 + G.src_head && at.src % 8 == 0);
                    EXPECT(at.src - head0 == ((size_t)(it.pos >> 5) * (G.DKP >> 3) + it.c) * 256 + (size_t)(it.pos & 31) * 8);
                    // the destination chunk: inside the cache of sequence dst[b], this layer, K | V, head; 16-byte aligned
                    const size_t seq0 = (size_t)layer * G.cache_layer + (size_t)kv * G.cache_kv + (size_t)q.dst * G.cache_seq + (size_t)it.head * G.cache_head;
                    EXPECT(at.dst >= seq0 && at.dst + 8 <= seq0 + G.cache_head && at.dst % 8 == 0 && at.dst + 8 <= W.S.cache_elems);
                    const int row = (int)((at.dst - seq0) / G.dkp);
                    EXPECT(row == (ring ? it.pos % rows : it.pos) && row < rows && (at.dst - seq0) % G.dkp == (size_t)8 * it.c);
                    for (int e = 0; e < 8; ++e) {
                        EXPECT(!W.written[cache0 + at.dst + e]);                  // no two sources share a destination
                        W.written[cache0 + at.dst + e] = 1;
                        cache[at.dst + e] = 8 * it.c + e < G.dk ? W.src[kv][at.src + e] : 0;      // the kernel's select
                    }
                }
            }
            // what a step at t = len[b] reads of this (layer, kv): every row, every element of dkp, holds its position's values
            for (int b = 0; b < B_src; ++b) {
                const PrefillSeq q = prefill_seq(dst[b], len[b], P, B_state, rows, ring);
                if (q.dst == MMT_PREFILL_SKIP) continue;
                const int t = q.len;
                if (!ring && t >= rows) continue;                                  // a full plain stream runs no further step
                const int n = ring ? ring_keys(t, rows) : t, r0 = ring ? ring_first_row(t, n, rows) : 0;
                for (int head = 0; head < h; ++head)
                    for (int i = 0; i < n; ++i) {
                        const int row = ring ? ring_row(r0, i, rows) : i, pos = t - n + i;
                        const size_t o = (size_t)layer * G.cache_layer + (size_t)kv * G.cache_kv + (size_t)q.dst * G.cache_seq
                                         + (size_t)head * G.cache_head + (size_t)row * G.dkp;
                        for (int e = 0; e < G.dkp; ++e) {
                            EXPECT(W.written[cache0 + o + e]);
                            const size_t s = ((size_t)b * h + head) * G.src_head + prefill_fragR_index(pos, e, G.DKP);
                            EXPECT(cache[o + e] == (e < G.dk ? W.src[kv][s] : 0u));
                        }
                    }
            }
        }
    }
    // nothing else changed: the weights, the sequences no dst names, rows >= len of a plain cache
    size_t count = 0, want = 0;
    for (size_t i = 0; i < W.written.size(); ++i) count += W.written[i];
    for (int b = 0; b < B_src; ++b) {
        const PrefillSeq q = prefill_seq(dst[b], len[b], P, B_state, rows, ring);
        if (q.dst != MMT_PREFILL_SKIP) want += (size_t)2 * N * h * (q.len - q.first) * G.dkp;
    }
    EXPECT(count == want);
    for (size_t i = 0; i < cache0; ++i) EXPECT(!W.written[i]);
    std::vector<int> named(B_state, -1);
    for (int b = 0; b < B_src; ++b) if (prefill_seq(dst[b], len[b], P, B_state, rows, ring).dst != MMT_PREFILL_SKIP) named[dst[b]] = len[b];
    for (int layer = 0; layer < N; ++layer) for (int kv = 0; kv < 2; ++kv) for (int s = 0; s < B_state; ++s) for (int head = 0; head < h; ++head)
        for (int row = 0; row < rows; ++row) {
            const size_t o = (size_t)layer * G.cache_layer + (size_t)kv * G.cache_kv + (size_t)s * G.cache_seq + (size_t)head * G.cache_head + (size_t)row * G.dkp;
            const bool may = named[s] >= 0 && (ring ? true : row < named[s]);
            if (!may) for (int e = 0; e < G.dkp; ++e) EXPECT(!W.written[cache0 + o + e]);
        }
}

static void decoder_case(int B_src, int B_state, int P, int d, int hdim, const std::vector<int>& dst, const std::vector<int>& len) {
    static char name[160];
    snprintf(name, sizeof(name), "decoder B_src=%d B_state=%d P=%d d=%d", B_src, B_state, P, d);
    g_case = name;
    DecStepPlan S; const char* why = "";
    EXPECT(decoder_step_plan(S, B_state, d, hdim, 1, &why) == MMT_DEC_STEP_OK);
    std::vector<float> h_all((size_t)P * B_src * d), c_all((size_t)P * B_src * d);
    for (size_t i = 0; i < h_all.size(); ++i) { h_all[i] = (float)(1 + i); c_all[i] = -(float)(1 + i); }
    std::vector<float> state(S.bytes / 4, 0.f);
    std::vector<uint8_t> written(S.bytes / 4, 0);
    float* dyn = state.data() + S.dyn_off / 4;
    for (int b = 0; b < B_src; ++b) {
        const PrefillSeq q = prefill_seq(dst[b], len[b], P, B_state, P, 0);
        if (q.dst == MMT_PREFILL_SKIP) continue;
        for (int i = 0; i < 2 * d; ++i) {
            const int which = i >= d, j = i - which * d;
            const DecPrefillAt at = dec_prefill_at(B_src, B_state, d, S.seq_floats, b, q.dst, q.len, which, j);
            EXPECT(at.src < h_all.size() && at.dst < S.dyn_floats);
            // the copy a step at t = len reads (step_common.h step_state: in = copy t & 1), sequence dst, [h | c]
            EXPECT(at.dst == ((size_t)(q.len & 1) * B_state + q.dst) * S.seq_floats + (size_t)which * d + j);
            EXPECT(!written[S.dyn_off / 4 + at.dst]);
            written[S.dyn_off / 4 + at.dst] = 1;
            dyn[at.dst] = (which ? c_all : h_all)[at.src];
            EXPECT(dyn[at.dst] == (which ? -1.f : 1.f) * (float)(1 + ((size_t)(q.len - 1) * B_src + b) * d + j));
        }
    }
    for (size_t i = 0; i < S.dyn_off / 4; ++i) EXPECT(!written[i]);
}

int main() {
    struct Shape { int d, h; };
    const Shape shapes[] = {{32, 4}, {40, 4}, {128, 8}, {64, 2}, {80, 2}, {256, 4}};      // d_k = 8, 10, 16, 32, 40, 64
    for (const Shape& s : shapes) {
        const int capacity = 45;
        for (int P : {1, 31, 32, 33, capacity}) {
            encoder_case(s.d, s.h, 2, 3, P, 3, capacity, 0, {0, 1, 2}, {P, P, P}, true);                         // the host form: dst[b] = b, len[b] = P
            encoder_case(s.d, s.h, 2, 3, P, 5, capacity, 0, {4, 0, 2}, {P, (P + 1) / 2, 1}, true);               // ragged, a permuted, partial dst
        }
        for (int span : {1, 5, 33}) {
            for (int P : {span > 1 ? span - 1 : 1, span, span + 1, 2 * span + 3, 70})
                encoder_case(s.d, s.h, 2, 3, P, 4, span, 1, {3, 1, 0}, {P, (P + 1) / 2, 1}, true);
        }
    }
    encoder_case(40, 4, 3, 4, 9, 4, 9, 0, {0, 7, -1, 2}, {9, 3, 3, 10}, false);      // dst outside the state, len > P: skipped, nothing written
    encoder_case(40, 4, 1, 2, 9, 2, 9, 0, {0, 1}, {0, -5}, false);                   // no windows: skipped
    {   // P > capacity is a pair prefill_seq refuses in the plain form and serves in a ring
        EXPECT(prefill_seq(0, 10, 10, 1, 9, 0).dst == MMT_PREFILL_SKIP);
        EXPECT(prefill_seq(0, 10, 10, 1, 9, 1).dst == 0 && prefill_seq(0, 10, 10, 1, 9, 1).first == 1);
    }
    decoder_case(3, 5, 7, 40, 16, {4, 0, 2}, {7, 4, 1});
    decoder_case(1, 1, 1, 8, 1, {0}, {1});
    decoder_case(3, 3, 6, 12, 5, {0, 9, 1}, {6, 2, 7});                               // a pair outside its ranges is skipped
    printf(fails ? "%d checks FAILED\n" : "prefill_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
