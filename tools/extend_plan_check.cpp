// Stand-alone host check of the extend rule (csrc/encoder_extend_plan.h): no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/bin/extend_plan_check tools/extend_plan_check.cpp && tools/bin/extend_plan_check
// encoder_extend_kernel (csrc/encoder_extend.h) moves a stream forward by a tile of up to 16 windows per launch on the K/V cache of
// encoder_step_plan.h, every decision and every cache row formed by the functions of the plan header and of step_ring.h.  This program
// walks those functions exactly as the kernel does, launch by launch and layer by layer (reads, the barrier, writes), on a host array
// of exactly the state's size (AddressSanitizer holds the edges), one word per bf16 element that names the position it holds, for
//   plain and ring forms;  span above, equal to and below the tile (1, 5, 16, 17, 33);  calls of 1 .. 70 windows from t = 0 and from
//   inside a recording, so every tile boundary and partial tile occurs;  ragged lengths;  idle and full slots, slots that would pass
//   the capacity;  (dst, len) pairs outside their ranges;  steps between the calls.
// It checks that
//   * every element read or written lies inside the cache rows of the sequence's own (layer, K | V, dst, head);
//   * no row is written twice in a launch, and a skipped pair writes nothing;
//   * every key a row reads from the cache holds, at the time of the read (before any write of the launch), the position the rule says,
//     and the keys of a row, cached and the tile's own, are exactly the positions of its band (plain: 0 .. p);
//   * behind the call the cache holds what a step at t + len reads;
//   * the LDS carve fits 160 KB for the shapes the project streams, and is refused with the limit named where it does not.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../multimodal_transformer_amd/csrc/encoder_extend_plan.h"

static int fails = 0;
static const char* g_case = "";
#define EXPECT(c) do { if (!(c)) { if (fails < 20) printf("FAILED %s (line %d; %s)\n", #c, __LINE__, g_case); ++fails; } } while (0)

struct Stream {
    StepPlan S; int B, rows, ring, h, N;
    std::vector<int32_t> state;                 // one word per bf16 element of the state: 0 untouched, else 1 + the position it holds
    std::vector<int> pos;                       // the positions, as the device holds them
    std::vector<uint8_t> stamp;                 // per element: written in the current launch
    size_t cache0;
};

static void open(Stream& W, int B, int rows, int ring, int d, int h, int N) {
    const char* why = "";
    W.B = B; W.rows = rows; W.ring = ring; W.h = h; W.N = N;
    EXPECT(step_plan(W.S, B, rows, d, h, 128, N, &why) == MMT_STEP_OK);
    W.state.assign(W.S.bytes / 2, 0);
    W.stamp.assign(W.S.bytes / 2, 0);
    W.pos.assign(B, MMT_SLOT_IDLE);
    W.cache0 = W.S.cache_off / 2;
}

// the element offset of (layer, kv, b, head, row), checked against the head's block; -1 on a violation
static size_t row_at(Stream& W, int layer, int kv, int b, int head, int row) {
    EXPECT(row >= 0 && row < W.rows && b >= 0 && b < W.B);
    const size_t o = (size_t)layer * W.S.cache_layer + (size_t)kv * W.S.cache_kv + (size_t)b * W.S.cache_seq + (size_t)head * W.S.cache_head
                     + (size_t)row * W.S.dkp;
    const size_t seq0 = (size_t)layer * W.S.cache_layer + (size_t)kv * W.S.cache_kv + (size_t)b * W.S.cache_seq + (size_t)head * W.S.cache_head;
    EXPECT(o >= seq0 && o + W.S.dkp <= seq0 + W.S.cache_head && o + W.S.dkp <= W.S.cache_elems && o % 8 == 0);
    return W.cache0 + o;
}

// one launch for one workgroup, as encoder_extend_body runs it.  Returns the rows it ran
static int launch_one(Stream& W, int dst, int len, int first, int p, int C, bool last, bool advance, bool slots) {
    const ExtendRun run = extend_decode(dst, len, first, p, C, W.B, W.rows, W.ring);
    if (run.dst == MMT_EXTEND_SKIP) return 0;
    EXPECT(run.dst == dst && run.c >= 0 && run.c <= MMT_EXTEND_ROWS && run.t == p + first && run.next == p + len);
    EXPECT(W.ring ? run.next < INT_MAX : run.next <= W.rows);
    EXPECT(run.c == 0 || run.t + run.c <= run.next);
    const int t = run.t, c = run.c, span = W.rows;
    if (c > 0) {
        const int n = W.ring ? ring_keys(t, span) : t;
        const int r0 = W.ring ? ring_first_row(t, n, span) : 0;
        for (int layer = 0; layer < W.N; ++layer) for (int kv = 0; kv < 2; ++kv) for (int head = 0; head < W.h; ++head) {
            // reads: every row of the tile, its cached keys by select and the tile's own keys
            for (int i = 0; i < c; ++i) {
                const int pi = t + i, lo = W.ring && pi - span + 1 > 0 ? pi - span + 1 : 0;
                int keys = 0;
                for (int j = 0; j < n; ++j) {
                    const size_t o = row_at(W, layer, kv, dst, head, W.ring ? ring_row(r0, j, span) : j);      // loaded whether or not it counts
                    if (!extend_cached_ok(i, j, n, span, W.ring)) { EXPECT(t - n + j < lo); continue; }
                    EXPECT(t - n + j >= lo);
                    for (int e = 0; e < W.S.dkp; ++e) EXPECT(W.state[o + e] == 1 + (t - n + j) && !W.stamp[o + e]);
                    ++keys;
                }
                for (int u = 0; u < MMT_EXTEND_ROWS; ++u) {
                    if (!extend_tile_ok(i, u, span, W.ring)) { EXPECT(u > i || t + u < lo); continue; }
                    EXPECT(u < c && t + u >= lo && t + u <= pi);
                    ++keys;
                }
                EXPECT(keys == pi - lo + 1);                                       // exactly the band
            }
            // the barrier; writes
            const int w0 = extend_first_written(c, span, W.ring);
            EXPECT(w0 >= 0 && w0 < c && c - w0 == (W.ring && c > span ? span : c));
            for (int i = w0; i < c; ++i) {
                const size_t o = row_at(W, layer, kv, dst, head, prefill_row(t + i, span, W.ring));
                for (int e = 0; e < W.S.dkp; ++e) {
                    EXPECT(!W.stamp[o + e]);                                       // no row twice in a launch
                    W.stamp[o + e] = 1;
                    W.state[o + e] = 1 + t + i;
                }
            }
        }
    }
    if (slots && last && advance) W.pos[dst] = run.next;
    return c;
}

// a call: ceil(C / 16) launches over the table; host form: dst = b, len = C, p = t.  Returns the rows run per table row
static std::vector<int> call(Stream& W, const std::vector<int>& dst, const std::vector<int>& len, int C, bool slots, int t_host, bool advance) {
    std::vector<int> ran(dst.size(), 0);
    const std::vector<int32_t> before = W.state;
    const std::vector<int> pos_before = W.pos;
    for (int first = 0; first < C; first += MMT_EXTEND_ROWS) {
        memset(W.stamp.data(), 0, W.stamp.size());
        const bool last = first + MMT_EXTEND_ROWS >= C;
        for (size_t b = 0; b < dst.size(); ++b) {
            const int p = slots ? (dst[b] >= 0 && dst[b] < W.B ? W.pos[dst[b]] : MMT_SLOT_IDLE) : t_host;
            ran[b] += launch_one(W, dst[b], len[b], first, p, C, last, advance, slots);
        }
    }
    // all or nothing, and nothing outside the named sequences
    std::vector<int> named(W.B, 0);
    for (size_t b = 0; b < dst.size(); ++b) {
        EXPECT(ran[b] == 0 || ran[b] == len[b]);
        if (ran[b]) named[dst[b]] = 1;
    }
    for (int s = 0; s < W.B; ++s) {
        if (named[s]) continue;
        EXPECT(W.pos[s] == pos_before[s]);
        for (int layer = 0; layer < W.N; ++layer) for (int kv = 0; kv < 2; ++kv) {
            const size_t o = W.cache0 + (size_t)layer * W.S.cache_layer + (size_t)kv * W.S.cache_kv + (size_t)s * W.S.cache_seq;
            EXPECT(memcmp(&W.state[o], &before[o], W.S.cache_seq * sizeof(int32_t)) == 0);
        }
    }
    EXPECT(memcmp(W.state.data(), before.data(), W.cache0 * sizeof(int32_t)) == 0);      // the prepared weights
    return ran;
}

// what a step at t reads of sequence b holds its positions; then the step's own write
static void step(Stream& W, int b, int t) {
    const int span = W.rows, n = W.ring ? ring_keys(t, span) : t, r0 = W.ring ? ring_first_row(t, n, span) : 0;
    for (int layer = 0; layer < W.N; ++layer) for (int kv = 0; kv < 2; ++kv) for (int head = 0; head < W.h; ++head) {
        for (int j = 0; j < n; ++j) {
            const size_t o = row_at(W, layer, kv, b, head, W.ring ? ring_row(r0, j, span) : j);
            for (int e = 0; e < W.S.dkp; ++e) EXPECT(W.state[o + e] == 1 + t - n + j);
        }
        const size_t o = row_at(W, layer, kv, b, head, W.ring ? ring_row(r0, n, span) : t);
        for (int e = 0; e < W.S.dkp; ++e) W.state[o + e] = 1 + t;
    }
}

static void host_recording(int d, int h, int rows, int ring, const std::vector<int>& groups) {
    static char name[160];
    snprintf(name, sizeof(name), "host d=%d h=%d rows=%d ring=%d groups=%zu", d, h, rows, ring, groups.size());
    g_case = name;
    Stream W; open(W, 2, rows, ring, d, h, 2);
    int t = 0;
    for (int g : groups) {
        if (g == 0) { step(W, 0, t); step(W, 1, t); ++t; continue; }             // a stepped window between the calls
        const std::vector<int> ran = call(W, {0, 1}, {g, g}, g, false, t, false);
        EXPECT(ran[0] == g && ran[1] == g);
        t += g;
    }
    if (ring || t < rows) { step(W, 0, t); step(W, 1, t); }                      // the cache behind the recording is what a step reads
}

int main() {
    struct Shape { int d, h; };
    const Shape shapes[] = {{32, 4}, {40, 4}, {128, 8}, {64, 2}, {256, 4}};       // d_k = 8, 10, 16, 32, 64
    for (const Shape& s : shapes) {
        host_recording(s.d, s.h, 1, 0, {1});
        host_recording(s.d, s.h, 45, 0, {1, 16, 17, 11});
        host_recording(s.d, s.h, 130, 0, {5, 64, 61});
        host_recording(s.d, s.h, 70, 0, {0, 0, 0, 20, 0, 0, 7, 15, 16, 1});
        for (int span : {1, 5, 16, 17, 33}) {
            host_recording(s.d, s.h, span, 1, {7, 16, 30, 17});
            host_recording(s.d, s.h, span, 1, {0, 0, 0, 20, 0, 0, 7, 33, 1, 70});
            host_recording(s.d, s.h, span, 1, {16, 16, 32, 48});
        }
    }
    for (int ring = 0; ring < 2; ++ring) {
        // slots, B = 4: seated at 17, idle, seated at 0, full (ring: standing at INT_MAX - 2, which len = 2 would take to INT_MAX)
        g_case = ring ? "slots ring" : "slots plain";
        const int rows = ring ? 5 : 40;
        Stream W; open(W, 4, rows, ring, 40, 4, 2);
        call(W, {0}, {17}, 17, true, 0, true);                                      // idle: nothing
        EXPECT(W.pos[0] == MMT_SLOT_IDLE);
        W.pos[0] = 0; W.pos[2] = 0;
        EXPECT(call(W, {0}, {17}, 17, true, 0, true)[0] == 17 && W.pos[0] == 17);
        W.pos[3] = ring ? INT_MAX - 2 : rows;
        const std::vector<int32_t> before = W.state;
        std::vector<int> ran = call(W, {2, 0, 1, 3}, {3, 17, 5, 2}, 17, true, 0, true);
        EXPECT(ran[0] == 3 && ran[1] == 17 && ran[2] == 0 && ran[3] == 0);
        EXPECT(W.pos[0] == 34 && W.pos[1] == MMT_SLOT_IDLE && W.pos[2] == 3 && W.pos[3] == (ring ? INT_MAX - 2 : rows));
        step(W, 0, 34); step(W, 2, 3);
        // advance off: the positions stay, in every launch
        ran = call(W, {2}, {20}, 20, true, 0, false);
        EXPECT(ran[0] == 20 && W.pos[2] == 3);
        if (!ring) {                                                                // position + len passes the capacity: skipped whole
            ran = call(W, {0, 2}, {7, 7}, 40, true, 0, true);
            EXPECT(ran[0] == 0 && ran[1] == 7 && W.pos[0] == 34 && W.pos[2] == 10);
            ran = call(W, {0}, {6}, 6, true, 0, true);
            EXPECT(ran[0] == 6 && W.pos[0] == 40);                                   // exactly full is served
        }
        // pairs outside their ranges: nothing is written
        ran = call(W, {4, -1, 1, 2}, {1, 1, 0, 9}, 8, true, 0, true);
        EXPECT(ran[0] == 0 && ran[1] == 0 && ran[2] == 0 && ran[3] == 0);
    }
    {   // the decision alone: overflow edges
        EXPECT(extend_decode(0, 1, 0, INT_MAX - 1, 1, 1, 5, 1).dst == MMT_EXTEND_SKIP);       // p + len would be INT_MAX
        EXPECT(extend_decode(0, 1, 0, INT_MAX - 2, 1, 1, 5, 1).next == INT_MAX - 1);
        EXPECT(extend_decode(0, 1, 0, INT_MAX, 1, 1, 5, 1).dst == MMT_EXTEND_SKIP);
        EXPECT(extend_decode(0, 4096, 4080, 0, 4096, 1, 4096, 0).c == 16);
        EXPECT(extend_decode(0, 4096, 4080, 1, 4096, 1, 4096, 0).dst == MMT_EXTEND_SKIP);
        EXPECT(extend_decode(0, 3, 16, 0, 20, 1, 40, 0).c == 0 && extend_decode(0, 3, 16, 0, 20, 1, 40, 0).dst == 0);
        EXPECT(extend_decode(0, 3, 32, 0, 20, 1, 40, 0).dst == MMT_EXTEND_SKIP);               // first behind C
    }
    {   // the LDS carve: the streamed shapes at d_ff = 128 fit; the widest shape with d_ff = 2048 is refused with the limit named
        g_case = "lds";
        const int served[][3] = {{32, 2, 128}, {40, 4, 128}, {128, 8, 128}, {64, 2, 128}, {256, 4, 128}, {512, 8, 128}, {256, 8, 128}, {512, 8, 1024}};
        for (const auto& s : served) {
            StepPlan S; ExtendLds L; const char* why = "";
            EXPECT(step_plan(S, 1, 16, s[0], s[1], s[2], 1, &why) == MMT_STEP_OK);
            EXPECT(extend_plan(L, S, s[0], s[2], &why) == MMT_STEP_OK && L.bytes <= MMT_EXTEND_MAX_LDS);
            EXPECT(L.xs % 16 == 0 && L.nb % 16 == 0 && L.hb % 16 == 0 && L.q % 16 == 0 && L.k % 16 == 0 && L.v % 16 == 0);
            EXPECT(L.nb_ld % 8 == 0 && L.hb_ld % 8 == 0 && L.xs_ld % 4 == 0 && L.nb_ld >= (s[0] + 31) / 32 * 32 && L.hb_ld >= (s[2] + 31) / 32 * 32);
            EXPECT(L.v + (size_t)MMT_EXTEND_ROWS * S.HDKP * 2 <= L.bytes);
        }
        StepPlan S; ExtendLds L; const char* why = "";
        EXPECT(step_plan(S, 1, 16, 512, 8, 2048, 1, &why) == MMT_STEP_OK);
        EXPECT(extend_plan(L, S, 512, 2048, &why) == MMT_STEP_EUNSUPPORTED && strstr(why, "160 KB") != nullptr);
    }
    printf(fails ? "%d checks FAILED\n" : "extend_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
