// Stand-alone host check of the feedback LSTM scan's limits and workspace layout (csrc/scan_fb_plan.h): no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -o tools/bin/fb_plan_check tools/fb_plan_check.cpp && tools/bin/fb_plan_check
// Walks every accepted (H, E, B) and the refused neighbours; carves a host buffer of the queried size and touches every fragment element
// the preparation kernel writes and the scan kernels read, so that an offset or size mistake is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../multimodal_transformer_amd/csrc/scan_fb_plan.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

int main() {
    const char* why = nullptr;
    FbPlan P;
    for (int H = -4; H <= 136; ++H)
        for (int E = -4; E <= 136; ++E) {
            const bool ok = fb_plan(P, 0, 0, H, E, true, &why);
            EXPECT(ok == (H >= 4 && H <= 128 && H % 4 == 0 && E >= 4 && E <= 128 && E % 4 == 0));
            if (!ok) { EXPECT(why && strstr(why, "feedback LSTM scan")); continue; }
            EXPECT(P.HP16 >= H && P.HP16 % 16 == 0 && P.HP16 <= P.HPAD && (P.HPAD == 64 || P.HPAD == 128));
            EXPECT(P.NW == P.HP16 / 16 && P.NW >= 1 && P.NW <= 8 && P.block == 64 * P.NW && P.block <= (P.HPAD == 64 ? 256 : 512));
            EXPECT((P.ES == 1 || P.ES == 2 || P.ES == 4 || P.ES == 8) && P.ER == 16 * P.ES * P.NW && P.ER >= E);
            EXPECT(P.HPAD == 64 || P.ES <= 2);                          // the instances api.hip builds
            EXPECT(P.EK >= E && P.EK % 32 == 0 && P.KE == P.EK / 32 && P.KE >= 1 && P.KE <= 4);
            EXPECT(2 * P.block >= E);                                   // the backward turns two MLP rows per thread into du
            EXPECT(P.wb_off >= P.wf_off + 2 * P.wf_elems && P.w1f_off >= P.wb_off + 2 * P.wb_elems && P.w1b_off >= P.w1f_off + 2 * P.w1f_elems);
            EXPECT(P.bytes >= P.w1b_off + 2 * P.w1b_elems && P.wb_off % 256 == 0 && P.w1f_off % 256 == 0 && P.w1b_off % 256 == 0);
            std::vector<unsigned char> ws(P.bytes);
            unsigned short* wf = reinterpret_cast<unsigned short*>(ws.data() + P.wf_off);
            unsigned short* wb = reinterpret_cast<unsigned short*>(ws.data() + P.wb_off);
            unsigned short* w1f = reinterpret_cast<unsigned short*>(ws.data() + P.w1f_off);
            unsigned short* w1b = reinterpret_cast<unsigned short*>(ws.data() + P.w1b_off);
            for (size_t i = 0; i < P.wf_elems; ++i) wf[i] = 1;          // what the preparation kernel writes
            for (size_t i = 0; i < P.wb_elems; ++i) wb[i] = 1;
            for (size_t i = 0; i < P.w1f_elems; ++i) w1f[i] = 1;
            for (size_t i = 0; i < P.w1b_elems; ++i) w1b[i] = 1;
            // what the scans read: 8 elements at row * ld + 8 lq + 32 ks, for every wave, lane and k-block
            unsigned long sum = 0;
            for (int jt = 0; jt < P.NW; ++jt)
                for (int lane = 0; lane < 64; ++lane) {
                    const int l15 = lane & 15, lq = lane >> 4, row = jt * 16 + l15;
                    for (int j = 0; j < 8; ++j) {
                        for (int q = 0; q < 4; ++q)
                            for (int ks = 0; ks < P.HPAD / 32; ++ks) sum += wf[((size_t)q * P.HP16 + row) * P.HPAD + 8 * lq + 32 * ks + j];
                        for (int ks = 0; ks < 4 * P.HPAD / 32; ++ks) sum += wb[(size_t)row * 4 * P.HPAD + 8 * lq + 32 * ks + j];
                        for (int s = 0; s < P.ES; ++s)
                            for (int ks = 0; ks < P.HPAD / 32; ++ks) sum += w1f[(size_t)((s * P.NW + jt) * 16 + l15) * P.HPAD + 8 * lq + 32 * ks + j];
                        for (int ks = 0; ks < P.KE; ++ks) sum += w1b[(size_t)row * P.EK + 8 * lq + 32 * ks + j];
                    }
                }
            EXPECT(sum > 0);
        }
    for (int B : {1, 2, 3, 256, 257, 511, 512}) {
        EXPECT(fb_plan(P, 5, B, 40, 24, false, &why));
        EXPECT(P.NR == (B > 256 ? 2 : 1) && P.grid == (B + P.NR - 1) / P.NR && P.grid <= 256 && (size_t)P.grid * P.NR >= (size_t)B);
    }
    EXPECT(!fb_plan(P, 5, 513, 40, 24, false, &why) && strstr(why, "512"));
    EXPECT(!fb_plan(P, 0, 4, 40, 24, false, &why));
    EXPECT(!fb_plan(P, 5, 0, 40, 24, false, &why));
    EXPECT(!fb_plan(P, 5, 4, 256, 24, false, &why) && strstr(why, "[4,128]"));
    EXPECT(!fb_plan(P, 5, 4, 64, 132, false, &why) && strstr(why, "[4,128]"));
    EXPECT(!fb_plan(P, 5, 4, 42, 24, false, &why) && strstr(why, "multiple of 4"));
    printf(fails ? "%d checks FAILED\n" : "fb_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
