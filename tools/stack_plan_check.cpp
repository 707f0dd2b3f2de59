// Stand-alone host check of the stacked LSTM scan's limits and workspace layout (csrc/scan_stack_plan.h): no HIP, no GPU.
//   c++ -std=c++17 -fsanitize=address,undefined -o tools/bin/stack_plan_check tools/stack_plan_check.cpp && tools/bin/stack_plan_check
// Walks every accepted (H, L, B) and the refused neighbours; carves a host buffer of the queried size and touches every fragment
// element the preparation kernel would write, so that an offset or size mistake is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../multimodal_transformer_amd/csrc/scan_stack_plan.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

int main() {
    const char* why = nullptr;
    StackPlan P;
    for (int L = 0; L <= 6; ++L)
        for (int H = -4; H <= 136; ++H) {
            const bool ok = stack_plan(P, 0, 0, H, L, true, &why);
            EXPECT(ok == (L >= 2 && L <= 4 && H > 0 && H <= 128 && H % 4 == 0));
            if (!ok) { EXPECT(why && strstr(why, "stacked LSTM scan")); continue; }
            EXPECT(P.HP16 >= H && P.HP16 % 16 == 0 && P.HP16 <= P.HPAD && (P.HPAD == 64 || P.HPAD == 128));
            EXPECT(P.block == 64 * (P.HP16 / 16) && P.block <= (P.HPAD == 64 ? 256 : 512));
            EXPECT(P.pb_off >= P.pf_off + 2 * P.pf_elems && P.bytes >= P.pb_off + 2 * P.pb_elems && P.pb_off % 256 == 0);
            std::vector<unsigned short> ws(P.bytes / 2);                   // bf16 elements: exactly the queried size
            unsigned short* pf = ws.data() + P.pf_off / 2;
            unsigned short* pb = ws.data() + P.pb_off / 2;
            for (size_t i = 0; i < P.pf_elems; ++i) pf[i] = 1;
            for (size_t i = 0; i < P.pb_elems; ++i) pb[i] += 2;            // an overlap with the forward fragments would read 3
            for (size_t i = 0; i < P.pb_elems; ++i) EXPECT(pb[i] == 2);
            // the last fragment reads of the kernels: forward row HP16-1 of gate 3 of layer L-1, k-block 2 HPAD/32 - 1, lane quarter 3
            const size_t lastf = (((size_t)(L - 1) * 4 + 3) * P.HP16 + P.HP16 - 1) * 2 * P.HPAD + 8 * 3 + (2 * P.HPAD / 32 - 1) * 32 + 7;
            const size_t lastb = (((size_t)(L - 1) * 2 + 1) * P.HP16 + P.HP16 - 1) * 4 * P.HPAD + 8 * 3 + (4 * P.HPAD / 32 - 1) * 32 + 7;
            EXPECT(lastf == P.pf_elems - 1 && lastb == P.pb_elems - 1);
        }
    for (int B : {1, 2, 3, 256, 257, 511, 512}) {
        EXPECT(stack_plan(P, 5, B, 40, 3, false, &why));
        EXPECT(P.NR == (B > 256 ? 2 : 1) && P.grid == (B + P.NR - 1) / P.NR && P.grid <= 256 && (size_t)P.grid * P.NR >= (size_t)B);
    }
    EXPECT(!stack_plan(P, 5, 513, 40, 3, false, &why) && strstr(why, "512"));
    EXPECT(!stack_plan(P, 0, 4, 40, 3, false, &why));
    EXPECT(!stack_plan(P, 5, 0, 40, 3, false, &why));
    EXPECT(!stack_plan(P, 5, 4, 256, 2, false, &why) && strstr(why, "128"));
    EXPECT(!stack_plan(P, 5, 4, 64, 5, false, &why) && strstr(why, "[2,4]"));
    printf(fails ? "%d checks FAILED\n" : "stack_plan_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
