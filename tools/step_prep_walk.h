// For the stand-alone plan checkers: walk the job table that a prepare entry really launches (csrc/step_prep.h) through the kernel's own
// index function, over a byte map of the state.  No source is dereferenced.  Returns the number of failed checks (printed):
//   the counts are within the table's capacity and `most` is the largest matrix job;
//   every byte a job writes lies inside ONE region of the plan, the one its destination starts in, and below dyn_off (the carried
//   state is never prepared);
//   every byte of every region is written exactly once (map[] counts the writes), which covers jobs that interleave rows of one matrix.
#pragma once
#include <stdio.h>
#include <vector>
#include "../multimodal_transformer_amd/csrc/step_prep.h"

struct PrepRegion { size_t off, len; };

static inline int step_prep_walk(const StepPrepParams& T, size_t most, const std::vector<PrepRegion>& regions, size_t dyn_off,
                                 unsigned char* map) {
    int bad = 0;
    auto expect = [&](bool ok, const char* what, int job) { if (!ok) { printf("FAILED prepare table: %s (job %d)\n", what, job); ++bad; } };
    expect(T.nmat >= 0 && T.nmat <= MMT_STEP_PREP_MATS && T.nvec >= 0 && T.nvec <= MMT_STEP_PREP_VECS, "counts within capacity", -1);
    if (bad) return bad;
    auto region_of = [&](size_t byte) -> const PrepRegion* {
        for (const PrepRegion& r : regions) if (byte >= r.off && byte - r.off < r.len) return &r;
        return nullptr;
    };
    auto write = [&](const PrepRegion* r, size_t byte, size_t n, int job) {
        const bool inside = r && byte >= r->off && byte + n <= r->off + r->len && byte + n <= dyn_off;
        if (!inside) { if (bad < 8) expect(false, "a write outside the job's region", job); else ++bad; return; }
        for (size_t i = 0; i < n; ++i) map[byte + i] += 1;
    };
    size_t largest = 1;
    for (int job = 0; job < T.nmat; ++job) {
        const StepPrepMat& J = T.mat[job];
        expect(J.src && J.rows > 0 && J.K > 0 && J.KP >= J.K && J.KP % 8 == 0 && J.KP - J.K < 8 && J.nout >= J.rows, "a matrix job's shape", job);
        const PrepRegion* r = region_of(J.dst);
        expect(r != nullptr, "the destination starts in no region", job);
        const size_t total = (size_t)J.rows * J.KP;
        if (total > largest) largest = total;
        for (size_t i = 0; i < total; ++i) {
            const StepPrepAt at = step_prep_at(J, i);
            expect(at.n >= 0 && at.n < J.rows && at.k >= 0 && at.k < J.KP, "the index function's (n, k)", job);
            write(r, J.dst + at.dst * 2, 2, job);                              // one bf16
        }
    }
    expect(largest == most, "most is the largest matrix job", -1);
    for (int job = 0; job < T.nvec; ++job) {
        const StepPrepVec& J = T.vec[job];
        expect(J.a && J.n > 0 && J.dst % 4 == 0, "a vector job's shape", T.nmat + job);
        const PrepRegion* r = region_of(J.dst);
        expect(r != nullptr, "the destination starts in no region", T.nmat + job);
        for (int i = 0; i < J.n; ++i) write(r, J.dst + (size_t)4 * i, 4, T.nmat + job);   // one float
    }
    for (const PrepRegion& r : regions) {
        bool once = true;
        for (size_t i = 0; i < r.len; ++i) once = once && map[r.off + i] == 1;
        if (!once) { printf("FAILED prepare table: the region at byte %zu is not written exactly once\n", r.off); ++bad; }
    }
    return bad;
}
