// Slots of a stream: the position of every sequence lives in device memory, int pos[B], and the positioned forms of the step kernels
// (encoder_step_slots_kernel, mfn_step_slots_kernel) read it, run the window at that position and advance it themselves.  A step then
// has no host-side position, so it can be captured into a graph and replayed, and the sequences of a batch need not start together.
//
// Values of pos[b]:
//   p < 0                 idle: no recording is seated in the slot
//   0 <= p < limit        seated; the next window of the recording is window p.  Seating a slot is pos[b] = 0 and nothing else: at
//                         position 0 the step kernels read no carried state and no cache row
//   p >= limit            full (the encoder's limit is the capacity of its K/V cache; limit <= 0: no limit).  The kernel leaves the value
//                         as it is, so the host can see it
//   INT_MAX               never run, with or without a limit: p + 1 would not be a position
// An idle or full slot is SKIPPED: its workgroup writes its row of the output as zeros and nothing else.
//
// slot_decode is the ONE place where a value read from device memory becomes a position: every address that a positioned kernel derives
// from pos[b] is formed from what this function returned, with `limit` taken from the launch arguments.  Plain C++ for the host and the
// device, so that a stand-alone program can walk it (tools/slot_pos_check.cpp).
#pragma once
#include <limits.h>

#if defined(__HIPCC__)
#define MMT_SLOT_HD __host__ __device__
#else
#define MMT_SLOT_HD
#endif

#define MMT_SLOT_IDLE (-1)                // what release() stores
#define MMT_SLOT_SKIP (-1)                // slot_decode: do not run this slot

// (p, limit) -> the position to run, in [0, limit) and below INT_MAX, or MMT_SLOT_SKIP
MMT_SLOT_HD static inline int slot_decode(int p, int limit) {
    if (p < 0 || p == INT_MAX) return MMT_SLOT_SKIP;
    if (limit > 0 && p >= limit) return MMT_SLOT_SKIP;
    return p;
}
