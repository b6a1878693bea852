// g++ check of the hand-off tracker (mpyc_amd/csrc/handoff.hpp): the overlap rule and the per-stream, per-kind prediction.
// Prints "handoff ok" and exits 0, or names the first failed check and exits 1.  Driven by tests/test_handoff_host.py.
#include <stdio.h>
#include "../mpyc_amd/csrc/handoff.hpp"

using namespace ffgpu;

static int fails = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED line %d: %s\n", __LINE__, #cond);         \
            ++fails;                                                 \
        }                                                            \
    } while (0)

static ByteRange R(uintptr_t lo, uintptr_t hi) { return {lo, hi}; }

int main() {
    // overlap: half-open ranges, empty ranges overlap nothing
    CHECK(overlaps(R(0, 100), R(99, 200)));
    CHECK(!overlaps(R(0, 100), R(100, 200)));
    CHECK(!overlaps(R(100, 200), R(0, 100)));
    CHECK(overlaps(R(0, 1000), R(10, 20)));
    CHECK(overlaps(R(10, 20), R(0, 1000)));
    CHECK(!overlaps(R(50, 50), R(0, 100)));
    CHECK(byte_range((const void*)0x1000, 16).hi == 0x1010);

    static HandoffTracker h;
    h.reset();
    const void* s0 = (const void*)0x10;
    const void* s1 = (const void*)0x20;
    const ByteRange a = R(0x100000, 0x200000), b = R(0x200000, 0x300000), c = R(0x300000, 0x400000);
    const ByteRange sh = R(0x400000, 0x700000), y = R(0x700000, 0x800000);
    const ByteRange ab[2] = {a, b};

    // first producer on a stream: nothing known, streamed (nt)
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);
    // the consumer reads the shares: settles SPLIT -> keep; its own kind is still unknown
    CHECK(h.launch(s0, HK_REC, &sh, 1, &y, 1) == 0);
    // the next split does not read y: REC -> stream; SPLIT keeps
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 1);
    CHECK(h.launch(s0, HK_REC, &sh, 1, &y, 1) == 0);
    // a split whose outputs nobody reads next: the following split streams again
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 1);
    CHECK(h.launch(s0, HK_EW, ab, 2, &c, 1) == 0);       // reads a, b, not the shares: SPLIT -> stream; EW unknown
    CHECK(h.launch(s0, HK_SPLIT, &c, 1, &sh, 1) == 0);   // reads c: EW -> keep
    CHECK(h.launch(s0, HK_EW, ab, 2, &c, 1) == 1);       // EW keeps; the split's shares went unread: SPLIT -> stream
    CHECK(h.launch(s0, HK_SPLIT, &c, 1, &sh, 1) == 0);
    CHECK(h.launch(s0, HK_REC, &sh, 1, &y, 1) == 0);     // SPLIT -> keep
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 1);

    // a partial overlap counts: the consumer reads one row of three
    h.reset();
    const ByteRange row1 = R(0x500000, 0x600000);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);
    CHECK(h.launch(s0, HK_REC, &row1, 1, &y, 1) == 0);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 1);
    // touching is not overlapping: a consumer of the bytes right after the outputs
    CHECK(h.launch(s0, HK_REC, &y, 1, &c, 1) == 0);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);

    // streams are tracked apart: a launch on s1 neither settles nor disturbs s0
    h.reset();
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);
    CHECK(h.launch(s1, HK_REC, &sh, 1, &y, 1) == 0);     // other stream: s0's split stays unsettled
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);
    CHECK(h.launch(s0, HK_REC, &sh, 1, &y, 1) == 0);
    CHECK(h.launch(s1, HK_EW, ab, 2, &c, 1) == 0);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 1);   // s0 kept its record across the s1 launch

    // kinds are predicted apart
    h.reset();
    CHECK(h.launch(s0, HK_EW, ab, 2, &c, 1) == 0);
    CHECK(h.launch(s0, HK_COPY, &c, 1, &y, 1) == 0);     // EW -> keep
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);   // SPLIT unknown; COPY -> stream
    CHECK(h.launch(s0, HK_EW, ab, 2, &c, 1) == 1);

    // outputs larger than the cache always stream
    h.reset();
    const ByteRange big = R(0x10000000, 0x10000000 + HandoffTracker::MAX_KEEP_BYTES + 16);
    const ByteRange fit = R(0x10000000, 0x10000000 + HandoffTracker::MAX_KEEP_BYTES);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &big, 1) == 0);
    CHECK(h.launch(s0, HK_REC, &big, 1, &y, 1) == 0);    // consumed: SPLIT -> keep ...
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &big, 1) == 0);  // ... but too large
    CHECK(h.launch(s0, HK_REC, &big, 1, &y, 1) == 0);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &fit, 1) == 1);  // exactly the cache: kept
    // the cap counts all output ranges together
    const ByteRange halves[2] = {R(0x10000000, 0x10000000 + HandoffTracker::MAX_KEEP_BYTES / 2 + 16),
                                 R(0x30000000, 0x30000000 + HandoffTracker::MAX_KEEP_BYTES / 2)};
    CHECK(h.launch(s0, HK_REC, &fit, 1, &y, 1) == 0);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, halves, 2) == 0);

    // more outputs than ROWS: the first ROWS are remembered
    h.reset();
    ByteRange many[HandoffTracker::ROWS + 2];
    for (int j = 0; j < HandoffTracker::ROWS + 2; ++j) many[j] = R(0x1000000 + 0x10000 * j, 0x1000000 + 0x10000 * j + 0x100);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, many, HandoffTracker::ROWS + 2) == 0);
    CHECK(h.launch(s0, HK_REC, &many[HandoffTracker::ROWS - 1], 1, &y, 1) == 0);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, many, HandoffTracker::ROWS + 2) == 1);
    CHECK(h.launch(s0, HK_REC, &many[HandoffTracker::ROWS], 1, &y, 1) == 0);      // not remembered: not a hand-off
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, many, HandoffTracker::ROWS + 2) == 0);

    // more streams than lanes: the least recently used lane is taken over and starts afresh
    h.reset();
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);
    CHECK(h.launch(s0, HK_REC, &sh, 1, &y, 1) == 0);     // s0: SPLIT -> keep
    for (int i = 0; i < HandoffTracker::STREAMS - 1; ++i)
        CHECK(h.launch((const void*)(uintptr_t)(0x1000 + i), HK_EW, ab, 2, &c, 1) == 0);
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 1);   // all lanes in use, s0 still among them
    for (int i = 0; i < HandoffTracker::STREAMS; ++i)    // STREAMS new streams: s0 (the oldest by then) is pushed out
        CHECK(h.launch((const void*)(uintptr_t)(0x2000 + i), HK_EW, ab, 2, &c, 1) == 0);
    CHECK(h.launch(s0, HK_REC, &sh, 1, &y, 1) == 0);     // a fresh lane: nothing to settle
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);   // and nothing known about SPLIT

    if (fails) return 1;
    printf("handoff ok\n");
    return 0;
}
