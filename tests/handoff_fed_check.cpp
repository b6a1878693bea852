// g++ check of the second answer of the hand-off tracker (mpyc_amd/csrc/handoff.hpp): does a launch read what the last
// launch on its stream wrote and kept -- operands that the Infinity Cache may hold, as against cold ones.
// Prints "handoff fed ok" and exits 0, or names the first failed check and exits 1.  Driven by tests/test_handoff_fed_host.py.
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

static HandoffTracker h;
// one launch with one output range: its two answers as keep + 2 * fed
static int go(const void* s, int kind, const ByteRange* in, int nin, const ByteRange& out) {
    int fed = -1;
    const int keep = h.launch(s, kind, in, nin, &out, 1, &fed);
    if (fed != 0 && fed != 1) return -1;
    return keep + 2 * fed;
}
enum { STREAM_COLD = 0, KEEP_COLD = 1, STREAM_FED = 2, KEEP_FED = 3 };

int main() {
    const void* s0 = (const void*)0x10;
    const void* s1 = (const void*)0x20;
    const ByteRange a = R(0x100000, 0x200000), b = R(0x200000, 0x300000), c = R(0x300000, 0x400000);
    const ByteRange sh = R(0x400000, 0x700000), y = R(0x700000, 0x800000), sh2 = R(0x800000, 0xb00000);
    const ByteRange ab[2] = {a, b};

    // the answer is optional: without it the call is the one tests/handoff_check.cpp makes
    h.reset();
    CHECK(h.launch(s0, HK_SPLIT, ab, 2, &sh, 1) == 0);

    // a fed launch.  The headline step: split, recombine, split, recombine ... on one stream
    h.reset();
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == STREAM_COLD);    // nothing before it
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_COLD);      // reads the shares, but they were streamed: nothing to find
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == KEEP_COLD);      // does not read y
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_FED);       // the shares were kept for it
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == KEEP_COLD);
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_FED);
    // one row of three is enough, and a second operand that is cold does not change it
    const ByteRange row1_a[2] = {a, R(0x500000, 0x600000)};
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == KEEP_COLD);
    CHECK(go(s0, HK_REC, row1_a, 2, y) == STREAM_FED);
    // a chain in which every launch reads the one before: split -> rec -> split (of y) -> rec
    h.reset();
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == STREAM_COLD);
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_COLD);
    CHECK(go(s0, HK_SPLIT, &y, 1, sh2) == KEEP_COLD);     // reads y, which was streamed; settles REC -> keep
    CHECK(go(s0, HK_REC, &sh2, 1, y) == KEEP_FED);
    CHECK(go(s0, HK_SPLIT, &y, 1, sh) == KEEP_FED);
    CHECK(go(s0, HK_REC, &sh, 1, y) == KEEP_FED);

    // an unfed launch: it reads other arrays, or the bytes right after the outputs, or nothing at all
    h.reset();
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == STREAM_COLD);
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_COLD);
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == KEEP_COLD);
    CHECK(go(s0, HK_EW, ab, 2, c) == STREAM_COLD);        // kept shares that nobody reads
    CHECK(go(s0, HK_SPLIT, &c, 1, sh) == STREAM_COLD);    // SPLIT streams again; c was streamed
    CHECK(go(s0, HK_EW, ab, 2, c) == KEEP_COLD);
    CHECK(go(s0, HK_SPLIT, &c, 1, sh) == STREAM_FED);
    CHECK(go(s0, HK_EW, &y, 1, c) == KEEP_COLD);          // y = [0x700000, ...) starts where the kept shares end
    CHECK(go(s0, HK_COPY, nullptr, 0, y) == STREAM_COLD);
    // an empty operand range inside the outputs is not read
    const ByteRange empty = R(0x750000, 0x750000);
    CHECK(go(s0, HK_EW, &empty, 1, c) == STREAM_COLD);

    // a launch on another stream: neither fed by s0's outputs nor in the way of s0's own consumer
    h.reset();
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == STREAM_COLD);
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_COLD);
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == KEEP_COLD);
    CHECK(go(s1, HK_REC, &sh, 1, y) == STREAM_COLD);      // s1 has no launch before it
    CHECK(go(s1, HK_REC, &sh, 1, y) == STREAM_COLD);      // and its own last launch did not write the shares
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_FED);       // s0's record stood through the s1 launches

    // outputs larger than the cache are streamed whatever the prediction: their consumer finds nothing
    h.reset();
    const ByteRange big = R(0x10000000, 0x10000000 + HandoffTracker::MAX_KEEP_BYTES + 16);
    const ByteRange fit = R(0x10000000, 0x10000000 + HandoffTracker::MAX_KEEP_BYTES);
    CHECK(go(s0, HK_SPLIT, ab, 2, big) == STREAM_COLD);
    CHECK(go(s0, HK_REC, &big, 1, y) == STREAM_COLD);
    CHECK(go(s0, HK_SPLIT, ab, 2, big) == STREAM_COLD);   // predicted to feed, too large to keep
    CHECK(go(s0, HK_REC, &big, 1, y) == STREAM_COLD);
    CHECK(go(s0, HK_SPLIT, ab, 2, fit) == KEEP_COLD);     // exactly the cache
    CHECK(go(s0, HK_REC, &fit, 1, y) == STREAM_FED);

    // lane eviction: a stream pushed out of the tracker comes back knowing nothing
    h.reset();
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == STREAM_COLD);
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_COLD);
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == KEEP_COLD);
    for (int i = 0; i < HandoffTracker::STREAMS; ++i)     // STREAMS other streams: s0 is the oldest and goes
        CHECK(go((const void*)(uintptr_t)(0x2000 + i), HK_EW, ab, 2, c) == STREAM_COLD);
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_COLD);      // the kept shares are forgotten: read as cold
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == STREAM_COLD);
    // with one lane to spare nothing is lost
    h.reset();
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == STREAM_COLD);
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_COLD);
    CHECK(go(s0, HK_SPLIT, ab, 2, sh) == KEEP_COLD);
    for (int i = 0; i < HandoffTracker::STREAMS - 1; ++i)
        CHECK(go((const void*)(uintptr_t)(0x2000 + i), HK_EW, ab, 2, c) == STREAM_COLD);
    CHECK(go(s0, HK_REC, &sh, 1, y) == STREAM_FED);

    if (fails) return 1;
    printf("handoff fed ok\n");
    return 0;
}
