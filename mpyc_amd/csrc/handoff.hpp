// handoff.hpp -- host-side hand-off tracker: which launches should leave their outputs in the Infinity Cache for the next
// launch on the same stream.  Plain C++ (no HIP): api.hip holds one per context, tests/handoff_check.cpp drives it with g++.
//
// Streamed outputs carry the non-temporal hint and do not stay in the 256 MiB Infinity Cache, so a consumer launched right
// after its producer reads them back from HBM.  Stored with the default policy they stay there (dirty) and the consumer finds
// them: 3 rows of 80 MB written, then read by the next launch, 139.5 -> 119.2 us for the pair (tools/tune_handoff.hip,
// profiles/r07_handoff.md).  Stored that way but NOT read next, they cost the producer 85 -> 91 us.  So the default policy
// pays only where a consumer follows, and that is what the tracker predicts, per stream and per producer kind:
//   * it remembers the byte ranges the last tracked launch on a stream wrote, and that launch's kind;
//   * the next launch on that stream tells whether it reads any of them: that settles, for the producer's kind, whether
//     the next producer of that kind keeps its outputs (default stores) or streams them (nt);
//   * outputs larger than the cache never keep: the producer would evict its own first rows before anyone reads them.
// Kept outputs of share generation are stored write-through (sc1) instead: they stay in the cache all the same and the
// producer leaves no dirty lines to write back when it ends, pair 117.7 -> 115.6 us (profiles/r19_handoff_account.md; the
// flavour per kind is chosen where the tracker is asked, CallScope in api.hip).  The tracker also says whether a launch
// reads what the launch before it kept, i.e. operands that the cache may hold: r19 measured the loads of such operands and
// of cold ones with every hint, nt won for both, so today no kernel treats the two differently.
// The tracked calls (api.hip, the tracked form of CallScope): element-wise operations, share generation (supplied coefficients, device RNG, the
// chain gate), recombination, device copy.  Launches of other calls are not seen: a split, a pow, then a recombination of the
// shares counts as a hand-off from the split.
// Host bookkeeping only: no synchronisation, no allocation, no device call.  A wrong guess costs speed, never a result --
// every store policy writes the same bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ffgpu {

struct ByteRange {
    uintptr_t lo, hi;    // [lo, hi)
};
inline ByteRange byte_range(const void* p, size_t bytes) {
    const uintptr_t lo = (uintptr_t)p;
    return {lo, lo + bytes};
}
inline bool overlaps(const ByteRange& a, const ByteRange& b) { return a.lo < b.hi && b.lo < a.hi && a.lo < a.hi && b.lo < b.hi; }

// producer kinds (what the prediction is kept for)
enum HandoffKind { HK_EW = 0, HK_SPLIT = 1, HK_REC = 2, HK_COPY = 3, HK_KINDS = 4 };

struct HandoffTracker {
    enum { STREAMS = 8, ROWS = 8 };
    static constexpr size_t MAX_KEEP_BYTES = (size_t)256 << 20;     // the Infinity Cache
    struct Lane {
        const void* stream;
        uint64_t stamp;                // last use (the least recently used lane goes to a new stream)
        int used;
        int kind;                      // of the last launch; its outputs:
        int nout;
        int kept;                      // ... were kept, not streamed (they may still sit in the cache)
        ByteRange out[ROWS];
        uint8_t keep[HK_KINDS];        // did the last output of this kind feed the next launch?
    } lanes[STREAMS];
    uint64_t clock;

    void reset() {
        for (Lane& l : lanes) {
            l.stream = nullptr;
            l.stamp = 0;
            l.used = 0;
            l.kind = 0;
            l.nout = 0;
            l.kept = 0;
            for (uint8_t& k : l.keep) k = 0;
        }
        clock = 0;
    }
    Lane& lane_of(const void* stream) {
        Lane* victim = nullptr;      // a free lane, else the least recently used one
        for (Lane& l : lanes) {
            if (l.used && l.stream == stream) return l;
            if (!victim || (!l.used && victim->used) || (l.used == victim->used && l.stamp < victim->stamp)) victim = &l;
        }
        Lane& l = *victim;
        l.stream = stream;
        l.used = 1;
        l.nout = 0;
        l.kept = 0;
        for (uint8_t& k : l.keep) k = 0;
        return l;
    }
    // A launch of `kind` on `stream` reads `in` and writes `out`.  Returns 1 if it should store its outputs with the
    // default cache policy (its kind fed the next launch last time and the outputs fit the cache), 0 for non-temporal.
    // (More than ROWS outputs: the first ROWS are remembered.)  *fed_in: 1 if this launch reads what the last launch on the
    // stream wrote AND that launch kept it -- operands that the cache may hold; 0 if all its operands are cold.
    int launch(const void* stream, int kind, const ByteRange* in, int nin, const ByteRange* out, int nout, int* fed_in = nullptr) {
        Lane& l = lane_of(stream);
        l.stamp = ++clock;
        bool fed = false;
        if (l.nout > 0) {
            for (int i = 0; i < nin && !fed; ++i)
                for (int j = 0; j < l.nout && !fed; ++j) fed = overlaps(in[i], l.out[j]);
            l.keep[l.kind] = fed ? 1 : 0;
        }
        if (fed_in) *fed_in = fed && l.kept;
        size_t bytes = 0;
        for (int j = 0; j < nout; ++j) bytes += out[j].hi > out[j].lo ? out[j].hi - out[j].lo : 0;
        const int keep = l.keep[kind] && bytes <= MAX_KEEP_BYTES;
        l.kind = kind;
        l.kept = keep;
        l.nout = nout < ROWS ? nout : ROWS;
        for (int j = 0; j < l.nout; ++j) l.out[j] = out[j];
        return keep;
    }
};

}  // namespace ffgpu
