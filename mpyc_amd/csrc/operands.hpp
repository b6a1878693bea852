// operands.hpp -- the arrays of one call of a secure entry, each stated once: the pointer together with the bytes the call
// touches behind it.  Plain C++ (no HIP, no allocation): api.hip builds one per call on the stack, tests/api_args_check.cpp
// drives it with g++ on synthetic addresses.
// An entry names every array by what the call does with it -- in / out / inout, a host array of device pointers, a host
// array the launcher reads -- and asks once, ok(): every required pointer was there, no output meets an input (but for a
// stated alias) and no output meets another output.  An array updated in place counts as an output: the rows and the
// other outputs must stay clear of it.  Empty ranges meet nothing (overlaps, handoff.hpp).
#pragma once
#include "handoff.hpp"

namespace ffgpu {

struct Operands {
    // the largest callers: ffgm_conv2d (x, w, b of 64 senders in, 64 out), ffgm_rbits_open (r, z of 64 rows in)
    enum { MAX_IN = 3 * 64 + 8, MAX_OUT = 64 + 8, NO_ALIAS = -1 };
    ByteRange in_[MAX_IN], out_[MAX_OUT];
    int alias_[MAX_OUT];           // the input this output may coincide with (same address), or NO_ALIAS
    int nin, nout;
    bool refused;                  // a required pointer was null, or more arrays than fit

    Operands() : nin(0), nout(0), refused(false) {}        // (the ranges stay as they are: only the first nin, nout are read)

    // inputs
    Operands& in(const void* p, size_t bytes) {
        if (!p) refused = true;
        return push_in(p, bytes);
    }
    Operands& in_opt(const void* p, size_t bytes) { return p ? push_in(p, bytes) : *this; }     // null: not given
    // a host array of `count` device pointers, `bytes` behind each: the array and every entry must be there; *first (if
    // given) gets the index of the first row among the inputs, to name the rows as aliases
    Operands& in_rows(const void* const* rows, int count, size_t bytes, int* first = nullptr) {
        if (first) *first = nin;
        if (!rows) refused = true;
        for (int i = 0; rows && i < count; ++i) in(rows[i], bytes);
        return *this;
    }
    // a host array the launcher reads (coefficients, scalars): it only has to be there
    Operands& host(const void* p) {
        if (!p) refused = true;
        return *this;
    }
    // outputs; alias: the index of the one input the output may coincide with, at the same address
    Operands& out(const void* p, size_t bytes, int alias = NO_ALIAS) {
        if (!p) refused = true;
        return push_out(p, bytes, alias);
    }
    Operands& out_opt(const void* p, size_t bytes) { return p ? push_out(p, bytes, NO_ALIAS) : *this; }
    Operands& inout(const void* p, size_t bytes) { return out(p, bytes); }
    // a host array of `count` device pointers written; alias_first: row i may coincide with input alias_first + i
    Operands& out_rows(void* const* rows, int count, size_t bytes, int alias_first = NO_ALIAS) {
        if (!rows) refused = true;
        for (int i = 0; rows && i < count; ++i) out(rows[i], bytes, alias_first == NO_ALIAS ? NO_ALIAS : alias_first + i);
        return *this;
    }

    bool ok() const {
        if (refused) return false;
        for (int j = 0; j < nout; ++j) {
            for (int i = 0; i < nin; ++i)
                if (overlaps(out_[j], in_[i]) && !(i == alias_[j] && out_[j].lo == in_[i].lo)) return false;
            for (int i = 0; i < j; ++i)
                if (overlaps(out_[j], out_[i])) return false;
        }
        return true;
    }

  private:
    Operands& push_in(const void* p, size_t bytes) {
        if (nin == MAX_IN) refused = true;
        else in_[nin++] = byte_range(p, bytes);
        return *this;
    }
    Operands& push_out(const void* p, size_t bytes, int alias) {
        if (nout == MAX_OUT) refused = true;
        else {
            out_[nout] = byte_range(p, bytes);
            alias_[nout++] = alias;
        }
        return *this;
    }
};

}  // namespace ffgpu
