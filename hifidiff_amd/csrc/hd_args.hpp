// hd_args.hpp -- the argument-check vocabulary of the entry points that take caller buffers (hd_image.hip, hd_photo.hip, hd_lpips.hip and
// the VAE boundary of hd_aux.hip).  Host only, and nothing from hd_internal.hpp: a unit without a context can include it on its own.
#pragma once
#include <cstdio>
#include <string>

#include "../../include/hifidiff_hip.h"

void set_contextless_error(const std::string& msg);               // hd_lib.hip: the message hd_last_error(NULL) returns

// An entry point without a context fails into the slot hd_last_error(NULL) reads
#define HD_ARG_FAIL(code, ...)                                    \
    do {                                                          \
        char _b[256];                                             \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                    \
        set_contextless_error(_b);                                \
        return (code);                                            \
    } while (0)

namespace hd_args {

// an image side: a multiple of 64 in [64, 512] (64-bit, so that a caller's 8 * latent_res cannot wrap into the range)
inline bool res_ok(long long r) { return r >= 64 && r <= 512 && r % 64 == 0; }

// a caller buffer by the name its entry point gives it; ptr NULL or bytes 0: absent, overlaps nothing
struct ByteRange { const char* name; const void* ptr; size_t bytes; };

inline bool overlap(const ByteRange& a, const ByteRange& b) {
    const uintptr_t pa = (uintptr_t)a.ptr, pb = (uintptr_t)b.ptr;
    return pa && pb && a.bytes && b.bytes && pa < pb + b.bytes && pb < pa + a.bytes;
}

// The first overlapping pair, every output against every input and then the outputs pairwise; false: none.  The caller words the message.
inline bool first_overlap(const ByteRange* outs, int n_out, const ByteRange* ins, int n_in, const ByteRange** a, const ByteRange** b) {
    for (int o = 0; o < n_out; ++o)
        for (int i = 0; i < n_in; ++i)
            if (overlap(outs[o], ins[i])) { *a = &outs[o]; *b = &ins[i]; return true; }
    for (int i = 0; i < n_out; ++i)
        for (int j = i + 1; j < n_out; ++j)
            if (overlap(outs[i], outs[j])) { *a = &outs[i]; *b = &outs[j]; return true; }
    return false;
}

}  // namespace hd_args
