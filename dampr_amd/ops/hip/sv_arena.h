// Row access to a var-len byte arena (gpu/strvals.py: blob + offs), shared
// by the string-key kernels (dampr_strkeys.hip) and the string row filter
// (dampr_strfilter.hip).
//
// Loads: row starts have arbitrary byte alignment and the arena itself may
// be a byte-offset view.  A word is read as one or two 8-byte loads at
// ABSOLUTE 8-byte-aligned addresses and funnel-shifted, only when those
// aligned words lie wholly inside [blob, blob + blob_n); at the arena's
// edges it is assembled from byte loads of the row's own bytes.  No load
// touches an address outside the arena.
#pragma once

#include "common.h"

// Little-endian u64 of the ``nvalid`` (1..8) bytes at ``p``, zero-padded.
// [p, p + nvalid) must lie inside [base, end).
__device__ __forceinline__ u64 sv_load_word(const u8* p, int nvalid,
                                            const u8* base, const u8* end) {
    const uintptr_t a = (uintptr_t)p;
    const u32 sh = (u32)(a & 7);
    const uintptr_t a0 = a - sh;
    const bool need_hi = sh + (u32)nvalid > 8;
    u64 w;
    if (a0 >= (uintptr_t)base &&
        a0 + (need_hi ? 16 : 8) <= (uintptr_t)end) {
        w = *(const u64*)a0 >> (8 * sh);
        if (need_hi)                      // implies sh >= 1
            w |= *(const u64*)(a0 + 8) << (64 - 8 * sh);
    } else {
        w = 0;
        for (int k = 0; k < nvalid; ++k) w |= (u64)p[k] << (8 * k);
    }
    if (nvalid < 8) w &= (1ULL << (8 * nvalid)) - 1;
    return w;
}

// Row r's byte range, clamped into the arena (offsets are trusted to be
// monotone; the clamp keeps a corrupt column from reading out of bounds).
__device__ __forceinline__ void sv_row(const long* __restrict__ offs, long r,
                                       long blob_n, long* b, long* len) {
    long lo = offs[r], hi = offs[r + 1];
    lo = lo < 0 ? 0 : (lo > blob_n ? blob_n : lo);
    hi = hi < lo ? lo : (hi > blob_n ? blob_n : hi);
    *b = lo;
    *len = hi - lo;
}
