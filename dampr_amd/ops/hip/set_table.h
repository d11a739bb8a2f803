// Device hash sets the row filters probe for their isin / notin clauses
// (dampr_filter.hip, dampr_strfilter.hip).  Built once per filter stage,
// read-only while a filter runs.
//
// Numeric set: an open-addressing table of u64 words, power-of-two capacity
// >= 2 * members and >= SET_MIN_CAPACITY, EMPTY = 0, linear probing from
// splitmix64(word) & mask.  The slot comes from the mixed word because
// member sets are often strided ids that share their low bits.  The word
// that collides with EMPTY is never remapped (that would alias 0 with
// another member): it is never stored, and "zero is a member" travels as a
// flag in the clause.
//
// String set: the members' own arena, their sv_hash64 hashes, and an i32
// slot table that holds member index + 1 (0 = EMPTY), linear probing from
// hash & mask.  Distinct members that share a hash occupy two slots; a row
// hits only when hash, length and every byte agree, so the answer is exact
// under hash collisions and only hash-equal candidates pay the byte loop.
//
// Every probe and insert loop runs at most ``capacity`` steps: a malformed
// table (full, or never zeroed) can give a wrong answer, never a spin.
#pragma once

#include "common.h"
#include "sv_arena.h"

#define SET_MIN_CAPACITY 16
#define SET_MAX_MEMBERS (1L << 30)

// Smallest legal capacity for m members (gpu/filters.py set_capacity).
inline long set_capacity_for(long m) {
    long cap = SET_MIN_CAPACITY;
    while (cap < 2 * m) cap <<= 1;
    return cap;
}

// Is w (never 0: the caller answers that from the clause's flag) in the
// table?
__device__ __forceinline__ bool set_has_u64(const u64* __restrict__ tab,
                                            u64 mask, u64 w) {
    u64 slot = splitmix64(w) & mask;
    for (u64 step = 0; step <= mask; ++step) {
        const u64 cur = tab[slot];
        if (cur == w) return true;
        if (cur == 0ULL) return false;
        slot = (slot + 1) & mask;
    }
    return false;
}

// table_insert_u64's sibling: starts at the mixed slot, bounded, no result.
__device__ __forceinline__ void set_insert_u64(u64* __restrict__ tab,
                                               u64 mask, u64 w) {
    u64 slot = splitmix64(w) & mask;
    for (u64 step = 0; step <= mask; ++step) {
        const u64 cur = tab[slot];
        if (cur == w) return;
        if (cur == 0ULL) {
            const u64 prev = atomicCAS(&tab[slot], 0ULL, w);
            if (prev == 0ULL || prev == w) return;
        }
        slot = (slot + 1) & mask;
    }
}

// The canonical set word of a double: false for NaN (no member equals it),
// -0.0 becomes 0.0 (the word 0, answered by the clause's flag).
__device__ __forceinline__ bool set_word_f64(long long bits, u64* w) {
    const double x = __longlong_as_double(bits);
    if (x != x) return false;
    *w = x == 0.0 ? 0ULL : (u64)bits;
    return true;
}

struct SvSet {
    const u8* blob;          // the members' arena
    long blob_n;
    const long* offs;        // m + 1
    long m;
    const u64* hashes;       // sv_hash64 of the members, m
    const int* slots;        // mask + 1: member index + 1, 0 = EMPTY
    u64 mask;
    const u64* row_hash;     // sv_hash64 of the filtered rows, same hash mask
};

// Is the row [b, b + len) of the arena [rblob, rend), whose hash is h, a
// member?
__device__ __forceinline__ bool sv_set_has(const SvSet& s, u64 h,
                                           const u8* rblob, const u8* rend,
                                           long b, long len) {
    const u8* mend = s.blob + s.blob_n;
    u64 slot = h & s.mask;
    for (u64 step = 0; step <= s.mask; ++step) {
        const long j = (long)s.slots[slot] - 1;
        if (j < 0) return false;
        if (j < s.m && s.hashes[j] == h) {
            long mb, mlen;
            sv_row(s.offs, j, s.blob_n, &mb, &mlen);
            if (mlen == len) {
                bool same = true;
                for (long o = 0; o < len && same; o += 8) {
                    const int nv = len - o < 8 ? (int)(len - o) : 8;
                    same = sv_load_word(rblob + b + o, nv, rblob, rend) ==
                           sv_load_word(s.blob + mb + o, nv, s.blob, mend);
                }
                if (same) return true;
            }
        }
        slot = (slot + 1) & s.mask;
    }
    return false;
}

// Member i (of m) into the slot table, at its hash's first free slot.
__device__ __forceinline__ void sv_set_insert(int* __restrict__ slots,
                                              u64 mask, u64 h, long i) {
    u64 slot = h & mask;
    for (u64 step = 0; step <= mask; ++step) {
        if (slots[slot] == 0 &&
            atomicCAS(&slots[slot], 0, (int)(i + 1)) == 0)
            return;
        slot = (slot + 1) & mask;
    }
}
