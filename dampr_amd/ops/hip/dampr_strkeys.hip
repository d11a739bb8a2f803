// String-key kernels for the dampr_amd device engine (gfx950): the device
// half of the dictionary encode that turns a var-len string VALUE column
// (byte arena: blob + offs, gpu/strvals.py) into dense i64 key ids.
//
//   sv_hash64       row -> strmix64(row) & mask
//   sv_adjacent_eq  over the hash-sorted rows: segment heads, with a byte
//                   compare of hash-equal neighbours (a mismatch there is a
//                   true 64-bit collision; the caller re-encodes exactly)
//   sv_lex_key      row -> the u64 order key of its 7-byte window d (the
//                   twin of keyhash.lex_window_key)
//   sv_lex_refine   over the (group, key)-sorted rows: class heads, and
//                   which rows another window must still decide
//
// Orchestration (radix sort between the two, cumsum + gather after) is
// relational.dict_encode_strs; the last two rank the uniques in byte
// order, round by round, under relational.lex_rank_strs.
//
// Lane mapping: rows are typically short tokens, so a wave per row (as
// varlen_gather does) would idle 63 lanes.  A group of SV_GROUP = 8 lanes
// owns one row and covers 8 lanes x 8 bytes = 64 bytes per iteration; a
// wave64 works on 8 rows at once and combines with three __shfl_xor steps
// that stay inside the group.  The row loops have a block-uniform trip
// count, so every shuffle runs with the whole wave converged.
//
// Row reads go through sv_arena.h (sv_row, sv_load_word): no load touches
// an address outside the arena.
#include <hip/hip_runtime.h>
#include "host.h"
#include "ops.h"

#include "common.h"
#include "sv_arena.h"

#define SV_GROUP 8                        // lanes per row
#define SV_BLOCK 256
#define SV_ROWS (SV_BLOCK / SV_GROUP)     // rows per block iteration

__global__ void sv_hash64_kernel(const u8* __restrict__ blob, long blob_n,
                                 const long* __restrict__ offs, long n,
                                 u64 mask, u64* __restrict__ out) {
    const int g = threadIdx.x & (SV_GROUP - 1);
    const long stride = (long)gridDim.x * SV_ROWS;
    const u8* end = blob + blob_n;
    for (long rb = (long)blockIdx.x * SV_ROWS; rb < n; rb += stride) {
        const long r = rb + threadIdx.x / SV_GROUP;
        long b = 0, len = 0;
        if (r < n) sv_row(offs, r, blob_n, &b, &len);
        const long nw = (len + 7) >> 3;
        u64 h = 0;
        for (long j = g; j < nw; j += SV_GROUP) {
            const long rem = len - 8 * j;
            h ^= strmix_word(
                sv_load_word(blob + b + 8 * j, rem < 8 ? (int)rem : 8,
                             blob, end), (u64)j);
        }
        h ^= __shfl_xor(h, 1);
        h ^= __shfl_xor(h, 2);
        h ^= __shfl_xor(h, 4);
        if (g == 0 && r < n) out[r] = strmix_final(h, (u64)len) & mask;
    }
}

__global__ void sv_adjacent_eq_kernel(const u8* __restrict__ blob,
                                      long blob_n,
                                      const long* __restrict__ offs,
                                      const u64* __restrict__ sorted_hash,
                                      const int* __restrict__ perm, long n,
                                      u8* __restrict__ heads,
                                      u64* __restrict__ n_mismatch) {
    const int g = threadIdx.x & (SV_GROUP - 1);
    const long stride = (long)gridDim.x * SV_ROWS;
    const u8* end = blob + blob_n;
    for (long ib = (long)blockIdx.x * SV_ROWS; ib < n; ib += stride) {
        const long i = ib + threadIdx.x / SV_GROUP;
        // 0: compare bytes, 1: head by hash, 2: head by mismatch
        int verdict = 1;
        long ba = 0, bb = 0, len = 0;
        if (i < n && i > 0 && sorted_hash[i] == sorted_hash[i - 1]) {
            const long ra = perm[i], rb = perm[i - 1];
            verdict = 2;
            if (ra >= 0 && ra < n && rb >= 0 && rb < n) {
                long la, lb;
                sv_row(offs, ra, blob_n, &ba, &la);
                sv_row(offs, rb, blob_n, &bb, &lb);
                if (la == lb) {
                    verdict = 0;
                    len = la;
                }
            }
        }
        const long nw = verdict == 0 ? (len + 7) >> 3 : 0;
        int diff = 0;
        for (long j = g; j < nw; j += SV_GROUP) {
            const long rem = len - 8 * j;
            const int nv = rem < 8 ? (int)rem : 8;
            diff |= sv_load_word(blob + ba + 8 * j, nv, blob, end) !=
                    sv_load_word(blob + bb + 8 * j, nv, blob, end);
        }
        diff |= __shfl_xor(diff, 1);
        diff |= __shfl_xor(diff, 2);
        diff |= __shfl_xor(diff, 4);
        if (g == 0 && i < n) {
            const bool mismatch = verdict == 2 || (verdict == 0 && diff);
            heads[i] = (verdict == 1 || mismatch) ? 1 : 0;
            if (mismatch) atomicAdd(n_mismatch, 1ULL);
        }
    }
}

// Round key of window [7d, 7d + 7) of a row: the window's bytes big-endian
// (zero-padded) in the high 56 bits, and in the low byte c = 8 when the row
// continues past the window, else the number of row bytes inside it (0..7).
// Unsigned key order is the rows' byte order on this window: equal padded
// bytes with a smaller c mean the row ended there, a proper prefix.  One
// lane per row: the window is at most two aligned words.
__global__ void sv_lex_key_kernel(const u8* __restrict__ blob, long blob_n,
                                  const long* __restrict__ offs, long n,
                                  const int* __restrict__ rows, long m,
                                  long d, u64* __restrict__ out) {
    const long stride = (long)gridDim.x * blockDim.x;
    const u8* end = blob + blob_n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += stride) {
        const long r = rows[i];
        u64 key = 0;
        if (r >= 0 && r < n) {
            long b, len;
            sv_row(offs, r, blob_n, &b, &len);
            const long rem = len - 7 * d;
            if (rem > 0) {
                const int nv = rem < 7 ? (int)rem : 7;
                const u64 w = sv_load_word(blob + b + 7 * d, nv, blob, end);
                // byte 0 of the window to bits 63..56; byte 7 of w is 0
                key = __builtin_bswap64(w) | (u64)(rem > 7 ? 8 : nv);
            }
        }
        out[i] = key;
    }
}

// Rows sorted by (grp, key).  A class is a run of equal (grp, key): its
// first row is a head.  A class of two or more rows whose window did not
// reach the row's end (c == 8) is open: the next window decides it.
__global__ void sv_lex_refine_kernel(const u64* __restrict__ grp,
                                     const u64* __restrict__ key, long m,
                                     u8* __restrict__ heads,
                                     u8* __restrict__ open) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += stride) {
        const u64 g = grp[i], k = key[i];
        const bool eq_prev = i > 0 && grp[i - 1] == g && key[i - 1] == k;
        const bool eq_next = i + 1 < m && grp[i + 1] == g && key[i + 1] == k;
        heads[i] = eq_prev ? 0 : 1;
        open[i] = ((k & 255) == 8 && (eq_prev || eq_next)) ? 1 : 0;
    }
}

namespace {
// A byte arena column: blob, and offs of n + 1 entries.
struct Arena {
    const u8* blob;
    const long* offs;
    long blob_n, n;
    Arena(Args& a, const torch::Tensor& b, const torch::Tensor& o) {
        blob = a.dev<const u8>(b, "blob");
        offs = a.dev_min<const long>(o, "offs", 1);
        blob_n = b.numel();
        n = o.numel() - 1;
    }
};
}  // namespace

void sv_hash64(torch::Tensor blob, torch::Tensor offs, uint64_t mask,
               torch::Tensor out) {
    Args a;
    const Arena sv(a, blob, offs);
    u64* o = a.dev<u64>(out, "out", sv.n);
    if (sv.n == 0) return;
    hipLaunchKernelGGL(sv_hash64_kernel,
        dim3(grid_for(sv.n * SV_GROUP, SV_BLOCK, 8192)), dim3(SV_BLOCK), 0,
        a.stream(), sv.blob, sv.blob_n, sv.offs, sv.n, (u64)mask, o);
}

void sv_adjacent_eq(torch::Tensor blob, torch::Tensor offs,
                    torch::Tensor sorted_hash, torch::Tensor perm,
                    torch::Tensor heads, torch::Tensor n_mismatch) {
    Args a;
    const Arena sv(a, blob, offs);
    const u64* sh = a.dev<const u64>(sorted_hash, "sorted_hash", sv.n);
    const int* pm = a.dev<const int>(perm, "perm", sv.n);
    u8* hd = a.dev<u8>(heads, "heads", sv.n);
    u64* nm = a.dev<u64>(n_mismatch, "n_mismatch", 1);
    if (sv.n == 0) return;
    hipLaunchKernelGGL(sv_adjacent_eq_kernel,
        dim3(grid_for(sv.n * SV_GROUP, SV_BLOCK, 8192)), dim3(SV_BLOCK), 0,
        a.stream(), sv.blob, sv.blob_n, sv.offs, sh, pm, sv.n, hd, nm);
}

void sv_lex_key(torch::Tensor blob, torch::Tensor offs, torch::Tensor rows,
                long d, torch::Tensor out) {
    Args a;
    const Arena sv(a, blob, offs);
    const long m = rows.numel();
    const int* r = a.dev<const int>(rows, "rows");
    u64* o = a.dev<u64>(out, "out", m);
    // 7 * d stays far inside i64
    TORCH_CHECK(d >= 0 && d < (1L << 48), "d: window index out of range");
    if (m == 0) return;
    hipLaunchKernelGGL(sv_lex_key_kernel,
        dim3(grid_for(m, SV_BLOCK, 8192)), dim3(SV_BLOCK), 0, a.stream(),
        sv.blob, sv.blob_n, sv.offs, sv.n, r, m, d, o);
}

void sv_lex_refine(torch::Tensor grp_sorted, torch::Tensor key_sorted,
                   torch::Tensor heads, torch::Tensor open) {
    Args a;
    const long m = key_sorted.numel();
    const u64* k = a.dev<const u64>(key_sorted, "key_sorted");
    const u64* g = a.dev<const u64>(grp_sorted, "grp_sorted", m);
    u8* hd = a.dev<u8>(heads, "heads", m);
    u8* op = a.dev<u8>(open, "open", m);
    if (m == 0) return;
    hipLaunchKernelGGL(sv_lex_refine_kernel,
        dim3(grid_for(m, SV_BLOCK, 8192)), dim3(SV_BLOCK), 0, a.stream(),
        g, k, m, hd, op);
}
