// dampr_amd gfx950 TF-IDF kernels: text ingest, tokenize+hash (K1) and
// the per-document dedupe + document-frequency count into device hash
// tables (K6).  The flagship tfidf_docs_kernel finds documents and tokens
// by itself in one pass over the text; the mark scans and
// tfidf_count_kernel are the fully general rerun path behind it.  These
// are the MI355X-native replacements for the reference's per-record Python
// hot loops; the roles, not the code, come from
// dampr/dataset.py + dampr/base.py.  The table ops, the idf epilogue and
// the TSV sink that finish a run are in dampr_tables.hip.
//
// Design notes (cdna_hip_programming.md):
//  - memory-bound kernels: 256-thread blocks, vectorized 16 B/lane loads,
//    grid capped with grid-stride loops (Guideline 11/13).
//  - wave64 ballots (u64 masks) for in-block stable compaction.
//  - all inter-block communication via device-scope atomics on HBM.
#include <hip/hip_runtime.h>
#include "host.h"
#include "ops.h"

#include "common.h"

#define BLOCK 256
#define VBYTES 16                     // bytes per lane per iteration
#define TILE (BLOCK * VBYTES)         // 4 KiB per block-iteration

// Mark modes for the position scan.
#define MODE_NEWLINE 0
#define MODE_TOKEN_START 1

__device__ __forceinline__ bool mark_at(int mode, const u8* text,
                                        long i, long n) {
    u8 c = text[i];
    if (mode == MODE_NEWLINE) return c == '\n';
    // token start: word char whose predecessor is not a word char
    if (!is_word(c)) return false;
    return i == 0 || !is_word(text[i - 1]);
}

// ---------------------------------------------------------------- scan pass 1
// Each block owns a contiguous [base, base + iters*TILE) byte range and
// counts its marks.
// SWAR newline detection: high bit of each byte equal to '\n' (5 VALU
// ops per 4 bytes instead of ~3 per byte) — lines are ~100 bytes, so
// matches are rare and position extraction is off the hot path.
__device__ __forceinline__ u32 nlmask32(u32 w) {
    u32 x = w ^ 0x0A0A0A0Au;
    return (x - 0x01010101u) & ~x & 0x80808080u;
}

__global__ void count_marks_kernel(const u8* __restrict__ text, long n,
                                   int mode, int iters,
                                   u32* __restrict__ counts) {
    long base = (long)blockIdx.x * iters * TILE;
    int tid = threadIdx.x;
    u32 local = 0;
    for (int it = 0; it < iters; ++it) {
        long off = base + (long)it * TILE + (long)tid * VBYTES;
        if (off >= n) break;
        if (off + VBYTES <= n) {
            uint4 v = *reinterpret_cast<const uint4*>(text + off);
            if (mode == MODE_NEWLINE) {
                local += __popc(nlmask32(v.x)) + __popc(nlmask32(v.y))
                       + __popc(nlmask32(v.z)) + __popc(nlmask32(v.w));
            } else {
                const u8* b = reinterpret_cast<const u8*>(&v);
                #pragma unroll
                for (int j = 0; j < VBYTES; ++j) {
                    bool prev_word = (j > 0)
                        ? is_word(b[j - 1])
                        : (off > 0 ? is_word(text[off - 1]) : false);
                    local += is_word(b[j]) && !prev_word;
                }
            }
        } else {
            for (long i = off; i < n; ++i)
                local += mark_at(mode, text, i, n);
        }
    }
    // block reduction: wave reduce then LDS
    __shared__ u32 wsum[BLOCK / WAVE];
    for (int d = WAVE / 2; d > 0; d >>= 1)
        local += __shfl_down(local, d, WAVE);
    int lane = tid & (WAVE - 1), wid = tid / WAVE;
    if (lane == 0) wsum[wid] = local;
    __syncthreads();
    if (tid == 0) {
        u32 total = 0;
        for (int w = 0; w < BLOCK / WAVE; ++w) total += wsum[w];
        counts[blockIdx.x] = total;
    }
}

// ---------------------------------------------------------------- scan pass 2
// Re-scan and write mark positions in ascending order.  Two-phase within
// the block: per-(wave, tile) counts into LDS, ONE barrier, then a
// sync-free scatter pass where every wave derives its own bases from the
// count matrix (the old per-tile cursor + double barrier serialized the
// block on memory latency every 4 KiB).
#define SCAN_MAX_ITERS 16

__device__ __forceinline__ u32 gather_marks(const u8* __restrict__ text,
                                            long n, int mode, long off,
                                            u8* rel) {
    u32 cnt = 0;
    if (off >= n) return 0;
    if (off + VBYTES <= n) {
        uint4 v = *reinterpret_cast<const uint4*>(text + off);
        if (mode == MODE_NEWLINE) {
            const u32 words[4] = {v.x, v.y, v.z, v.w};
            #pragma unroll
            for (int wi = 0; wi < 4; ++wi) {
                u32 m = nlmask32(words[wi]);
                while (m) {
                    int bit = __ffs(m) - 1;
                    rel[cnt++] = (u8)(wi * 4 + (bit >> 3));
                    m &= m - 1;
                }
            }
            return cnt;
        }
        const u8* b = reinterpret_cast<const u8*>(&v);
        #pragma unroll
        for (int j = 0; j < VBYTES; ++j) {
            u8 c = b[j];
            bool prev_word = (j > 0)
                ? is_word(b[j - 1])
                : (off > 0 ? is_word(text[off - 1]) : false);
            bool m = is_word(c) && !prev_word;
            if (m) rel[cnt++] = (u8)j;
        }
    } else {
        long lim = n - off;
        for (long j = 0; j < lim; ++j)
            if (mark_at(mode, text, off + j, n)) rel[cnt++] = (u8)j;
    }
    return cnt;
}

__global__ void write_marks_kernel(const u8* __restrict__ text, long n,
                                   int mode, int iters,
                                   const u32* __restrict__ block_offsets,
                                   u32* __restrict__ out) {
    long base = (long)blockIdx.x * iters * TILE;
    int tid = threadIdx.x;
    int lane = tid & (WAVE - 1), wid = tid / WAVE;
    __shared__ u32 wtile[BLOCK / WAVE][SCAN_MAX_ITERS];

    // phase 1: per-(wave, tile) mark counts
    for (int it = 0; it < iters; ++it) {
        long off = base + (long)it * TILE + (long)tid * VBYTES;
        u8 rel[VBYTES];
        u32 cnt = gather_marks(text, n, mode, off, rel);
        u32 tot = cnt;
        for (int d = WAVE / 2; d > 0; d >>= 1)
            tot += __shfl_down(tot, d, WAVE);
        if (lane == 0) wtile[wid][it] = tot;
    }
    __syncthreads();

    // phase 2: rescan (L2-hot) and scatter; bases derived per wave
    u32 run = block_offsets[blockIdx.x];
    for (int it = 0; it < iters; ++it) {
        u32 wb = run;
        u32 tile_tot = 0;
        for (int w = 0; w < BLOCK / WAVE; ++w) {
            if (w < wid) wb += wtile[w][it];
            tile_tot += wtile[w][it];
        }
        long off = base + (long)it * TILE + (long)tid * VBYTES;
        u8 rel[VBYTES];
        u32 cnt = gather_marks(text, n, mode, off, rel);
        u32 scan = cnt;
        for (int d = 1; d < WAVE; d <<= 1) {
            u32 x = __shfl_up(scan, d, WAVE);
            if (lane >= d) scan += x;
        }
        u32 excl = wb + scan - cnt;
        for (u32 j = 0; j < cnt; ++j)
            out[excl + j] = (u32)(off + rel[j]);
        run += tile_tot;
    }
}

// ------------------------------------------------------------ tokenize+count
// One thread per token: hash the token (K1), locate its document (binary
// search over newline positions), dedupe (doc, token) in the seen table
// and bump the document-frequency table (K6).  First global occurrence of
// a token also records (byte offset, length) in the string dictionary so
// results can be materialized as text.
__global__ void tfidf_count_kernel(
        const u8* __restrict__ text, long n,
        const u32* __restrict__ nl_pos, long n_nl,
        const u32* __restrict__ tok_start, long n_tok,
        u64* __restrict__ seen_keys, u64 seen_mask,
        u64* __restrict__ cnt_keys, u64* __restrict__ cnt_vals,
        u64 cnt_mask,
        u64* __restrict__ dict_keys, u64* __restrict__ dict_vals,
        u64 dict_mask, u64 pos_base, u64 doc_base) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n_tok;
         t += stride) {
        u32 start = tok_start[t];
        long p = start;
        u64 h = 0;
        u32 j = 0;
        while (p < n) {
            u8 c = text[p];
            if (!is_word(c)) break;
            h = tokmix_step(h, j, lower_ascii(c));
            ++p;
            ++j;
        }
        u32 len = (u32)(p - start);
        h = tokmix_final(h, len);
        // doc id = number of newlines strictly before `start`
        long lo = 0, hi = n_nl;
        while (lo < hi) {
            long mid = (lo + hi) >> 1;
            if (nl_pos[mid] < start) lo = mid + 1; else hi = mid;
        }
        u64 doc = (u64)lo + doc_base;
        u64 tok_key = h ? h : 1ULL;
        u64 sk = splitmix64(h ^ (doc * 0x9E3779B97F4A7C15ULL));
        if (!sk) sk = 1;
        u64 slot;
        if (table_insert_u64(seen_keys, seen_mask, sk, &slot)) {
            table_add_u64(cnt_keys, cnt_vals, cnt_mask, tok_key, 1ULL);
            if (table_insert_u64(dict_keys, dict_mask, tok_key, &slot))
                dict_vals[slot] = ((pos_base + (u64)start) << 8)
                                  | (u64)min(len, 255u);
        }
    }
}

// ------------------------------------------------------- doc-centric count
// Fast path: a wave owns a fixed byte span of the chunk and finds the
// documents that start in it by itself.  The text is staged into LDS with
// coalesced loads, newlines and token starts are found in-register, and
// the per-doc `set()` dedupe is a tiny per-wave LDS hash set — no newline
// position buffer, no global seen table, no per-token binary search, one
// pass over the text.  Documents whose
// distinct-token count overflows the LDS set fall back to a global
// (doc,hash)-keyed seen table; if THAT overflows its probe bound the
// kernel sets an error flag and the host reruns the chunk on the fully
// general token-centric kernel above.
#ifndef DOC_WAVES
#define DOC_WAVES 4                  // waves per block
#endif
#ifndef STAGE_B
#define STAGE_B 2048                 // staged line segment bytes
#endif
#define SEG_OVERLAP 272              // > max dict token length (255)
#ifndef DOC_SET
#define DOC_SET 256                  // per-wave dedupe set slots (pow2)
#endif
#ifndef FB_PROBE_CAP
#define FB_PROBE_CAP 512
#endif
#ifndef DOC_SPAN
#define DOC_SPAN 8192                // text bytes owned by a wave per visit
#endif
#ifndef GROUP_BYTES
#define GROUP_BYTES 1024             // target bytes per doc group
#endif
#ifndef CCACHE
#define CCACHE 1024                  // block-level LDS count cache slots
#endif
#ifndef DOC_BPL
#define DOC_BPL 8                    // text bytes per lane per window
#endif
#define DOC_LENMIX_N 128             // token lengths served by the table
#define DOC_SALT_K 0x9E3779B97F4A7C15ULL   // odd; low byte 0x15
#define DOC_WIN (WAVE * DOC_BPL)     // bytes per wave window
static_assert(DOC_BPL == 4 || DOC_BPL == 8, "lane word is b32 or b64");
// Stage edges must fall on lane boundaries: a token live at the edge is
// carried out as the edge lane's tail run.
static_assert(STAGE_B % 16 == 0, "stage edge on a lane boundary");
static_assert(DOC_SPAN % 16 == 0 && DOC_SPAN >= 16, "span on a 16 B edge");
// One 16 B LDS read per lane covers a group's boundary search.
static_assert(GROUP_BYTES == WAVE * 16 && GROUP_BYTES <= STAGE_B,
              "group search is one uint4 per lane of staged text");
#define GROUP_OPEN (1L << 62)        // group end not found yet

// SWAR byte classification, 4 text bytes per call; result bit j = byte j.
// swar_ge: high bit of each byte set iff the byte's low 7 bits >= k
// (sum <= 0xFE, so no carry crosses bytes); exact for every byte value,
// bytes >= 0x80 are never word characters (matches is_word).
__device__ __forceinline__ u32 swar_ge(u32 x7, u32 k) {
    return x7 + (0x80u - k) * 0x01010101u;
}
__device__ __forceinline__ u32 swar_pack4(u32 m) {
    // flags at bits 7/15/23/31 -> bits 0..3 (no colliding partial products)
    return (((m & 0x80808080u) >> 7) * 0x01020408u) >> 24;
}
__device__ __forceinline__ u32 wordbits4(u32 x) {
    const u32 x7 = x & 0x7F7F7F7Fu;
    const u32 y7 = x7 | 0x20202020u;           // fold A-Z onto a-z
    const u32 m = (swar_ge(y7, 'a') ^ swar_ge(y7, 'z' + 1))
                | (swar_ge(x7, '0') ^ swar_ge(x7, '9' + 1))
                | (swar_ge(x7, '_') ^ swar_ge(x7, '_' + 1));
    return swar_pack4(m & ~x);
}
__device__ __forceinline__ u32 nlbits4(u32 x) {
    const u32 v = x ^ 0x0A0A0A0Au;             // exact zero-byte test
    return swar_pack4(~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v));
}
// Newline bits of 16 staged bytes at p (16 B aligned), bit j = byte j,
// kept for byte positions [from, to) when p holds position `at`.
__device__ __forceinline__ u32 nlbits16(const u8* p, long at, long from,
                                        long to) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    const u32 m = nlbits4(v.x) | (nlbits4(v.y) << 4) | (nlbits4(v.z) << 8)
                | (nlbits4(v.w) << 12);
    const int lo = (int)min(max(from - at, 0L), 16L);
    const int hi = (int)min(max(to - at, 0L), 16L);
    return m & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}
// Mask of the nlbits16 bits at byte positions >= pos for 16 B held at `at`.
__device__ __forceinline__ u32 nlbits_from(long at, long pos) {
    const int k = (int)min(max(pos - at, 0L), 16L);
    return ~((1u << k) - 1u);
}
__device__ __forceinline__ u64 low_bytes_mask(int k) {
    return k >= 8 ? ~0ULL : ((1ULL << (8 * k)) - 1ULL);
}

// Two-level counting: Zipf-hot keys would serialize ~50M same-address L2
// atomics; the block-level LDS cache turns that into one global add per
// (block, hot key).  Cache misses (cold keys) go straight to the global
// table — cold keys have no contention.
#define CC_PROBES 4                  // probe bound of the block cache
#define CC_HIT 0                     // key was cached already
#define CC_NEW 1                     // this lane's CAS cached the key
#define CC_MISS 2                    // no room within the bound: global add
#define EMIT_CNT 1u                  // emit needs a global count add
#define EMIT_DICT 2u                 // emit needs a string-dict insert

// One sequential probe step at `slot`: CC_HIT / CC_NEW when the count
// went into the cache, -1 to move on to the next slot.
__device__ __forceinline__ int block_cache_step(
        u64* __restrict__ cck, u32* __restrict__ ccv, u32 slot, u64 key,
        u64 cur) {
    if (cur == key) { atomicAdd(&ccv[slot], 1u); return CC_HIT; }
    if (cur == 0ULL) {
        const u64 prev = atomicCAS(&cck[slot], 0ULL, key);
        if (prev == 0ULL || prev == key) {
            atomicAdd(&ccv[slot], 1u);
            return prev == 0ULL ? CC_NEW : CC_HIT;
        }
    }
    return -1;
}

// Count `key` in the block cache.  The CC_PROBES slots of its probe run
// (wrapping at CCACHE) are read back to back before one wait; hit, empty
// (CAS) or miss is then decided from registers.  A slot read as another
// key stays that key (keys are never removed) and a slot read as empty is
// revalidated by the CAS, so early reads decide exactly what a probe by
// probe walk decides; only a lost CAS goes on probe by probe, over the
// rest of the bound.
__device__ __forceinline__ int block_cache_add(
        u64* __restrict__ cck, u32* __restrict__ ccv, u64 key) {
    const u32 s0 = (u32)(key & (CCACHE - 1));
    u64 c[CC_PROBES];
    #pragma unroll
    for (int p = 0; p < CC_PROBES; ++p)
        c[p] = cck[(s0 + p) & (CCACHE - 1)];
    #pragma unroll
    for (int p = 0; p < CC_PROBES; ++p)
        asm volatile("" : "+v"(c[p]));
    // first slot of the run that holds the key or is empty
    int f = CC_PROBES;
    u64 cf = 0;
    #pragma unroll
    for (int p = CC_PROBES - 1; p >= 0; --p)
        if (c[p] == key || c[p] == 0ULL) { f = p; cf = c[p]; }
    if (f == CC_PROBES) return CC_MISS;
    u32 slot = (s0 + f) & (CCACHE - 1);
    int r = block_cache_step(cck, ccv, slot, key, cf);
    if (r >= 0) return r;
    for (int p = f + 1; p < CC_PROBES; ++p) {  // lost the CAS
        slot = (slot + 1) & (CCACHE - 1);
        r = block_cache_step(cck, ccv, slot, key, cck[slot]);
        if (r >= 0) return r;
    }
    return CC_MISS;
}

__device__ __forceinline__ int lds_set_insert(u64* set, u64 h) {
    // 1 = fresh, 0 = dup, -1 = set full (h definitely absent: full scan)
    u32 slot = (u32)(h & (DOC_SET - 1));
    for (int probe = 0; probe < DOC_SET; ++probe) {
        u64 prev = atomicCAS(&set[slot], 0ULL, h);
        if (prev == 0ULL) return 1;
        if (prev == h) return 0;
        slot = (slot + 1) & (DOC_SET - 1);
    }
    return -1;
}

__global__ void __launch_bounds__(DOC_WAVES * WAVE, 5)
tfidf_docs_kernel(const u8* __restrict__ text, long n,
                  u64* __restrict__ cnt_keys, u64* __restrict__ cnt_vals,
                  u64 cnt_mask,
                  u64* __restrict__ dict_keys, u64* __restrict__ dict_vals,
                  u64 dict_mask, u64 pos_base,
                  u64* __restrict__ fb_seen, u64 fb_mask,
                  u32* __restrict__ err_flag, u32 ablate) {
    // v5: span ownership, group-of-docs stream processing, DOC_BPL text
    // bytes per lane.  err_flag[0] = overflow flag, [1] = ablation sink,
    // [2] = documents counted (one atomic per block).
    //  * a wave owns the byte span [a, a + DOC_SPAN) and processes exactly
    //    the docs that START in it: it skips to the first newline at a
    //    position >= a-1 (nothing when a == 0) and runs through the first
    //    newline at a position >= b-1 (or to n), however far past b that
    //    is.  Every doc has one owner and no wave waits on another.
    //  * docs are processed in *groups* (<= GROUP_BYTES of consecutive
    //    docs): windows run continuously across doc boundaries, so short
    //    docs no longer waste partial windows or per-doc framing
    //  * a group's end is found in the staged text itself: one 16 B LDS
    //    read per lane, SWAR newline bits, a ballot and a clz give the last
    //    newline within GROUP_BYTES of the group start (or the span's
    //    closing newline).  A doc with no newline there forms its own
    //    group and streams stages until the one holding its newline.
    //  * doc identity inside a window comes from the newline ballot;
    //    dedupe keys are salted with the doc id (group start byte + ordinal
    //    in the group: unique per chunk, a group of k docs spans >= k
    //    bytes), so the per-wave LDS set only needs clearing once per
    //    group (always at a doc boundary)
    //  * a lane reads one aligned DOC_BPL-byte word per window, classifies
    //    it with SWAR masks and hashes its bytes serially in registers
    //    (tokmix prefix XORs, positions counted from the lane start)
    //  * tokmix partials join as A.g ^ rotl(P.g, A.len), len = A.len +
    //    P.len (rotation distributes over XOR), so tokens crossing lanes
    //    are stitched by a segmented scan over lane tail summaries whose
    //    depth adapts to the longest unresolved chain; tokens crossing
    //    window/stage edges ride a wave-uniform carry
    //  * each lane owns the token ends inside its word; the emit loop has
    //    a wave-uniform trip count (max ends per lane)
    __shared__ __align__(16) u8 stage[DOC_WAVES][STAGE_B + 16];
    __shared__ u64 dset[DOC_WAVES][DOC_SET];
    __shared__ u64 cck[CCACHE];
    __shared__ u32 ccv[CCACHE];
    __shared__ u64 toktab[256];
    __shared__ u64 lenmix[DOC_LENMIX_N];
    __shared__ u32 blk_docs;
    // five blocks per CU (launch bounds) share 160 KB of LDS
    static_assert(sizeof(stage) + sizeof(dset) + sizeof(cck) + sizeof(ccv)
                  + sizeof(toktab) + sizeof(lenmix) + 8 <= 32768,
                  "block LDS allows 5 blocks per CU");
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x % WAVE;
    const long gwave = (long)blockIdx.x * DOC_WAVES + wid;
    const long nwaves = (long)gridDim.x * DOC_WAVES;
    const long nspans = (n + DOC_SPAN - 1) / DOC_SPAN;
    u8* st = stage[wid];
    u64* set = dset[wid];
    u32 my_docs = 0;                           // wave-uniform

    for (int i = threadIdx.x; i < CCACHE; i += blockDim.x) {
        cck[i] = 0;
        ccv[i] = 0;
    }
    // indexed by the RAW byte: the lowercase fold is baked into the table.
    // The walk reads the table for every byte, word byte or not: a
    // non-word byte's entry is 0, so it (and a masked byte, which reads
    // entry 0) drops out of the XOR without a select.
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
        toktab[i] = is_word((u8)i) ? toktab_entry(lower_ascii((u8)i)) : 0ULL;
    // the length finaliser's splitmix64(len), from the same function
    for (int i = threadIdx.x; i < DOC_LENMIX_N; i += blockDim.x)
        lenmix[i] = splitmix64((u64)i);
    if (threadIdx.x == 0) blk_docs = 0;
    __syncthreads();

    // Emit phases.  A fresh token that needs the global tables (EMIT_CNT:
    // its count missed the block cache; EMIT_DICT: its string may be new)
    // first issues the cnt_keys and dict_keys loads of its home slots
    // back to back and waits once, then finishes here: a loaded word
    // equal to the key is a count add / a dict no-op; anything else
    // (empty or another key) runs the ordinary probe loop, whose CAS
    // revalidates.  The dict goes first and the no-return count add last,
    // so no load of an emit waits behind one of its atomics; the add is
    // next waited for in the following emit, a window later.
    auto finish_emit = [&](u64 key, u64 pk, u64 cw, u64 dw, u32 fl) {
        if ((fl & EMIT_DICT) && dw != key) {
            u64 slot;
            if (table_insert_u64(dict_keys, dict_mask, key, &slot))
                dict_vals[slot] = pk;
        }
        if (fl & EMIT_CNT) {
            if (cw == key) atomicAdd(&cnt_vals[key & cnt_mask], 1ULL);
            else table_add_u64(cnt_keys, cnt_vals, cnt_mask, key, 1ULL);
        }
    };

    for (long sp = gwave; sp < nspans; sp += nwaves) {
        const long a = sp * DOC_SPAN;          // a < n
        const long b = a + DOC_SPAN;
        long win_lo = -1, win_hi = -1, aseg = 0;

        // (Re)stage an aligned window from seg < n: bytes [seg, win_hi)
        // become valid in LDS at st + (pos - aseg).  Bytes past a group
        // belong to following docs and are reused.  Full interior
        // windows use the async global->LDS copy (zero staging VGPRs, no
        // reg->ds_write pass; LDS dest = wave-uniform base + lane*16 =
        // exactly this linear layout).  A double-buffered prefetch
        // variant measured WORSE (999M vs 1130M rows/s): the extra 8 KB
        // LDS costs an occupancy step, which outweighs hiding the
        // staging stall.  Corpus tail keeps the byte path.
        auto stage_at = [&](long seg) {
            aseg = seg & ~15L;
            const int stage_bytes =
                (int)min((long)(STAGE_B + 16), n - aseg);
            if (aseg + STAGE_B + 16 <= n) {
                #pragma unroll
                for (int i = 0; i < STAGE_B; i += WAVE * 16)
                    __builtin_amdgcn_global_load_lds(
                        (const u32*)(text + aseg + i + lane * 16),
                        (u32*)(st + i), 16, 0, 0);
                if (lane == 0)
                    __builtin_amdgcn_global_load_lds(
                        (const u32*)(text + aseg + STAGE_B),
                        (u32*)(st + STAGE_B), 16, 0, 0);
            } else {
                for (int i = lane * 16; i < stage_bytes; i += WAVE * 16) {
                    if (aseg + i + 16 <= n) {
                        *reinterpret_cast<uint4*>(st + i) =
                            *reinterpret_cast<const uint4*>(
                                text + aseg + i);
                    } else {
                        for (int j = i; j < stage_bytes; ++j)
                            st[j] = (aseg + j < n)
                                ? text[aseg + j] : (u8)0;
                    }
                }
            }
            // vmcnt(0) lgkmcnt(0) (expcnt field 7 = no wait), as a
            // builtin the compiler's wait counting sees: with the wait
            // hidden in an asm string it takes the global->LDS copies
            // for still in flight and puts its own vmcnt(0) in front of
            // every window's text read, which drains the no-return
            // count adds of the window before.
            __builtin_amdgcn_s_waitcnt(0x0070);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            win_lo = seg;
            win_hi = aseg + stage_bytes;
        };
        // Lane's newline bits for its 16 B of the 1 KiB of staged text
        // at `base` (16 B aligned, >= aseg), kept for [from, to) with
        // to <= win_hi.
        auto nl_lane16 = [&](long base, long from, long to) -> u32 {
            const long at = base + lane * 16;
            return at < to
                ? nlbits16(st + (int)(at - aseg), at, from, to) : 0u;
        };
        // First newline in the staged bytes [from, to), or -1.
        auto first_nl = [&](long from, long to) -> long {
            for (long base = from & ~15L; base < to; base += WAVE * 16) {
                const u32 m = nl_lane16(base, from, to);
                const u64 any = __ballot(m != 0);
                if (any) {
                    const int fl = __ffsll((unsigned long long)any) - 1;
                    const u32 mf = __builtin_amdgcn_readlane(m, fl);
                    return base + fl * 16 + (__ffs(mf) - 1);
                }
            }
            return -1;
        };

        // first doc start in the span: byte 0, or one past the first
        // newline in [a-1, b-2]; none there = this wave owns nothing
        long gs = 0;
        if (a > 0) {
            const long lim = min(b - 1, n);
            long p = -1;
            for (long pos = a - 1; pos < lim; ) {
                if (pos < win_lo || pos >= win_hi) stage_at(pos);
                const long to = min(win_hi, lim);
                p = first_nl(pos, to);
                if (p >= 0) break;
                pos = to;
            }
            if (p < 0) continue;
            gs = p + 1;
        }

        while (gs < n) {
            // group = the docs in [gs, gend]: gend is the last newline
            // within GROUP_BYTES of the (16 B aligned) group start, or
            // the first newline at a position >= b-1 (the span's last
            // doc), or n for an unterminated tail.  Only staged bytes are
            // searched: a newline in the staged part closes a shorter
            // group; with none there the window is restaged at gs.
            if (gs < win_lo || gs >= win_hi) stage_at(gs);
            const long gbase = gs & ~15L;
            long gend = GROUP_OPEN;            // open = oversized doc
            for (int attempt = 0; attempt < 2; ++attempt) {
                const long to = min(gbase + (long)GROUP_BYTES, win_hi);
                const u32 m = nl_lane16(gbase, gs, to);
                const u32 mh = m & nlbits_from(gbase + lane * 16, b - 1);
                const u64 any = __ballot(m != 0);
                const u64 anyh = __ballot(mh != 0);
                if (anyh) {                    // closes the span
                    const int fl = __ffsll((unsigned long long)anyh) - 1;
                    const u32 mf = __builtin_amdgcn_readlane(mh, fl);
                    gend = gbase + fl * 16 + (__ffs(mf) - 1);
                    break;
                }
                long last = -1;
                if (any) {
                    const int ll = 63 - __clzll((long long)any);
                    const u32 ml = __builtin_amdgcn_readlane(m, ll);
                    last = gbase + ll * 16 + (31 - __clz((int)ml));
                }
                if (to == n) {                 // text ends in the range
                    gend = (last == n - 1) ? last : n;
                    break;
                }
                if (last >= 0) { gend = last; break; }
                if (to == gbase + (long)GROUP_BYTES) break;
                stage_at(gs);
            }

            for (int s = lane; s < DOC_SET; s += WAVE) set[s] = 0;
            u32 carry_word = 0;                // wave-uniform token carry
            u32 carry_len = 0;
            u64 carry_g = 0;
            long carry_start = gs;
            u32 carry_lines = 0;               // newlines seen in group

            // dedupe + count + dict insert for one finished token
            // (token start = wave-uniform tbase + trel, doc = gs + drel)
            auto emit_token = [&](u64 gh, u32 tl, long tbase, int trel,
                                  u32 drel) {
                if (ablate & 1) {              // ablation: consume hash
                    if (gh == 0xdeadbeefdeadbeefULL) err_flag[1] = 1;
                    return;
                }
                u64 lm;
                if (tl < DOC_LENMIX_N) lm = lenmix[tl];
                else lm = splitmix64((u64)tl);
                const u64 hh = gh ^ lm;        // == tokmix_final(gh, tl)
                const u64 key = hh ? hh : 1ULL;
                const long doc_id = gs + (long)drel;
                // Dedupe salt = doc_id * K mod 2^64, K odd (hoisting
                // gs * K by hand compiles to the same multiply).  It
                // never reaches an output; it must only keep (hash, doc)
                // pairs apart and spread them over the set:
                //  * x -> x * K is a bijection of the 64-bit integers
                //    (K is odd), so two doc ids of a chunk never share a
                //    salt, and dk = hh ^ salt is equal for two pairs only
                //    when the pairs are equal or hh1 ^ hh2 hits one fixed
                //    non-zero 64-bit value: the 2^-64 chance of before.
                //  * the low 8 bits of the salt are (doc_id * 0x15) mod
                //    256, a bijection of doc_id mod 256 (0x15 is odd):
                //    any two ids less than 256 apart, consecutive ones
                //    included, put the same token into different start
                //    slots of the 256-slot set.
                u64 dk = hh ^ ((u64)doc_id * DOC_SALT_K);
                if (!dk) dk = 1;
                int fresh = lds_set_insert(set, dk);
                if (fresh < 0) {
                    // set overflow: global (doc,hash) seen fallback
                    u64 sk = splitmix64(hh ^ ((u64)doc_id
                                              * 0x9E3779B97F4A7C15ULL));
                    if (!sk) sk = 1;
                    u64 slot = sk & fb_mask;
                    fresh = 0;
                    int probe = 0;
                    while (true) {
                        u64 prev = atomicCAS(&fb_seen[slot], 0ULL, sk);
                        if (prev == 0ULL) { fresh = 1; break; }
                        if (prev == sk) break;
                        slot = (slot + 1) & fb_mask;
                        if (++probe > FB_PROBE_CAP) {
                            atomicOr(err_flag, 1u);
                            break;
                        }
                    }
                }
                u32 fl = 0;
                if (fresh == 1 && !(ablate & 2)) {
                    const int cc = block_cache_add(cck, ccv, key);
                    if (cc == CC_MISS) fl |= EMIT_CNT;
                    // a key found in the block cache went to the dict
                    // with the lane whose CAS cached it
                    if (!(ablate & 4) && cc != CC_HIT) fl |= EMIT_DICT;
                }
                const u64 pk = ((pos_base + (u64)(tbase + trel)) << 8)
                             | (u64)min(tl, 255u);
                u64 cw = 0, dw = 0;
                if (fl & EMIT_CNT) cw = cnt_keys[key & cnt_mask];
                if (fl & EMIT_DICT) dw = dict_keys[key & dict_mask];
                if (fl) finish_emit(key, pk, cw, dw, fl);
            };

            for (long seg = gs; seg < gend; ) {
                if (seg < win_lo || seg >= win_hi) stage_at(seg);
                if (gend == GROUP_OPEN) {
                    // oversized doc: its newline is in this stage, or the
                    // text ends here, or the doc streams on
                    const long p = first_nl(seg, win_hi);
                    if (p >= 0) gend = p;
                    else if (win_hi == n) gend = n;
                }
                const long seg_end = min(gend, win_hi);
                const int soff = (int)(seg - aseg);
                const int soff_end = (int)(seg_end - aseg);
                const bool group_continues = seg_end < gend;
                // windows start at a DOC_BPL-aligned stage offset so every
                // lane issues one aligned LDS read
                for (int wb = soff & ~(DOC_BPL - 1); wb < soff_end;
                     wb += DOC_WIN) {
                    const int o = wb + lane * DOC_BPL;
                    // bytes outside [seg, seg_end) become 0: neither a
                    // word character nor a newline
                    const int keep_lo = min(max(soff - o, 0), DOC_BPL);
                    const int keep_hi = min(max(soff_end - o, 0), DOC_BPL);
                    u64 raw = 0;
                    if (keep_hi > 0) {
#if DOC_BPL == 8
                        raw = *reinterpret_cast<const u64*>(st + o);
#else
                        raw = *reinterpret_cast<const u32*>(st + o);
#endif
                    }
                    raw &= low_bytes_mask(keep_hi) & ~low_bytes_mask(keep_lo);
                    u32 W = wordbits4((u32)raw);       // bit j: byte j is \w
                    u32 NLb = nlbits4((u32)raw);       // bit j: byte j is \n
#if DOC_BPL == 8
                    W |= wordbits4((u32)(raw >> 32)) << 4;
                    NLb |= nlbits4((u32)(raw >> 32)) << 4;
#endif
                    // lane-local prefix hashes: P[j] = XOR over word bytes
                    // i <= j of rotl(TAB[b_i], i); pz = P at the last
                    // non-word byte.  A run [s, j] hashes to
                    // rotr(P[j] ^ P[s-1], s).
                    u64 P[DOC_BPL];
                    u64 acc = 0, pz = 0;
                    // all table reads first, unconditional and back to
                    // back, then one wait: left to itself the compiler
                    // sinks each read under its byte's word test and the
                    // window pays DOC_BPL dependent LDS round trips.
                    // Non-word entries are 0, so acc needs no select.
                    u64 T[DOC_BPL];
                    #pragma unroll
                    for (int j = 0; j < DOC_BPL; ++j)
                        T[j] = toktab[(u32)(raw >> (8 * j)) & 0xFFu];
                    #pragma unroll
                    for (int j = 0; j < DOC_BPL; ++j)
                        asm volatile("" : "+v"(T[j]));
                    #pragma unroll
                    for (int j = 0; j < DOC_BPL; ++j) {
                        acc ^= rotl64(T[j], (u32)j);
                        pz = ((W >> j) & 1u) ? pz : acc;
                        P[j] = acc;
                    }
                    const bool first_w = W & 1u;
                    const bool last_w = (W >> (DOC_BPL - 1)) & 1u;
                    const u64 fw = __ballot(first_w);
                    const u64 lw = __ballot(last_w);
                    if (carry_word && !(fw & 1ULL)) {
                        // carried token ended exactly at the window edge
                        if (lane == 0)
                            emit_token(carry_g, carry_len, carry_start,
                                       0, carry_lines);
                        carry_word = 0;
                        carry_len = 0;
                        carry_g = 0;
                    }
                    // edge lane: holds the last valid byte of this window.
                    // A token live at its last byte rides the carry when
                    // the window is full or the group goes on past the
                    // stage edge; otherwise the masked bytes end it.
                    const int span = soff_end - wb;
                    const int e = span >= DOC_WIN ? WAVE - 1
                                                  : (span - 1) / DOC_BPL;
                    const bool hold = (e == WAVE - 1) || group_continues;
                    u64 nf = fw;               // next lane starts with \w
                    if (hold && e < WAVE - 1) nf |= 1ULL << (e + 1);
                    const bool next_first = (lane == WAVE - 1)
                        ? true : (bool)((nf >> (lane + 1)) & 1ULL);
                    const bool cont_in = first_w
                        && (lane == 0 ? carry_word != 0
                                      : (bool)((lw >> (lane - 1)) & 1ULL));
                    // token ends owned by this lane
                    u32 E = W & ~((W >> 1)
                                  | ((u32)next_first << (DOC_BPL - 1)));

                    // tail summary (g, len): the run reaching the lane's
                    // last byte, positions from its lane-local start.
                    // closed = the run starts in this lane (or no run).
                    const u32 zb = ~W & ((1u << DOC_BPL) - 1u);
                    const int ts = zb ? 32 - __clz(zb) : 0;
                    u64 tg = 0;
                    u32 tlen = 0;
                    bool closed = true;
                    if (last_w) {
                        tg = rotl64(acc ^ pz, (u32)(64 - ts));
                        tlen = (u32)(DOC_BPL - ts);
                        closed = !(ts == 0 && cont_in);
                    }
                    // segmented inclusive scan with the tokmix join; runs
                    // only while some all-word lane's chain is unresolved
                    for (int d = 1; d < WAVE; d <<= 1) {
                        if (!__ballot(!closed && lane >= d)) break;
                        const u64 ag = __shfl_up(tg, d, WAVE);
                        const u32 al = __shfl_up(tlen, d, WAVE);
                        const int ac = __shfl_up((int)closed, d, WAVE);
                        if (!closed && lane >= d) {
                            tg = ag ^ rotl64(tg, al);
                            tlen += al;
                            closed = ac;
                        }
                    }
                    if (!closed) {             // chain reaches the carry
                        tg = carry_g ^ rotl64(tg, carry_len);
                        tlen += carry_len;
                    }
                    // prefix of a token continuing into this lane
                    u64 pg = __shfl_up(tg, 1, WAVE);
                    u32 plen = __shfl_up(tlen, 1, WAVE);
                    if (lane == 0) { pg = carry_g; plen = carry_len; }

                    // exclusive prefix count of newlines before this lane;
                    // one ballot per newline a single lane can hold
                    const u32 nlc = __popc(NLb);
                    u32 nl_before = carry_lines;
                    for (u32 k = 1; ; ++k) {
                        const u64 b = __ballot(nlc >= k);
                        if (!b) break;
                        nl_before = __builtin_amdgcn_mbcnt_hi(
                            (u32)(b >> 32),
                            __builtin_amdgcn_mbcnt_lo((u32)b, nl_before));
                        carry_lines += (u32)__popcll(b);
                    }

                    // wave-uniform carry update from the edge lane
                    if (((lw >> e) & 1ULL) && hold) {
                        carry_word = 1;
                        carry_g = __shfl(tg, e, WAVE);
                        carry_len = (u32)__shfl((int)tlen, e, WAVE);
                        carry_start = aseg + wb + (long)(e + 1) * DOC_BPL
                                      - (long)carry_len;
                    } else {
                        carry_word = 0;
                        carry_len = 0;
                        carry_g = 0;
                    }

                    // emit: wave-uniform trip count = max ends per lane
                    u64 pprev = 0;             // P at the previous end
                    while (__ballot(E != 0)) {
                        if (E) {
                            const int j = __ffs(E) - 1;
                            E &= E - 1;
                            u64 pj = P[0];
                            #pragma unroll
                            for (int i = 1; i < DOC_BPL; ++i)
                                pj = (j == i) ? P[i] : pj;
                            const u32 zj = zb & ((1u << j) - 1u);
                            const int s = zj ? 32 - __clz(zj) : 0;
                            u64 g = rotl64(pj ^ pprev, (u32)(64 - s));
                            pprev = pj;
                            u32 len = (u32)(j - s + 1);
                            if (s == 0 && cont_in) {
                                g = pg ^ rotl64(g, plen);
                                len += plen;
                            }
                            emit_token(g, len, aseg,
                                       o + j + 1 - (int)len,
                                       nl_before
                                       + __popc(NLb & ((1u << j) - 1u)));
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
                seg = seg_end;
            }
            if (carry_word) {
                // group ended at a window edge with a live token
                if (lane == 0)
                    emit_token(carry_g, carry_len, carry_start, 0,
                               carry_lines);
            }
            // newlines inside the group, plus the doc that gend closes
            my_docs += carry_lines + 1;
            if (gend >= b - 1) break;          // the span's last doc
            gs = gend + 1;                     // past the newline
        }
    }
    if (lane == 0 && my_docs) atomicAdd(&blk_docs, my_docs);

    // flush the block's count cache and document count
    __syncthreads();
    if (threadIdx.x == 0 && blk_docs) atomicAdd(&err_flag[2], blk_docs);
    for (int i = threadIdx.x; i < CCACHE; i += blockDim.x)
        if (cck[i])
            table_add_u64(cnt_keys, cnt_vals, cnt_mask, cck[i],
                          (u64)ccv[i]);
}

// ==========================================================================
// Host wrappers
// ==========================================================================

namespace {
constexpr int SCAN_ITERS = 8;                     // 32 KiB per block
constexpr long SCAN_SPAN = (long)SCAN_ITERS * TILE;

// The count table and the string dict that both count kernels fill.
struct TfidfTables {
    u64 *cnt_keys, *cnt_vals, *dict_keys, *dict_vals;
    u64 cnt_mask, dict_mask;
    TfidfTables(Args& a, const torch::Tensor& ck, const torch::Tensor& cv,
                const torch::Tensor& dk, const torch::Tensor& dv) {
        cnt_keys = a.table(ck, "cnt_keys", &cnt_mask);
        cnt_vals = a.dev<u64>(cv, "cnt_vals", ck.numel());
        dict_keys = a.table(dk, "dict_keys", &dict_mask);
        dict_vals = a.dev<u64>(dv, "dict_vals", dk.numel());
    }
};
}  // namespace

// Returns per-block mark counts; python computes exclusive offsets.
torch::Tensor mark_counts(torch::Tensor text, long mode) {
    Args a;
    const u8* t = a.dev<const u8>(text, "text");
    const long n = text.numel();
    const long nblocks = tiles_for(n, SCAN_SPAN);
    auto counts = torch::empty({std::max(nblocks, 1L)},
                               like(text, torch::kUInt32));
    if (n == 0) { counts.zero_(); return counts; }
    u32* c = a.dev<u32>(counts, "counts");
    hipLaunchKernelGGL(count_marks_kernel, dim3((u32)nblocks), dim3(BLOCK),
                       0, a.stream(), t, n, (int)mode, SCAN_ITERS, c);
    return counts;
}

// block_offsets: the exclusive scan of mark_counts' result; out: one slot
// per mark (the scan's total, which only the device knows).
void mark_positions(torch::Tensor text, long mode,
                    torch::Tensor block_offsets, torch::Tensor out) {
    Args a;
    const u8* t = a.dev<const u8>(text, "text");
    const long n = text.numel();
    const long nblocks = tiles_for(n, SCAN_SPAN);
    const u32* offs = a.dev_min<const u32>(block_offsets, "block_offsets",
                                           nblocks);
    u32* o = a.dev<u32>(out, "out");
    if (n == 0 || out.numel() == 0) return;
    hipLaunchKernelGGL(write_marks_kernel, dim3((u32)nblocks), dim3(BLOCK),
                       0, a.stream(), t, n, (int)mode, SCAN_ITERS, offs, o);
}

void tfidf_count(torch::Tensor text, torch::Tensor nl_pos,
                 torch::Tensor tok_start, torch::Tensor seen_keys,
                 torch::Tensor cnt_keys, torch::Tensor cnt_vals,
                 torch::Tensor dict_keys, torch::Tensor dict_vals,
                 long pos_base, long doc_base) {
    Args a;
    const u8* t = a.dev<const u8>(text, "text");
    const u32* nl = a.dev<const u32>(nl_pos, "nl_pos");
    const u32* tok = a.dev<const u32>(tok_start, "tok_start");
    u64 seen_mask;
    u64* seen = a.table(seen_keys, "seen_keys", &seen_mask);
    const TfidfTables tb(a, cnt_keys, cnt_vals, dict_keys, dict_vals);
    const long n_tok = tok_start.numel();
    if (n_tok == 0) return;
    hipLaunchKernelGGL(tfidf_count_kernel,
        dim3(grid_for(n_tok)), dim3(BLOCK), 0, a.stream(),
        t, text.numel(), nl, nl_pos.numel(), tok, n_tok, seen, seen_mask,
        tb.cnt_keys, tb.cnt_vals, tb.cnt_mask, tb.dict_keys, tb.dict_vals,
        tb.dict_mask, (u64)pos_base, (u64)doc_base);
}

// `meta` is int32[>= 3], zeroed by the caller: the kernel ORs 1 into
// meta[0] when the fallback seen table overflowed (host must rerun the
// chunk via the token-centric kernel) and adds the chunk's document
// count (newlines, +1 for an unterminated tail) to meta[2]; meta[1] is
// the ablation sink.
void tfidf_count_docs(torch::Tensor text, torch::Tensor cnt_keys,
                      torch::Tensor cnt_vals, torch::Tensor dict_keys,
                      torch::Tensor dict_vals, long pos_base,
                      torch::Tensor fb_seen, torch::Tensor meta,
                      long ablate) {
    Args a;
    const u8* t = a.dev<const u8>(text, "text");
    const TfidfTables tb(a, cnt_keys, cnt_vals, dict_keys, dict_vals);
    u64 fb_mask;
    u64* fb = a.table(fb_seen, "fb_seen", &fb_mask);
    u32* m = (u32*)a.dev_min<int>(meta, "meta", 3);
    TORCH_CHECK(text.numel() < (1L << 31), "text: chunk must be < 2 GiB");
    const long n = text.numel();
    if (n == 0) return;
    long waves_needed = tiles_for(n, DOC_SPAN);        // a span per wave
    long blocks = std::min<long>(tiles_for(waves_needed, DOC_WAVES), 8192);
    hipLaunchKernelGGL(tfidf_docs_kernel, dim3((u32)blocks),
        dim3(DOC_WAVES * WAVE), 0, a.stream(), t, n,
        tb.cnt_keys, tb.cnt_vals, tb.cnt_mask, tb.dict_keys, tb.dict_vals,
        tb.dict_mask, (u64)pos_base, fb, fb_mask, m, (u32)ablate);
}

long tfidf_span_bytes() { return DOC_SPAN; }
