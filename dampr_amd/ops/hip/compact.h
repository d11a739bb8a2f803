// The stable two-pass tile compaction both row filters are built on
// (dampr_filter.hip, dampr_strfilter.hip).  A filter supplies a row
// predicate and an emit step; tiling and output position live here.
//
//   count pass    one block per tile of COMPACT_TILE rows: predicate,
//                 ballot + popcount per 64-row strip, per-wave counts summed
//                 -> block_counts[tile]            (compact_store_total)
//   (host glue)   exclusive scan of block_counts (torch.cumsum); its last
//                 entry is read once to size the outputs exactly
//   scatter pass  same tiling, same ballots; a survivor goes to
//                 block_off[tile] + the counts of the waves before its own
//                 (compact_wave_pos) + the strips before its own + its rank
//                 in its strip's ballot           (compact_emit)
//
// Order: a wave owns COMPACT_STRIPS consecutive 64-row strips, waves of a
// block own consecutive strip groups, blocks own consecutive tiles, and
// within a strip mbcnt counts the surviving lanes below this one.  Output
// position is therefore monotone in input position: the compaction is
// stable, which is what lets a filtered sorted run stay sorted.
//
// There is no inter-block communication inside a launch (no decoupled
// look-back, no spin): the scan between the two launches carries it.
//
// How a kernel walks its strips is its own choice (unrolled with the
// ballots in registers, or rolled with the ballots in LDS); the helpers
// below are the parts that must agree between every pass of every filter.
#pragma once

#include "common.h"

#define COMPACT_BLOCK 256
#define COMPACT_WAVES (COMPACT_BLOCK / WAVE)
#define COMPACT_STRIPS 16                      // 64-row strips per wave
#define COMPACT_TILE (COMPACT_BLOCK * COMPACT_STRIPS)

__device__ __forceinline__ int compact_lane() {
    return threadIdx.x & (WAVE - 1);
}
__device__ __forceinline__ int compact_wave() { return threadIdx.x / WAVE; }

// This lane's row of its wave's strip 0; strip s is s * WAVE rows on.
__device__ __forceinline__ long compact_first_row() {
    return (long)blockIdx.x * COMPACT_TILE +
           (long)compact_wave() * (COMPACT_STRIPS * WAVE) + compact_lane();
}

// Every wave's survivor count (cnt, wave-uniform), readable by the whole
// block once this returns.
__device__ __forceinline__ const int* compact_wave_counts(int cnt) {
    __shared__ int wave_cnt[COMPACT_WAVES];
    if (compact_lane() == 0) wave_cnt[compact_wave()] = cnt;
    __syncthreads();
    return wave_cnt;
}

// Count pass: the tile's survivor total.
__device__ __forceinline__ void compact_store_total(
        const int* wave_cnt, int* __restrict__ block_counts) {
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < COMPACT_WAVES; ++w) total += wave_cnt[w];
        block_counts[blockIdx.x] = total;
    }
}

// Scatter pass: the output position of this wave's first survivor.
__device__ __forceinline__ long compact_wave_pos(
        const int* wave_cnt, const long* __restrict__ block_off) {
    long pos = block_off[blockIdx.x];
#pragma unroll
    for (int w = 0; w < COMPACT_WAVES; ++w)
        if (w < compact_wave()) pos += wave_cnt[w];
    return pos;
}

// Scatter pass, one strip: if this lane's row survived (its bit of the
// strip's ballot), emit(o) writes it to its output slot o.  ``pos`` is the
// slot of the strip's first survivor; returns the next strip's.
template <typename Emit>
__device__ __forceinline__ long compact_emit(u64 ballot, long pos, long n_out,
                                             Emit emit) {
    if ((ballot >> compact_lane()) & 1ULL) {
        const long o = pos + __builtin_amdgcn_mbcnt_hi(
            (u32)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((u32)ballot, 0u));
        // o < n_out whenever block_off is the scan of this program's
        // counts over these columns; the guard keeps a mismatched call
        // from writing out of bounds
        if (o < n_out) emit(o);
    }
    return pos + __popcll(ballot);
}
