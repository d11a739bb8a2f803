// Sort/group/join kernels for the dampr_amd device engine (gfx950).
//
// Roles: K2/K3 radix partition+sort (replaces the
// reference's per-batch Python sort, dataset.py:161-188), K5/K7 segment +
// segmented reduce (grouped_read + fold, dataset.py:429-433/base.py:197-207)
// and K8 hash join (reference's sort-merge InnerJoin/LeftJoin,
// base.py:259-315).
//
// Sort design: stable LSD radix, 8-bit digits.  Per pass: block histograms
// (bin-major), a device exclusive scan (torch.cumsum at the Python layer —
// metadata-sized), then a stable scatter whose in-block ranks come from
// wave64 ballot bit-split matching + per-wave LDS bin histograms.
#include <hip/hip_runtime.h>
#include "host.h"
#include "ops.h"

#include "common.h"

#define RS_BLOCK 256
#define RS_TPB 16                         // tiles per block
#define RS_SPAN (RS_BLOCK * RS_TPB)       // elements per block

// ------------------------------------------------------------------ radix

__global__ void rs_hist_kernel(const u64* __restrict__ keys, long n,
                               int shift, u32* __restrict__ hist,
                               int nblocks) {
    __shared__ u32 h[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) h[i] = 0;
    __syncthreads();
    long base = (long)blockIdx.x * RS_SPAN;
    for (int t = 0; t < RS_TPB; ++t) {
        long i = base + (long)t * RS_BLOCK + threadIdx.x;
        if (i < n)
            atomicAdd(&h[(u32)((keys[i] >> shift) & 255)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 256; b += blockDim.x)
        hist[(long)b * nblocks + blockIdx.x] = h[b];
}

// Stable scatter with span-level LDS binning: the block's whole
// RS_SPAN tile is staged into LDS *grouped by bin* (stable ranks from
// wave64 ballot bit-splits + per-wave histograms, exactly one LDS slot
// per element), then written out bin-run by bin-run — consecutive LDS
// positions within a bin map to consecutive global addresses, so the
// HBM writes coalesce into ~(span/256)-element runs instead of the
// per-element random scatter of the naive form (measured ~2x pass
// throughput on uniform u64 keys; profiles/README.md).
__global__ void __launch_bounds__(RS_BLOCK)
rs_scatter_kernel(const u64* __restrict__ keys,
                  const u32* __restrict__ payload, long n,
                  int shift,
                  const long* __restrict__ scanned,
                  int nblocks, u64* __restrict__ out_k,
                  u32* __restrict__ out_p) {
    __shared__ u64 lk[RS_SPAN];                  // 32 KB bin-grouped keys
    // source index within the span (u16: RS_SPAN = 4096) instead of the
    // u32 payload itself: 8 KB of LDS saved buys a third resident block
    // per CU (48 KB total), and the drain's payload gather stays inside
    // a 16 KB window (L1-resident)
    __shared__ unsigned short lsrc[RS_SPAN];     // 8 KB
    __shared__ u32 hist[256];                    // span histogram
    __shared__ u32 cursor[256];                  // LDS write cursor per bin
    __shared__ long gbase[256];                  // global base - span start
    __shared__ u32 whist[RS_BLOCK / WAVE][256];  // per-round wave counts
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;
    const long start = (long)blockIdx.x * RS_SPAN;
    const int count = (int)min((long)RS_SPAN, n - start);

    // span histogram; keys stay in registers (32 VGPRs) so phase C
    // does not re-read them from global
    u64 rk[RS_TPB];
    for (int b = tid; b < 256; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    #pragma unroll
    for (int t = 0; t < RS_TPB; ++t) {
        const int j = t * RS_BLOCK + tid;
        rk[t] = 0;
        if (j < count) {
            rk[t] = keys[start + j];
            atomicAdd(&hist[(u32)((rk[t] >> shift) & 255)], 1u);
        }
    }
    __syncthreads();
    // exclusive scan of the 256 bins (Hillis-Steele over LDS; the span
    // work is 4096 elements, this is noise)
    for (int d = 1; d < 256; d <<= 1) {
        u32 v = 0;
        if (tid < 256 && tid >= d) v = hist[tid - d];
        __syncthreads();
        if (tid < 256 && tid >= d) hist[tid] += v;
        __syncthreads();
    }
    // hist now holds the INCLUSIVE scan; span_start[b] = hist[b]-count[b]
    if (tid < 256) {
        u32 ex = tid ? hist[tid - 1] : 0u;
        cursor[tid] = ex;
        gbase[tid] = scanned[(long)tid * nblocks + blockIdx.x] - (long)ex;
    }
    __syncthreads();

    // stable bin-grouped stage into LDS, one 256-element round at a time
    #pragma unroll
    for (int t = 0; t < RS_TPB; ++t) {
        for (int j = tid; j < (RS_BLOCK / WAVE) * 256; j += blockDim.x)
            (&whist[0][0])[j] = 0;
        __syncthreads();
        const int j = t * RS_BLOCK + tid;
        const bool valid = j < count;
        const u64 k = rk[t];
        int b = 0;
        if (valid)
            b = (int)((k >> shift) & 255);
        // wave-wide same-bin mask via 8 ballot bit-splits
        u64 m = __ballot(valid);
        #pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            u64 bb = __ballot(valid && ((b >> bit) & 1));
            m &= ((b >> bit) & 1) ? bb : ~bb;
        }
        const u64 below = (1ULL << lane) - 1;
        const u32 rank = (u32)__popcll(m & below);
        if (valid && rank == 0)
            whist[wid][b] = (u32)__popcll(m);
        __syncthreads();
        if (valid) {
            u32 pos = cursor[b] + rank;
            for (int w = 0; w < wid; ++w) pos += whist[w][b];
            lk[pos] = k;
            lsrc[pos] = (unsigned short)j;
        }
        __syncthreads();
        for (int b2 = tid; b2 < 256; b2 += blockDim.x) {
            u32 tot = 0;
            for (int w = 0; w < RS_BLOCK / WAVE; ++w)
                tot += whist[w][b2];
            cursor[b2] += tot;
        }
        __syncthreads();
    }

    // coalesced drain: LDS position i of bin b lands at gbase[b] + i;
    // the payload gather reads a 16 KB window (L1-resident)
    for (int i = tid; i < count; i += blockDim.x) {
        u64 k = lk[i];
        int b = (int)((k >> shift) & 255);
        long dest = gbase[b] + i;
        out_k[dest] = k;
        out_p[dest] = payload[start + lsrc[i]];
    }
}

// Skip-pass detection in one streaming read: a byte pass is skippable
// iff that byte is CONSTANT across all keys, which is min==max per
// digit.  AND/OR-fold in registers (no per-element LDS atomics — the
// old 8x256 LDS histogram ran at 0.56 TB/s from atomic serialization;
// this runs at read bandwidth), wave-reduce, one atomic per wave.
// Digit d is constant iff and8[d] == or8[d] byte-wise.
__global__ void rs_digit_fold_kernel(const u64* __restrict__ keys, long n,
                                     u64* __restrict__ and_or) {
    const long stride = (long)gridDim.x * blockDim.x;
    u64 a = ~0ULL, o = 0ULL;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const u64 k = keys[i];
        a &= k;
        o |= k;
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a &= __shfl_down(a, d, WAVE);
        o |= __shfl_down(o, d, WAVE);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        atomicAnd(&and_or[0], a);
        atomicOr(&and_or[1], o);
    }
}

namespace {
// One radix pass's shape: byte-aligned digit, one block per RS_SPAN keys.
void check_radix_pass(long n, long shift, long nblocks) {
    TORCH_CHECK(shift >= 0 && shift <= 56 && shift % 8 == 0,
                "shift: one of 0, 8, ..., 56, got ", shift);
    TORCH_CHECK(nblocks == tiles_for(n, RS_SPAN), "nblocks: expected ",
                tiles_for(n, RS_SPAN), " blocks of RS_SPAN keys, got ",
                nblocks);
}
}  // namespace

torch::Tensor rs_digit_fold(torch::Tensor keys) {
    Args a;
    const u64* k = a.dev<const u64>(keys, "keys");
    auto and_or = torch::empty({2}, like(keys, torch::kInt64));
    and_or.index_put_({0}, -1);
    and_or.index_put_({1}, 0);
    long n = keys.numel();
    if (n)
        hipLaunchKernelGGL(rs_digit_fold_kernel,
            dim3(grid_for(n, RS_BLOCK, 2048)), dim3(RS_BLOCK), 0,
            a.stream(), k, n, a.dev<u64>(and_or, "and_or"));
    return and_or;
}

long rs_span() { return RS_SPAN; }

torch::Tensor rs_hist(torch::Tensor keys, long shift, long nblocks) {
    Args a;
    const u64* k = a.dev<const u64>(keys, "keys");
    const long n = keys.numel();
    check_radix_pass(n, shift, nblocks);
    // int32 storage (counts <= RS_SPAN): torch.cumsum upcasts to i64 in
    // one fused pass (dtype=), so no separate conversion kernel/alloc
    auto hist = torch::empty({256L * nblocks}, like(keys, torch::kInt));
    if (n == 0) return hist;
    hipLaunchKernelGGL(rs_hist_kernel, dim3((u32)nblocks), dim3(RS_BLOCK),
        0, a.stream(), k, n, (int)shift, a.dev<u32>(hist, "hist"),
        (int)nblocks);
    return hist;
}

// scanned: exclusive scan of rs_hist's result for the same keys and shift.
void rs_scatter(torch::Tensor keys, torch::Tensor payload,
                torch::Tensor scanned, long shift, long nblocks,
                torch::Tensor out_k, torch::Tensor out_p) {
    Args a;
    const u64* k = a.dev<const u64>(keys, "keys");
    const long n = keys.numel();
    check_radix_pass(n, shift, nblocks);
    const u32* p = a.dev<const u32>(payload, "payload", n);
    const long* sc = a.dev<const long>(scanned, "scanned", 256L * nblocks);
    u64* ok = a.dev<u64>(out_k, "out_k", n);
    u32* op = a.dev<u32>(out_p, "out_p", n);
    if (n == 0) return;
    check_distinct(out_k, "out_k", keys, "keys");
    check_distinct(out_p, "out_p", payload, "payload");
    hipLaunchKernelGGL(rs_scatter_kernel, dim3((u32)nblocks),
        dim3(RS_BLOCK), 0, a.stream(), k, p, n, (int)shift, sc,
        (int)nblocks, ok, op);
}

// ------------------------------------------------------------- hash join
// Build: chain right-side rows per key (slot -> head row, next[] links).
// Probe: count matches per left row, then emit (l, r) index pairs at
// exclusive offsets.  Row indices allow the Python layer to gather values.
//
// Keys are RAW u64 (dictionary rank ids start at 0; int columns may
// contain 0), so key 0 must be representable even though the open table
// uses 0 as its EMPTY sentinel: slot mask+1 of t_head is a dedicated
// zero-key chain and key 0 never enters t_keys (t_head has mask+2
// entries; the Python layer allocates cap+1).

__global__ void hj_build_kernel(const u64* __restrict__ keys_r, long nr,
                                u64* __restrict__ t_keys,
                                long* __restrict__ t_head, u64 mask,
                                long* __restrict__ next) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nr;
         i += stride) {
        u64 k = keys_r[i];
        u64 slot;
        if (k == 0ULL)
            slot = mask + 1;              // dedicated zero-key chain
        else
            table_insert_u64(t_keys, mask, k, &slot);
        long old = atomicExch((unsigned long long*)&t_head[slot],
                              (unsigned long long)i);
        next[i] = old;
    }
}

__device__ __forceinline__ long hj_find(const u64* t_keys,
                                        const long* t_head, u64 mask,
                                        u64 k) {
    if (k == 0ULL) return t_head[mask + 1];
    u64 slot = k & mask;
    while (true) {
        u64 cur = t_keys[slot];
        if (cur == k) return t_head[slot];
        if (cur == 0) return -1;
        slot = (slot + 1) & mask;
    }
}

__global__ void hj_count_kernel(const u64* __restrict__ keys_l, long nl,
                                const u64* __restrict__ t_keys,
                                const long* __restrict__ t_head, u64 mask,
                                const long* __restrict__ next,
                                int left_outer,
                                long* __restrict__ counts) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nl;
         i += stride) {
        u64 k = keys_l[i];
        long c = 0;
        for (long r = hj_find(t_keys, t_head, mask, k); r >= 0;
             r = next[r])
            ++c;
        counts[i] = (c == 0 && left_outer) ? 1 : c;
    }
}

__global__ void hj_emit_kernel(const u64* __restrict__ keys_l, long nl,
                               const u64* __restrict__ t_keys,
                               const long* __restrict__ t_head, u64 mask,
                               const long* __restrict__ next,
                               const long* __restrict__ offsets,
                               int left_outer,
                               long* __restrict__ out_l,
                               long* __restrict__ out_r,
                               u8* __restrict__ r_matched) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nl;
         i += stride) {
        u64 k = keys_l[i];
        long o = offsets[i];
        long c = 0;
        for (long r = hj_find(t_keys, t_head, mask, k); r >= 0;
             r = next[r]) {
            out_l[o] = i;
            out_r[o] = r;
            if (r_matched) r_matched[r] = 1;
            ++o;
            ++c;
        }
        if (c == 0 && left_outer) {
            out_l[o] = i;
            out_r[o] = -1;
        }
    }
}

namespace {
// The chained table hj_build fills: a power of two of key slots, a chain
// head per slot plus the zero-key chain's, and the rows' next links.
struct JoinTable {
    u64* keys;
    long *head, *next;
    u64 mask;
    JoinTable(Args& a, const torch::Tensor& t_keys,
              const torch::Tensor& t_head, const torch::Tensor& nxt,
              long nr = 0) {
        keys = a.table(t_keys, "t_keys", &mask);
        head = a.dev<long>(t_head, "t_head", t_keys.numel() + 1);
        next = a.dev_min<long>(nxt, "next", nr);
    }
};
}  // namespace

void hj_build(torch::Tensor keys_r, torch::Tensor t_keys,
              torch::Tensor t_head, torch::Tensor next) {
    Args a;
    const u64* kr = a.dev<const u64>(keys_r, "keys_r");
    const long nr = keys_r.numel();
    const JoinTable t(a, t_keys, t_head, next, nr);
    if (nr == 0) return;
    hipLaunchKernelGGL(hj_build_kernel, dim3(grid_for(nr)), dim3(256), 0,
        a.stream(), kr, nr, t.keys, t.head, t.mask, t.next);
}

// One count per left row (one entry even when there are no rows).
torch::Tensor hj_count(torch::Tensor keys_l, torch::Tensor t_keys,
                       torch::Tensor t_head, torch::Tensor next,
                       long left_outer) {
    Args a;
    const u64* kl = a.dev<const u64>(keys_l, "keys_l");
    const JoinTable t(a, t_keys, t_head, next);
    const long nl = keys_l.numel();
    auto counts = torch::zeros({std::max(nl, 1L)},
                               like(keys_l, torch::kInt64));
    if (nl)
        hipLaunchKernelGGL(hj_count_kernel, dim3(grid_for(nl)), dim3(256),
            0, a.stream(), kl, nl, t.keys, t.head, t.mask, t.next,
            (int)left_outer, a.dev<long>(counts, "counts"));
    return counts;
}

// offsets: exclusive scan of hj_count's result, of its length; total: the
// scan's total; nr: the build side's row count.
std::vector<torch::Tensor> hj_emit(torch::Tensor keys_l,
                                   torch::Tensor t_keys,
                                   torch::Tensor t_head,
                                   torch::Tensor next,
                                   torch::Tensor offsets, long total,
                                   long left_outer, long track_matched,
                                   long nr) {
    Args a;
    const u64* kl = a.dev<const u64>(keys_l, "keys_l");
    const long nl = keys_l.numel();
    TORCH_CHECK(total >= 0, "total: must be >= 0");
    TORCH_CHECK(nr >= 0, "nr: must be >= 0");
    const JoinTable t(a, t_keys, t_head, next, nr);
    const long* off = a.dev<const long>(offsets, "offsets",
                                        std::max(nl, 1L));
    auto i64 = like(keys_l, torch::kInt64);
    auto out_l = torch::empty({std::max(total, 1L)}, i64);
    auto out_r = torch::empty({std::max(total, 1L)}, i64);
    auto matched = torch::zeros({std::max(nr, 1L)},
                                like(keys_l, torch::kUInt8));
    if (nl && total)
        hipLaunchKernelGGL(hj_emit_kernel, dim3(grid_for(nl)), dim3(256),
            0, a.stream(), kl, nl, t.keys, t.head, t.mask, t.next, off,
            (int)left_outer, a.dev<long>(out_l, "out_l"),
            a.dev<long>(out_r, "out_r"),
            track_matched ? a.dev<u8>(matched, "matched") : (u8*)nullptr);
    return {out_l, out_r, matched};
}

// ------------------------------------------------- var-len value gather
// Row gather for byte-arena (string) value columns: out row r =
// blob[src_off[r] .. src_off[r]+lens[r]).  One wave per row; lanes copy
// 64 bytes per iteration (typical rows are short tokens/lines, one
// iteration).  The reorder op under sort permutations, join row indices
// and partition routing for var-len values.

__global__ void varlen_gather_kernel(const u8* __restrict__ blob,
                                     const long* __restrict__ src_off,
                                     const long* __restrict__ lens,
                                     const long* __restrict__ new_offs,
                                     long n, u8* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    const int wpb = blockDim.x / WAVE;
    const long stride = (long)gridDim.x * wpb;
    for (long r = (long)blockIdx.x * wpb + wid; r < n; r += stride) {
        const long so = src_off[r];
        const long ln = lens[r];
        const long do_ = new_offs[r];
        for (long j = lane; j < ln; j += WAVE)
            out[do_ + j] = blob[so + j];
    }
}

// new_offs: the output rows' offsets, n + 1 entries as StrVals keeps them
// (the kernel reads the first n).  out must hold new_offs' total, which
// only the device knows: its size is the caller's to get right.
void varlen_gather(torch::Tensor blob, torch::Tensor src_off,
                   torch::Tensor lens, torch::Tensor new_offs,
                   torch::Tensor out) {
    Args a;
    const long n = src_off.numel();
    const u8* b = a.dev<const u8>(blob, "blob");
    const long* so = a.dev<const long>(src_off, "src_off");
    const long* ln = a.dev<const long>(lens, "lens", n);
    const long* no = a.dev<const long>(new_offs, "new_offs", n + 1);
    u8* o = a.dev<u8>(out, "out");
    if (n == 0) return;
    hipLaunchKernelGGL(varlen_gather_kernel,
        dim3(grid_for(n * WAVE, 256, 8192)), dim3(256), 0, a.stream(),
        b, so, ln, no, n, o);
}

// ------------------------------------------------------ merge-path (K4)
// Stable 2-way merge of key-sorted runs (Merge Path, Green et al.): each
// block owns one output tile, finds its (i, j) split with a diagonal
// binary search, and its threads merge per-thread sub-segments found
// the same way.  K-way merge of spilled sorted runs = pairwise tree of
// these (log2 R passes) — replaces the cat+re-sort of sorted runs
// (reference's heapq.merge role, dataset.py:567-588).  ``bias`` is
// XORed into keys for comparisons only (1<<63 = signed order for i64
// keys; 0 = raw unsigned for f64-encoded keys), so no separate
// re-encode passes are needed.  Ties take run A first (stability).

#define MP_TILE 4096
#define MP_IPT 16

__device__ __forceinline__ long mp_diag(const u64* __restrict__ a,
                                        long na,
                                        const u64* __restrict__ b,
                                        long nb, long diag, u64 bias) {
    long lo = diag > nb ? diag - nb : 0;
    long hi = diag < na ? diag : na;
    while (lo < hi) {
        long mid = (lo + hi) >> 1;
        if ((a[mid] ^ bias) <= (b[diag - 1 - mid] ^ bias))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
mp_merge_kernel(const u64* __restrict__ ka, const u32* __restrict__ pa,
                long na, const u64* __restrict__ kb,
                const u32* __restrict__ pb, long nb, u64 bias,
                u64* __restrict__ out_k, u32* __restrict__ out_p) {
    const long total = na + nb;
    const long tile0 = (long)blockIdx.x * MP_TILE;
    if (tile0 >= total) return;
    const long tile1 = min(tile0 + (long)MP_TILE, total);
    // block split
    const long bi0 = mp_diag(ka, na, kb, nb, tile0, bias);
    const long bi1 = mp_diag(ka, na, kb, nb, tile1, bias);
    const long bj0 = tile0 - bi0;
    const long bj1 = tile1 - bi1;
    // per-thread split within the block's segments
    const long d0 = min(tile0 + (long)threadIdx.x * MP_IPT, tile1);
    const long d1 = min(d0 + (long)MP_IPT, tile1);
    if (d0 >= d1) return;
    long i = bi0 + mp_diag(ka + bi0, bi1 - bi0, kb + bj0, bj1 - bj0,
                           d0 - tile0, bias);
    long j = d0 - i;
    for (long o = d0; o < d1; ++o) {
        bool take_a;
        if (i >= bi1) take_a = false;
        else if (j >= bj1) take_a = true;
        else take_a = (ka[i] ^ bias) <= (kb[j] ^ bias);
        if (take_a) {
            out_k[o] = ka[i];
            out_p[o] = pa[i];
            ++i;
        } else {
            out_k[o] = kb[j];
            out_p[o] = pb[j];
            ++j;
        }
    }
}

void mp_merge(torch::Tensor ka, torch::Tensor pa, torch::Tensor kb,
              torch::Tensor pb, long bias_signed, torch::Tensor out_k,
              torch::Tensor out_p) {
    Args a;
    const long na = ka.numel(), nb = kb.numel();
    const long total = na + nb;
    const u64* a_k = a.dev<const u64>(ka, "ka");
    const u32* a_p = a.dev<const u32>(pa, "pa", na);
    const u64* b_k = a.dev<const u64>(kb, "kb");
    const u32* b_p = a.dev<const u32>(pb, "pb", nb);
    u64* ok = a.dev<u64>(out_k, "out_k", total);
    u32* op = a.dev<u32>(out_p, "out_p", total);
    if (total == 0) return;
    u64 bias = bias_signed ? 0x8000000000000000ULL : 0ULL;
    hipLaunchKernelGGL(mp_merge_kernel,
        dim3((u32)tiles_for(total, MP_TILE)), dim3(256), 0, a.stream(),
        a_k, a_p, na, b_k, b_p, nb, bias, ok, op);
}

// ----------------------------------- fused segmented reduce (K5 + K7)
// Group-by over a key-sorted column WITHOUT materializing per-element
// segment ids: kernel 1 counts segment starts per tile; a (tiny)
// device scan of tile counts gives each tile its base segment id;
// kernel 2 re-derives boundary flags from neighbor keys, scans them
// within the tile, writes each segment head's key to out_keys and
// folds values with the wave-segmented scan + one atomic per
// (wave, segment) tail.  Replaces the flags -> cumsum -> nonzero ->
// gather chain (4+ full-column passes and a host sync) with two
// column reads.

#define OP_SUM 0
#define OP_MIN 1
#define OP_MAX 2

#define SEG_TPB 16
#define SEG_SPAN (RS_BLOCK * SEG_TPB)

__global__ void seg_count_kernel(const u64* __restrict__ keys, long n,
                                 u32* __restrict__ counts) {
    const long start = (long)blockIdx.x * SEG_SPAN;
    const int count = (int)min((long)SEG_SPAN, n - start);
    u32 local = 0;
    for (int j = threadIdx.x; j < count; j += blockDim.x) {
        const long i = start + j;
        local += (i == 0) || (keys[i] != keys[i - 1]);
    }
    #pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1)
        local += __shfl_down(local, d, WAVE);
    __shared__ u32 wsum[RS_BLOCK / WAVE];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    if (lane == 0) wsum[wid] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 tot = 0;
        for (int w = 0; w < RS_BLOCK / WAVE; ++w) tot += wsum[w];
        counts[blockIdx.x] = tot;
    }
}

__device__ __forceinline__ void seg_atomic_fold(long* addr, long v,
                                                int op) {
    if (op == OP_SUM) {
        atomicAdd((u64*)addr, (u64)v);
    } else if (op == OP_MIN) {
        atomicMin((long long*)addr, (long long)v);
    } else {
        atomicMax((long long*)addr, (long long)v);
    }
}

__device__ __forceinline__ void seg_atomic_fold(double* addr, double v,
                                                int op) {
    if (op == OP_SUM) {
        atomicAdd(addr, v);
        return;
    }
    u64* a = (u64*)addr;
    u64 old = *a;
    while (true) {
        double cur = __longlong_as_double((long long)old);
        double nv = (op == OP_MIN) ? min(cur, v) : max(cur, v);
        if (nv == cur) break;
        u64 assumed = old;
        old = atomicCAS(a, assumed, (u64)__double_as_longlong(nv));
        if (old == assumed) break;
    }
}

template <typename V>
__global__ void __launch_bounds__(RS_BLOCK)
seg_reduce_fused_kernel(const u64* __restrict__ keys,
                        const V* __restrict__ vals, long n,
                        const long* __restrict__ tile_base, int op,
                        u64* __restrict__ out_keys,
                        V* __restrict__ out_vals) {
    const long start = (long)blockIdx.x * SEG_SPAN;
    const int count = (int)min((long)SEG_SPAN, n - start);
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    __shared__ long wseg[RS_BLOCK / WAVE];  // per-wave start counts
    __shared__ long round_tot;
    long base = tile_base[blockIdx.x];      // starts before this round
    for (int t = 0; t < SEG_TPB; ++t) {
        const int j = t * RS_BLOCK + threadIdx.x;
        const bool valid = j < count;
        const long i = start + j;
        u64 k = 0;
        V v = V(0);
        long f = 0;
        if (valid) {
            k = keys[i];
            v = vals[i];
            f = (i == 0) || (k != keys[i - 1]);
        }
        // wave-inclusive scan of start flags
        long fs = f;
        #pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            long x = __shfl_up(fs, d, WAVE);
            if (lane >= d) fs += x;
        }
        const long wave_tot = __shfl(fs, WAVE - 1, WAVE);
        if (lane == 0) wseg[wid] = wave_tot;
        __syncthreads();
        long wbase = base;
        for (int w = 0; w < wid; ++w) wbase += wseg[w];
        // seg id: starts at-or-before this element, minus one (fs == 0
        // for a run continuing from the left -> wbase - 1)
        const long seg = wbase + fs - 1;
        if (valid && f)
            out_keys[seg] = k;
        // wave-segmented value fold (runs are contiguous)
        V acc = v;
        long s = valid ? seg : -1;
        #pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            V v2 = __shfl_up(acc, d, WAVE);
            long s2 = __shfl_up(s, d, WAVE);
            if (lane >= d && s2 == s) {
                if (op == OP_SUM) acc += v2;
                else if (op == OP_MIN) acc = min(acc, v2);
                else acc = max(acc, v2);
            }
        }
        long s_next = __shfl_down(s, 1, WAVE);
        if (valid && (lane == WAVE - 1 || s_next != s))
            seg_atomic_fold(&out_vals[s], acc, op);
        if (threadIdx.x == 0) {
            long tot = 0;
            for (int w = 0; w < RS_BLOCK / WAVE; ++w) tot += wseg[w];
            round_tot = tot;
        }
        __syncthreads();
        base += round_tot;
        __syncthreads();
    }
}

torch::Tensor seg_count(torch::Tensor keys) {
    Args a;
    const u64* k = a.dev<const u64>(keys, "keys");
    const long n = keys.numel();
    const long nblocks = tiles_for(n, SEG_SPAN);
    auto counts = torch::empty({std::max(nblocks, 1L)},
                               like(keys, torch::kInt));
    if (n)
        hipLaunchKernelGGL(seg_count_kernel, dim3((u32)nblocks),
            dim3(RS_BLOCK), 0, a.stream(), k, n,
            a.dev<u32>(counts, "counts"));
    return counts;
}

// tile_base: exclusive scan of seg_count's result for the same keys;
// out_keys / out_vals: one slot per segment (the scan's total), out_vals
// of vals' dtype and preset to op's identity.
void seg_reduce_fused(torch::Tensor keys, torch::Tensor vals,
                      torch::Tensor tile_base, long op,
                      torch::Tensor out_keys, torch::Tensor out_vals) {
    Args a;
    const u64* k = a.dev<const u64>(keys, "keys");
    const long n = keys.numel();
    const long nblocks = tiles_for(n, SEG_SPAN);
    const long long* v = a.col(vals, "vals", n);
    const long* tb = a.dev<const long>(tile_base, "tile_base",
                                       std::max(nblocks, 1L));
    TORCH_CHECK(op == OP_SUM || op == OP_MIN || op == OP_MAX,
                "op: 0 (sum), 1 (min) or 2 (max), got ", op);
    long long* ov = a.col(out_vals, "out_vals");
    TORCH_CHECK(out_vals.scalar_type() == vals.scalar_type(),
                "out_vals: expected vals' dtype ", vals.scalar_type(),
                ", got ", out_vals.scalar_type());
    u64* ok = a.dev<u64>(out_keys, "out_keys", out_vals.numel());
    if (n == 0) return;
    if (vals.scalar_type() == torch::kFloat64)
        hipLaunchKernelGGL(seg_reduce_fused_kernel<double>,
            dim3((u32)nblocks), dim3(RS_BLOCK), 0, a.stream(), k,
            (const double*)v, n, tb, (int)op, ok, (double*)ov);
    else
        hipLaunchKernelGGL(seg_reduce_fused_kernel<long>,
            dim3((u32)nblocks), dim3(RS_BLOCK), 0, a.stream(), k,
            (const long*)v, n, tb, (int)op, ok, (long*)ov);
}
