// dampr_amd gfx950 table kernels: what finishes a TF-IDF run once
// dampr_tfidf.hip has counted.  Merge / put / lookup / extract over the
// open-addressing u64 tables of common.h (K6 combine and extraction), the
// idf epilogue (K9 broadcast-apply), token string gather and the TSV sink.
// All are small grid-stride kernels over table slots or result rows.
#include <hip/hip_runtime.h>
#include "host.h"
#include "ops.h"

#include "common.h"
#include "compact.h"

#define BLOCK 256

// ---------------------------------------------------------------- table ops
__global__ void table_merge_kernel(const u64* __restrict__ in_keys,
                                   const long* __restrict__ in_vals,
                                   long n, u64* __restrict__ keys,
                                   u64* __restrict__ vals, u64 mask) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        u64 k = in_keys[i];
        if (k) table_add_u64(keys, vals, mask, k, (u64)in_vals[i]);
    }
}

__global__ void table_put_kernel(const u64* __restrict__ in_keys,
                                 const u64* __restrict__ in_vals, long n,
                                 u64* __restrict__ keys,
                                 u64* __restrict__ vals, u64 mask) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        u64 k = in_keys[i];
        if (!k) continue;
        u64 slot;
        if (table_insert_u64(keys, mask, k, &slot))
            vals[slot] = in_vals[i];
    }
}

// Compacts the live slots of a table; output order is free (callers sort
// by key).  One block per tile of COMPACT_TILE slots, tiled as the row
// filters tile (compact.h): ballot + popcount per 64-slot strip, wave
// counts in LDS, then ONE returning add on the cursor per tile for the
// tile's output base, where a per-key cursor add ran ~100k same-address
// atomics one after another.  A live lane writes to base + the counts of
// the waves before its own + the strips before its own + its rank in the
// strip's ballot, guarded by n_out.  cursor[0] ends at the live count
// whatever n_out is.
__global__ void __launch_bounds__(COMPACT_BLOCK)
table_extract_kernel(const u64* __restrict__ keys,
                     const u64* __restrict__ vals, long cap,
                     u64* __restrict__ out_k, long* __restrict__ out_v,
                     long n_out, u64* __restrict__ cursor) {
    __shared__ u64 tile_base;
    const long base = compact_first_row();
    u64 k[COMPACT_STRIPS];
    u64 ballots[COMPACT_STRIPS];
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        const long slot = base + (long)s * WAVE;
        k[s] = slot < cap ? keys[slot] : 0ULL;
    }
#pragma unroll
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        ballots[s] = __ballot(k[s] != 0ULL);
        cnt += __popcll(ballots[s]);
    }
    const int* wave_cnt = compact_wave_counts(cnt);
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < COMPACT_WAVES; ++w) total += wave_cnt[w];
        tile_base = total ? atomicAdd(cursor, (u64)total) : 0ULL;
    }
    __syncthreads();
    long pos = (long)tile_base;
#pragma unroll
    for (int w = 0; w < COMPACT_WAVES; ++w)
        if (w < compact_wave()) pos += wave_cnt[w];
#pragma unroll
    for (int s = 0; s < COMPACT_STRIPS; ++s)
        pos = compact_emit(ballots[s], pos, n_out, [&](long o) {
            out_k[o] = k[s];
            out_v[o] = (long)vals[base + (long)s * WAVE];
        });
}

__global__ void table_lookup_kernel(const u64* __restrict__ keys,
                                    const u64* __restrict__ vals, u64 mask,
                                    const u64* __restrict__ query, long n,
                                    u64* __restrict__ out) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        u64 k = query[i];
        u64 slot = k & mask;
        u64 r = 0;
        while (true) {
            u64 cur = keys[slot];
            if (cur == k) { r = vals[slot]; break; }
            if (cur == 0) break;
            slot = (slot + 1) & mask;
        }
        out[i] = r;
    }
}

// ------------------------------------------------------------------ epilogue
// idf = log(1 + total/df): the reference's cross_right scalar apply (K9 +
// benchmarks/tf-idf-dampr.py:18-20), fused elementwise.
__global__ void idf_kernel(const long* __restrict__ df, long n,
                           double total, double* __restrict__ out) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        out[i] = log(1.0 + total / (double)df[i]);
}

// Gather token strings: out[offsets[i] .. offsets[i]+len_i) = bytes of
// token i (packed = pos<<8 | len).
__global__ void gather_tokens_kernel(const u8* __restrict__ text,
                                     const u64* __restrict__ packed, long n,
                                     const long* __restrict__ offsets,
                                     u8* __restrict__ out) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        u64 pk = packed[i];
        u32 pos = (u32)(pk >> 8);
        u32 len = (u32)(pk & 0xFF);
        long o = offsets[i];
        for (u32 j = 0; j < len; ++j)
            out[o + j] = lower_ascii(text[pos + j]);
    }
}

// ------------------------------------------------------------------ tsv sink
// Device-side TSV formatting (K10's "serialize results" role): rows are
// "token\tDF\tIDF\n" with IDF fixed at 9 decimals.  Two passes: sizes
// (host cumsums them) then formatted writes.  Replaces a per-row Python
// format loop that dominated step time.

__device__ __forceinline__ int dec_digits_u64(u64 v) {
    int d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

__device__ __forceinline__ void fmt_idf_parts(double x, u64* int_part,
                                              u64* frac_part) {
    double scaled = x * 1e9 + 0.5;
    u64 v = (u64)scaled;
    *int_part = v / 1000000000ULL;
    *frac_part = v % 1000000000ULL;
}

__global__ void tsv_sizes_kernel(const long* __restrict__ lens,
                                 const long* __restrict__ df,
                                 const double* __restrict__ idf, long n,
                                 long* __restrict__ sizes) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        u64 ip, fp;
        fmt_idf_parts(idf[i], &ip, &fp);
        sizes[i] = lens[i] + 1 + dec_digits_u64((u64)df[i]) + 1
                 + dec_digits_u64(ip) + 1 + 9 + 1;
    }
}

__device__ __forceinline__ u8* write_u64_dec(u8* p, u64 v, int width) {
    for (int j = width - 1; j >= 0; --j) { p[j] = '0' + (v % 10); v /= 10; }
    return p + width;
}

__global__ void tsv_format_kernel(const u8* __restrict__ blob,
                                  const long* __restrict__ tok_off,
                                  const long* __restrict__ lens,
                                  const long* __restrict__ df,
                                  const double* __restrict__ idf,
                                  const long* __restrict__ row_off, long n,
                                  u8* __restrict__ out) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        u8* p = out + row_off[i];
        const u8* t = blob + tok_off[i];
        for (long j = 0; j < lens[i]; ++j) *p++ = t[j];
        *p++ = '\t';
        u64 d = (u64)df[i];
        p = write_u64_dec(p, d, dec_digits_u64(d));
        *p++ = '\t';
        u64 ip, fp;
        fmt_idf_parts(idf[i], &ip, &fp);
        p = write_u64_dec(p, ip, dec_digits_u64(ip));
        *p++ = '.';
        p = write_u64_dec(p, fp, 9);
        *p++ = '\n';
    }
}

// ==========================================================================
// Host wrappers
// ==========================================================================

namespace {
// A table and its value array, one value per slot.
struct Table {
    u64 *keys, *vals;
    u64 mask;
    Table(Args& a, const torch::Tensor& k, const torch::Tensor& v) {
        keys = a.table(k, "keys", &mask);
        vals = a.dev<u64>(v, "vals", k.numel());
    }
};
}  // namespace

void table_merge(torch::Tensor in_keys, torch::Tensor in_vals,
                 torch::Tensor keys, torch::Tensor vals) {
    Args a;
    const long n = in_keys.numel();
    const u64* ik = a.dev<const u64>(in_keys, "in_keys");
    const long* iv = a.dev<const long>(in_vals, "in_vals", n);
    const Table t(a, keys, vals);
    if (n == 0) return;
    hipLaunchKernelGGL(table_merge_kernel, dim3(grid_for(n)), dim3(BLOCK),
        0, a.stream(), ik, iv, n, t.keys, t.vals, t.mask);
}

void table_put(torch::Tensor in_keys, torch::Tensor in_vals,
               torch::Tensor keys, torch::Tensor vals) {
    Args a;
    const long n = in_keys.numel();
    const u64* ik = a.dev<const u64>(in_keys, "in_keys");
    const u64* iv = a.dev<const u64>(in_vals, "in_vals", n);
    const Table t(a, keys, vals);
    if (n == 0) return;
    hipLaunchKernelGGL(table_put_kernel, dim3(grid_for(n)), dim3(BLOCK),
        0, a.stream(), ik, iv, n, t.keys, t.vals, t.mask);
}

// The extract walks slots, it does not probe: any slot count will do.
std::vector<torch::Tensor> table_extract(torch::Tensor keys,
                                         torch::Tensor vals, long n_out) {
    Args a;
    const long cap = keys.numel();
    TORCH_CHECK(n_out >= 0, "n_out: must be >= 0");
    const u64* k = a.dev<const u64>(keys, "keys");
    const u64* v = a.dev_min<const u64>(vals, "vals", cap);
    auto out_k = torch::empty({n_out}, like(keys, torch::kInt64));
    auto out_v = torch::empty({n_out}, like(keys, torch::kInt64));
    auto cursor = torch::zeros({1}, out_k.options());
    if (cap > 0)
        hipLaunchKernelGGL(table_extract_kernel,
            dim3((u32)tiles_for(cap, COMPACT_TILE)), dim3(COMPACT_BLOCK), 0,
            a.stream(), k, v, cap, a.dev<u64>(out_k, "out_k"),
            a.dev<long>(out_v, "out_v"), n_out,
            a.dev<u64>(cursor, "cursor"));
    return {out_k, out_v, cursor};
}

torch::Tensor table_lookup(torch::Tensor keys, torch::Tensor vals,
                           torch::Tensor query) {
    Args a;
    const Table t(a, keys, vals);
    const u64* q = a.dev<const u64>(query, "query");
    const long n = query.numel();
    auto out = torch::zeros({n}, query.options());
    if (n > 0)
        hipLaunchKernelGGL(table_lookup_kernel, dim3(grid_for(n)),
            dim3(BLOCK), 0, a.stream(), t.keys, t.vals, t.mask, q, n,
            a.dev<u64>(out, "out"));
    return out;
}

torch::Tensor idf(torch::Tensor df, double total) {
    Args a;
    const long* d = a.dev<const long>(df, "df");
    const long n = df.numel();
    auto out = torch::empty({n}, like(df, torch::kFloat64));
    if (n > 0)
        hipLaunchKernelGGL(idf_kernel, dim3(grid_for(n)), dim3(BLOCK), 0,
            a.stream(), d, n, total, a.dev<double>(out, "out"));
    return out;
}

// offsets: exclusive scan of the tokens' lengths (the low byte of each
// packed entry); total_bytes: its total, which sizes the result.
torch::Tensor gather_tokens(torch::Tensor text, torch::Tensor packed,
                            torch::Tensor offsets, long total_bytes) {
    Args a;
    const long n = packed.numel();
    const u8* t = a.dev<const u8>(text, "text");
    const u64* pk = a.dev<const u64>(packed, "packed");
    const long* off = a.dev<const long>(offsets, "offsets", n);
    TORCH_CHECK(total_bytes >= 0, "total_bytes: must be >= 0");
    auto out = torch::empty({std::max(total_bytes, 1L)},
                            like(text, torch::kUInt8));
    if (n > 0)
        hipLaunchKernelGGL(gather_tokens_kernel, dim3(grid_for(n)),
            dim3(BLOCK), 0, a.stream(), t, pk, n, off,
            a.dev<u8>(out, "out"));
    return out;
}

torch::Tensor tsv_sizes(torch::Tensor lens, torch::Tensor df,
                        torch::Tensor idf) {
    Args a;
    const long n = lens.numel();
    const long* l = a.dev<const long>(lens, "lens");
    const long* d = a.dev<const long>(df, "df", n);
    const double* w = a.dev<const double>(idf, "idf", n);
    auto out = torch::empty({std::max(n, 1L)}, like(lens, torch::kInt64));
    if (n > 0)
        hipLaunchKernelGGL(tsv_sizes_kernel, dim3(grid_for(n)), dim3(BLOCK),
            0, a.stream(), l, d, w, n, a.dev<long>(out, "out"));
    return out;
}

// row_off: exclusive scan of tsv_sizes' result (which has an entry even
// for n == 0); total_bytes: its total.
torch::Tensor tsv_format(torch::Tensor blob, torch::Tensor tok_off,
                         torch::Tensor lens, torch::Tensor df,
                         torch::Tensor idf, torch::Tensor row_off,
                         long total_bytes) {
    Args a;
    const long n = lens.numel();
    const u8* b = a.dev<const u8>(blob, "blob");
    const long* to = a.dev<const long>(tok_off, "tok_off", n);
    const long* l = a.dev<const long>(lens, "lens");
    const long* d = a.dev<const long>(df, "df", n);
    const double* w = a.dev<const double>(idf, "idf", n);
    const long* ro = a.dev_min<const long>(row_off, "row_off", n);
    TORCH_CHECK(total_bytes >= 0, "total_bytes: must be >= 0");
    auto out = torch::empty({std::max(total_bytes, 1L)},
                            like(blob, torch::kUInt8));
    if (n > 0)
        hipLaunchKernelGGL(tsv_format_kernel, dim3(grid_for(n)),
            dim3(BLOCK), 0, a.stream(), b, to, l, d, w, ro, n,
            a.dev<u8>(out, "out"));
    return out;
}
