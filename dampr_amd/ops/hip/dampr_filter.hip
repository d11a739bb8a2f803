// Row filter for the dampr_amd device engine (gfx950): a stable two-pass
// stream compaction of a (key, value) column pair under a conjunction of
// at most FILTER_MAX_CLAUSES comparisons against constants.
//
//   filter_count    one block per tile of FILTER_TILE rows: evaluate the
//                   conjunction, ballot + popcount per wave, block sum ->
//                   block_counts[tile]
//   (host glue)     exclusive scan of block_counts (torch.cumsum); its last
//                   entry is read once to size the outputs exactly
//   filter_scatter  same tiling, predicate re-evaluated (cheaper than a
//                   flag column: 2 x 8 B read per row instead of a 1 B write
//                   plus read and a second launch over it); survivor goes to
//                   block_off[tile] + wave_prefix + mbcnt(ballot)
//
// Order: a wave owns FILTER_STRIPS consecutive 64-row strips, waves of a
// block own consecutive strip groups, blocks own consecutive tiles, and
// within a strip mbcnt counts the surviving lanes below this one.  Output
// position is therefore monotone in input position: the compaction is
// stable, which is what lets a filtered sorted run stay sorted.
//
// There is no inter-block communication inside a launch (no decoupled
// look-back, no spin): the scan between the two launches carries it.
//
// The clause program travels by value in the kernel arguments.  The clause
// loop is fully unrolled so every program access has a constant index and
// stays a scalar kernarg load (a dynamic index would copy the struct to
// scratch).  Both value dtypes (i64, f64) are 8 bytes, so columns move as
// raw 64-bit words and a clause's domain says how to read them.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "common.h"
#include "filter_clause.h"

#define FILTER_BLOCK 256
#define FILTER_WAVES (FILTER_BLOCK / WAVE)
#define FILTER_STRIPS 16                       // 64-row strips per wave
#define FILTER_TILE (FILTER_BLOCK * FILTER_STRIPS)
struct FilterProgram {
    int n;
    int need_k;        // some clause reads the key column
    int need_v;
    int pad_;
    FilterClause c[FILTER_MAX_CLAUSES];
};

namespace {
inline hipStream_t cur_stream() {
    return at::hip::getCurrentHIPStream().stream();
}
}  // namespace

__device__ __forceinline__ bool filter_eval(const FilterProgram& prog,
                                            long long kraw, long long vraw) {
    bool keep = true;
#pragma unroll
    for (int i = 0; i < FILTER_MAX_CLAUSES; ++i) {
        if (i < prog.n) {
            const long long raw = prog.c[i].col ? vraw : kraw;
            const int dom = prog.c[i].dom;
            bool t;
            if (dom == FD_I64) {
                t = filter_cmp<long long>(prog.c[i].op, raw, prog.c[i].a,
                                          prog.c[i].b);
            } else {
                const long long bits =
                    dom == FD_FKEY ? fkey_decode_bits(raw) : raw;
                t = filter_cmp<double>(prog.c[i].op,
                                       __longlong_as_double(bits),
                                       __longlong_as_double(prog.c[i].a),
                                       __longlong_as_double(prog.c[i].b));
            }
            keep = keep && t;
        }
    }
    return keep;
}

// Does row r (of n) survive?  Loads only the columns the program reads.
__device__ __forceinline__ bool filter_row(const FilterProgram& prog,
                                           const long long* __restrict__ keys,
                                           const long long* __restrict__ vals,
                                           long r, long n) {
    if (r >= n) return false;
    const long long k = prog.need_k ? keys[r] : 0;
    const long long v = prog.need_v ? vals[r] : 0;
    return filter_eval(prog, k, v);
}

__global__ void __launch_bounds__(FILTER_BLOCK)
filter_count_kernel(const long long* __restrict__ keys,
                    const long long* __restrict__ vals, long n,
                    FilterProgram prog, int* __restrict__ block_counts) {
    __shared__ int wave_cnt[FILTER_WAVES];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const long base = (long)blockIdx.x * FILTER_TILE +
                      (long)wave * (FILTER_STRIPS * WAVE) + lane;
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < FILTER_STRIPS; ++s) {
        const bool p = filter_row(prog, keys, vals, base + (long)s * WAVE, n);
        cnt += __popcll(__ballot(p));
    }
    if (lane == 0) wave_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < FILTER_WAVES; ++w) total += wave_cnt[w];
        block_counts[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(FILTER_BLOCK)
filter_scatter_kernel(const long long* __restrict__ keys,
                      const long long* __restrict__ vals, long n,
                      FilterProgram prog, const long* __restrict__ block_off,
                      long long* __restrict__ out_k,
                      long long* __restrict__ out_v, long n_out) {
    __shared__ int wave_cnt[FILTER_WAVES];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const long base = (long)blockIdx.x * FILTER_TILE +
                      (long)wave * (FILTER_STRIPS * WAVE) + lane;
    u64 ballots[FILTER_STRIPS];
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < FILTER_STRIPS; ++s) {
        const bool p = filter_row(prog, keys, vals, base + (long)s * WAVE, n);
        ballots[s] = __ballot(p);
        cnt += __popcll(ballots[s]);
    }
    if (lane == 0) wave_cnt[wave] = cnt;
    __syncthreads();
    long pos = block_off[blockIdx.x];
#pragma unroll
    for (int w = 0; w < FILTER_WAVES; ++w)
        if (w < wave) pos += wave_cnt[w];
#pragma unroll
    for (int s = 0; s < FILTER_STRIPS; ++s) {
        const u64 b = ballots[s];
        if ((b >> lane) & 1ULL) {
            const long r = base + (long)s * WAVE;       // < n: it survived
            const long o = pos + __builtin_amdgcn_mbcnt_hi(
                (u32)(b >> 32), __builtin_amdgcn_mbcnt_lo((u32)b, 0u));
            // o < n_out whenever block_off is the scan of this program's
            // counts over these columns; the guard keeps a mismatched
            // call from writing out of bounds
            if (o < n_out) {
                out_k[o] = keys[r];
                out_v[o] = vals[r];
            }
        }
        pos += __popcll(b);
    }
}

namespace {
bool is_col(const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() &&
           (t.dtype() == torch::kInt64 || t.dtype() == torch::kFloat64);
}

// prog: 5 int64 per clause (col, dom, op, a, b)
FilterProgram make_program(const std::vector<int64_t>& prog,
                           const torch::Tensor& vals) {
    TORCH_CHECK(prog.size() % 5 == 0 && prog.size() >= 5 &&
                prog.size() <= 5 * FILTER_MAX_CLAUSES,
                "filter program: 1..", FILTER_MAX_CLAUSES,
                " clauses of (col, dom, op, a, b)");
    FilterProgram p = {};
    p.n = (int)(prog.size() / 5);
    for (int i = 0; i < p.n; ++i) {
        const int64_t* c = &prog[5 * i];
        TORCH_CHECK(c[0] == 0 || c[0] == 1, "filter clause: col is 0 or 1");
        TORCH_CHECK(c[1] >= FD_I64 && c[1] <= FD_FKEY,
                    "filter clause: unknown domain");
        TORCH_CHECK(c[2] >= FO_GT && c[2] <= FO_BETWEEN,
                    "filter clause: unknown op");
        // the key column is always i64 words: raw ints or encoded doubles
        TORCH_CHECK(c[0] == 1 || c[1] != FD_F64,
                    "filter clause: the key column has no f64 domain");
        TORCH_CHECK(c[0] == 0 ||
                    (c[1] == FD_F64) == (vals.dtype() == torch::kFloat64),
                    "filter clause: domain does not match the value dtype");
        p.c[i].col = (int)c[0];
        p.c[i].dom = (int)c[1];
        p.c[i].op = (int)c[2];
        p.c[i].a = c[3];
        p.c[i].b = c[4];
        if (c[0]) p.need_v = 1; else p.need_k = 1;
    }
    return p;
}

long check_columns(const torch::Tensor& keys, const torch::Tensor& vals) {
    TORCH_CHECK(is_col(keys) && keys.dtype() == torch::kInt64,
                "keys: contiguous i64 device tensor");
    TORCH_CHECK(is_col(vals) && vals.numel() == keys.numel(),
                "vals: contiguous i64/f64 device tensor of keys' length");
    const long n = keys.numel();
    TORCH_CHECK(n < (1L << 31), "filter: row count exceeds i32");
    return n;
}
}  // namespace

long filter_tile() { return FILTER_TILE; }

// Survivors per tile of FILTER_TILE rows: i32[ceil(n / FILTER_TILE)].
torch::Tensor filter_count(torch::Tensor keys, torch::Tensor vals,
                           std::vector<int64_t> prog) {
    const long n = check_columns(keys, vals);
    const FilterProgram p = make_program(prog, vals);
    const long nblocks = (n + FILTER_TILE - 1) / FILTER_TILE;
    auto counts = torch::empty({nblocks},
        torch::TensorOptions().dtype(torch::kInt32).device(keys.device()));
    if (nblocks > 0)
        hipLaunchKernelGGL(filter_count_kernel, dim3((unsigned)nblocks),
            dim3(FILTER_BLOCK), 0, cur_stream(),
            (const long long*)keys.data_ptr(),
            (const long long*)vals.data_ptr(), n, p,
            counts.data_ptr<int>());
    return counts;
}

// block_off: exclusive i64 scan of filter_count's result for the same
// columns and program; out_k/out_v hold exactly the survivor total.
void filter_scatter(torch::Tensor keys, torch::Tensor vals,
                    std::vector<int64_t> prog, torch::Tensor block_off,
                    torch::Tensor out_k, torch::Tensor out_v) {
    const long n = check_columns(keys, vals);
    const FilterProgram p = make_program(prog, vals);
    const long nblocks = (n + FILTER_TILE - 1) / FILTER_TILE;
    TORCH_CHECK(block_off.is_cuda() && block_off.dtype() == torch::kInt64 &&
                block_off.is_contiguous() && block_off.numel() == nblocks,
                "block_off: contiguous i64 device tensor, one per tile");
    TORCH_CHECK(is_col(out_k) && out_k.dtype() == torch::kInt64,
                "out_k: contiguous i64 device tensor");
    TORCH_CHECK(is_col(out_v) && out_v.dtype() == vals.dtype() &&
                out_v.numel() == out_k.numel(),
                "out_v: contiguous device tensor of vals' dtype and out_k's "
                "length");
    if (nblocks == 0 || out_k.numel() == 0) return;
    hipLaunchKernelGGL(filter_scatter_kernel, dim3((unsigned)nblocks),
        dim3(FILTER_BLOCK), 0, cur_stream(),
        (const long long*)keys.data_ptr(),
        (const long long*)vals.data_ptr(), n, p,
        block_off.data_ptr<long>(), (long long*)out_k.data_ptr(),
        (long long*)out_v.data_ptr(), (long)out_k.numel());
}
