// Row filter for the dampr_amd device engine (gfx950): compact.h's stable
// two-pass stream compaction of a (key, value) column pair under a
// conjunction of at most FILTER_MAX_CLAUSES comparisons against constants.
//
//   filter_count    the count pass over filter_row
//   filter_scatter  the scatter pass, predicate re-evaluated (cheaper than a
//                   flag column: 2 x 8 B read per row instead of a 1 B write
//                   plus read and a second launch over it); a survivor's key
//                   and value words go to its slot
//
// Both strip loops are fully unrolled, so the scatter pass keeps its
// ballots in registers (constant indices).
//
// The clause program travels by value in the kernel arguments.  The clause
// loop is fully unrolled so every program access has a constant index and
// stays a scalar kernarg load (a dynamic index would copy the struct to
// scratch).  Both value dtypes (i64, f64) are 8 bytes, so columns move as
// raw 64-bit words and a clause's domain says how to read them.
//
// Set membership (FO_ISIN / FO_NOTIN) is one more case of the clause
// evaluator: a probe of the column's hash set (set_table.h), whose pointer
// and mask travel by value beside the clauses.  Both kernels are
// instantiated on HAS_SET and the program selects the instantiation, so a
// program without a set clause runs code without the probe.
//
//   set_build       grid-stride insert of the members' words into a zeroed
//                   table, once per filter stage
#include <hip/hip_runtime.h>
#include "host.h"

#include "common.h"
#include "compact.h"
#include "filter_clause.h"

struct FilterProgram {
    int n;
    int need_k;        // some clause reads the key column
    int need_v;
    int pad_;
    FilterClause c[FILTER_MAX_CLAUSES];
};

// Does row r (of n) survive?  Loads only the columns the program reads.
template <bool HAS_SET>
__device__ __forceinline__ bool filter_row(const FilterProgram& prog,
                                           const FilterSets& sets,
                                           const long long* __restrict__ keys,
                                           const long long* __restrict__ vals,
                                           long r, long n) {
    if (r >= n) return false;
    const long long k = prog.need_k ? keys[r] : 0;
    const long long v = prog.need_v ? vals[r] : 0;
    bool keep = true;
#pragma unroll
    for (int i = 0; i < FILTER_MAX_CLAUSES; ++i) {
        if (i < prog.n) {
            const int col = prog.c[i].col;
            const bool t = filter_clause_num<false, HAS_SET>(
                prog.c[i], col ? v : k, col ? sets.tab[1] : sets.tab[0],
                col ? sets.mask[1] : sets.mask[0]);
            keep = keep && t;
        }
    }
    return keep;
}

template <bool HAS_SET>
__global__ void __launch_bounds__(COMPACT_BLOCK)
filter_count_kernel(const long long* __restrict__ keys,
                    const long long* __restrict__ vals, long n,
                    FilterProgram prog, FilterSets sets,
                    int* __restrict__ block_counts) {
    const long base = compact_first_row();
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        const bool p = filter_row<HAS_SET>(prog, sets, keys, vals,
                                           base + (long)s * WAVE, n);
        cnt += __popcll(__ballot(p));
    }
    compact_store_total(compact_wave_counts(cnt), block_counts);
}

template <bool HAS_SET>
__global__ void __launch_bounds__(COMPACT_BLOCK)
filter_scatter_kernel(const long long* __restrict__ keys,
                      const long long* __restrict__ vals, long n,
                      FilterProgram prog, FilterSets sets,
                      const long* __restrict__ block_off,
                      long long* __restrict__ out_k,
                      long long* __restrict__ out_v, long n_out) {
    const long base = compact_first_row();
    u64 ballots[COMPACT_STRIPS];
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        const bool p = filter_row<HAS_SET>(prog, sets, keys, vals,
                                           base + (long)s * WAVE, n);
        ballots[s] = __ballot(p);
        cnt += __popcll(ballots[s]);
    }
    long pos = compact_wave_pos(compact_wave_counts(cnt), block_off);
#pragma unroll
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        pos = compact_emit(ballots[s], pos, n_out, [&](long o) {
            const long r = base + (long)s * WAVE;       // < n: it survived
            out_k[o] = keys[r];
            out_v[o] = vals[r];
        });
    }
}

__global__ void set_build_kernel(const u64* __restrict__ members, long m,
                                 u64* __restrict__ tab, u64 mask) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += stride) {
        const u64 w = members[i];
        if (w) set_insert_u64(tab, mask, w);    // 0 is the clause's flag
    }
}

namespace {
bool is_col(const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() &&
           (t.dtype() == torch::kInt64 || t.dtype() == torch::kFloat64);
}

// ``sets``: the tables of the program's set clauses, by column; has_set:
// whether it holds any.
FilterProgram make_program(const std::vector<int64_t>& prog,
                           const torch::Tensor& vals,
                           const c10::optional<torch::Tensor>& set_k,
                           const c10::optional<torch::Tensor>& set_v,
                           FilterSets* sets, bool* has_set) {
    FilterProgram p = {};
    *sets = FilterSets{};
    *has_set = false;
    p.n = filter_parse_clauses(prog, p.c);
    for (int i = 0; i < p.n; ++i) {
        const FilterClause& c = p.c[i];
        TORCH_CHECK(c.dom != FD_STR,
                    "filter clause: no str domain over numeric values");
        TORCH_CHECK(c.col == 0 ||
                    (c.dom == FD_F64) == (vals.dtype() == torch::kFloat64),
                    "filter clause: domain does not match the value dtype");
        if (c.col) p.need_v = 1; else p.need_k = 1;
        if (filter_is_set_op(c.op)) {
            filter_take_set(c.col ? set_v : set_k, c.col, c.a, sets);
            *has_set = true;
        }
    }
    return p;
}

long check_columns(const torch::Tensor& keys, const torch::Tensor& vals) {
    TORCH_CHECK(is_dev_i64(keys), "keys: contiguous i64 device tensor");
    TORCH_CHECK(is_col(vals) && vals.numel() == keys.numel(),
                "vals: contiguous i64/f64 device tensor of keys' length");
    const long n = keys.numel();
    TORCH_CHECK(n < (1L << 31), "filter: row count exceeds i32");
    return n;
}
}  // namespace

long filter_tile() { return COMPACT_TILE; }

// Survivors per tile of COMPACT_TILE rows: i32[ceil(n / COMPACT_TILE)].
torch::Tensor filter_count(torch::Tensor keys, torch::Tensor vals,
                           std::vector<int64_t> prog,
                           c10::optional<torch::Tensor> set_k,
                           c10::optional<torch::Tensor> set_v) {
    const long n = check_columns(keys, vals);
    FilterSets sets;
    bool has_set;
    const FilterProgram p =
        make_program(prog, vals, set_k, set_v, &sets, &has_set);
    const long nblocks = (n + COMPACT_TILE - 1) / COMPACT_TILE;
    auto counts = torch::empty({nblocks},
        torch::TensorOptions().dtype(torch::kInt32).device(keys.device()));
    if (nblocks > 0)
        hipLaunchKernelGGL(
            has_set ? filter_count_kernel<true> : filter_count_kernel<false>,
            dim3((unsigned)nblocks), dim3(COMPACT_BLOCK), 0, cur_stream(),
            (const long long*)keys.data_ptr(),
            (const long long*)vals.data_ptr(), n, p, sets,
            counts.data_ptr<int>());
    return counts;
}

// block_off: exclusive i64 scan of filter_count's result for the same
// columns and program; out_k/out_v hold exactly the survivor total.
void filter_scatter(torch::Tensor keys, torch::Tensor vals,
                    std::vector<int64_t> prog, torch::Tensor block_off,
                    torch::Tensor out_k, torch::Tensor out_v,
                    c10::optional<torch::Tensor> set_k,
                    c10::optional<torch::Tensor> set_v) {
    const long n = check_columns(keys, vals);
    FilterSets sets;
    bool has_set;
    const FilterProgram p =
        make_program(prog, vals, set_k, set_v, &sets, &has_set);
    const long nblocks = (n + COMPACT_TILE - 1) / COMPACT_TILE;
    TORCH_CHECK(is_dev_i64(block_off) && block_off.numel() == nblocks,
                "block_off: contiguous i64 device tensor, one per tile");
    TORCH_CHECK(is_dev_i64(out_k), "out_k: contiguous i64 device tensor");
    TORCH_CHECK(is_col(out_v) && out_v.dtype() == vals.dtype() &&
                out_v.numel() == out_k.numel(),
                "out_v: contiguous device tensor of vals' dtype and out_k's "
                "length");
    if (nblocks == 0 || out_k.numel() == 0) return;
    hipLaunchKernelGGL(
        has_set ? filter_scatter_kernel<true> : filter_scatter_kernel<false>,
        dim3((unsigned)nblocks), dim3(COMPACT_BLOCK), 0, cur_stream(),
        (const long long*)keys.data_ptr(),
        (const long long*)vals.data_ptr(), n, p, sets,
        block_off.data_ptr<long>(), (long long*)out_k.data_ptr(),
        (long long*)out_v.data_ptr(), (long)out_k.numel());
}

long set_capacity(long m) {
    TORCH_CHECK(m >= 0 && m <= SET_MAX_MEMBERS, "set: 0..2**30 members");
    return set_capacity_for(m);
}

// The members' non-zero words into ``table``, which the caller zeroed:
// a power of two of at least set_capacity(m) words.
void set_build(torch::Tensor members, torch::Tensor table) {
    TORCH_CHECK(is_dev_i64(members) && is_dev_i64(table),
                "members, table: contiguous i64 device tensors");
    const long m = members.numel(), cap = table.numel();
    TORCH_CHECK(m <= SET_MAX_MEMBERS, "set: more than 2**30 members");
    TORCH_CHECK((cap & (cap - 1)) == 0 && cap >= set_capacity_for(m),
                "table: a power of two of at least set_capacity(m) words");
    if (m == 0) return;
    const long grid = std::min<long>((m + 255) / 256, 4096);
    hipLaunchKernelGGL(set_build_kernel, dim3((unsigned)grid), dim3(256), 0,
        cur_stream(), (const u64*)members.data_ptr(), m,
        (u64*)table.data_ptr(), (u64)cap - 1);
}
