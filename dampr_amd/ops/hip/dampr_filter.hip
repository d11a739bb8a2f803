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
#include "ops.h"

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
// ``sets``: the tables of the program's set clauses, by column; has_set:
// whether it holds any.
FilterProgram make_program(Args& a, const std::vector<int64_t>& prog,
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
            filter_take_set(a, c.col ? set_v : set_k, c.col, c.a, sets);
            *has_set = true;
        }
    }
    return p;
}

// The (key, value) column pair both passes read, and its tiling.
struct Columns {
    const long long *keys, *vals;
    long n, nblocks;
    Columns(Args& a, const torch::Tensor& k, const torch::Tensor& v) {
        n = k.numel();
        keys = a.dev<const long long>(k, "keys");
        vals = a.col(v, "vals", n);
        TORCH_CHECK(n < (1L << 31), "keys: row count exceeds i32");
        nblocks = tiles_for(n, COMPACT_TILE);
    }
};
}  // namespace

long filter_tile() { return COMPACT_TILE; }

// Survivors per tile of COMPACT_TILE rows: i32[ceil(n / COMPACT_TILE)].
torch::Tensor filter_count(torch::Tensor keys, torch::Tensor vals,
                           std::vector<int64_t> prog,
                           c10::optional<torch::Tensor> set_k,
                           c10::optional<torch::Tensor> set_v) {
    Args a;
    const Columns c(a, keys, vals);
    FilterSets sets;
    bool has_set;
    const FilterProgram p =
        make_program(a, prog, vals, set_k, set_v, &sets, &has_set);
    auto counts = torch::empty({c.nblocks}, like(keys, torch::kInt32));
    if (c.nblocks > 0)
        hipLaunchKernelGGL(
            has_set ? filter_count_kernel<true> : filter_count_kernel<false>,
            dim3((unsigned)c.nblocks), dim3(COMPACT_BLOCK), 0, a.stream(),
            c.keys, c.vals, c.n, p, sets, a.dev<int>(counts, "counts"));
    return counts;
}

// block_off: exclusive i64 scan of filter_count's result for the same
// columns and program; out_k/out_v hold exactly the survivor total.
void filter_scatter(torch::Tensor keys, torch::Tensor vals,
                    std::vector<int64_t> prog, torch::Tensor block_off,
                    torch::Tensor out_k, torch::Tensor out_v,
                    c10::optional<torch::Tensor> set_k,
                    c10::optional<torch::Tensor> set_v) {
    Args a;
    const Columns c(a, keys, vals);
    FilterSets sets;
    bool has_set;
    const FilterProgram p =
        make_program(a, prog, vals, set_k, set_v, &sets, &has_set);
    const long* off = a.dev<const long>(block_off, "block_off", c.nblocks);
    long long* ok = a.dev<long long>(out_k, "out_k");
    long long* ov = a.col(out_v, "out_v", out_k.numel());
    TORCH_CHECK(out_v.dtype() == vals.dtype(),
                "out_v: expected vals' dtype");
    if (c.nblocks == 0 || out_k.numel() == 0) return;
    hipLaunchKernelGGL(
        has_set ? filter_scatter_kernel<true> : filter_scatter_kernel<false>,
        dim3((unsigned)c.nblocks), dim3(COMPACT_BLOCK), 0, a.stream(),
        c.keys, c.vals, c.n, p, sets, off, ok, ov, (long)out_k.numel());
}

long set_capacity(long m) {
    TORCH_CHECK(m >= 0 && m <= SET_MAX_MEMBERS, "m: a set of 0..2**30 members");
    return set_capacity_for(m);
}

// The members' non-zero words into ``table``, which the caller zeroed:
// a power of two of at least set_capacity(m) words.
void set_build(torch::Tensor members, torch::Tensor table) {
    Args a;
    const u64* mem = a.dev<const u64>(members, "members");
    const long m = members.numel();
    TORCH_CHECK(m <= SET_MAX_MEMBERS, "members: more than 2**30 members");
    u64 mask;
    u64* tab = a.table(table, "table", &mask, set_capacity_for(m));
    if (m == 0) return;
    hipLaunchKernelGGL(set_build_kernel, dim3(grid_for(m)), dim3(256), 0,
        a.stream(), mem, m, tab, mask);
}
