// String row filter for the dampr_amd device engine (gfx950): compact.h's
// stable two-pass stream compaction over a (key i64, value StrVals) column
// pair.  The program is a conjunction of at most FILTER_MAX_CLAUSES
// clauses: the numeric i64 / fkey clauses on the key column, and FD_STR
// clauses on the value column that compare a row's bytes against constants
// (gt/ge/lt/le/eq/ne/between/startswith).
//
//   sv_filter_count    the count pass over svf_row; alone, the sum of its
//                      result is "how many rows satisfy the program" (keys
//                      may be absent then)
//   sv_filter_scatter  the scatter pass, predicate re-evaluated; survivor o
//                      gets its key and its row's (source offset, length)
//                      in the arena
//   (host glue)        scan of the lengths, varlen_gather moves the bytes
//
// Order: unsigned bytes, a proper prefix is smaller, NUL is an ordinary byte
// (_OpsBase.str_rank's order).  Row and constant are cut into 8-byte words,
// zero-padded and byte-swapped so that byte 0 is the most significant; the
// first differing word decides, and when all ceil(|c| / 8) words agree the
// longer string is the larger one.  That is exact: a padded byte is 0, so a
// difference against padding makes the padded side, a proper prefix of the
// other, the smaller; and two strings whose padded words all agree differ
// only by trailing NULs (or by bytes of the row past the constant's last
// word), where length decides.
//
// Lane mapping: one lane per row.  The verdict against a constant c needs
// the row's first ceil(|c| / 8) words and its length, whatever the row's
// length, so the word loop's trip count (max_words, the longest constant of
// the program) is uniform over the grid and every lane does the same work;
// lane groups per row (sv_hash64) would idle on it.  Neighbouring lanes
// read neighbouring rows, which are neighbours in the arena.  A row word is
// loaded once and tested against every string clause.
//
// Constants: lengths travel in the by-value program, read with constant
// indices (the clause loop is fully unrolled; see dampr_filter.hip on why).
// The pre-swapped words sit in a small device buffer, slot 2 * clause (+ 1
// for between's upper end) of SVF_CONST_WORDS words, indexed by the word
// loop's counter: a wave-uniform address, so a scalar load, where the same
// dynamic index into a kernarg struct would copy it to scratch.
//
// Set membership (FO_ISIN / FO_NOTIN): a key clause probes the key
// column's numeric set as in dampr_filter.hip; an FD_STR clause probes a
// string set (set_table.h) by the row's hash.  The row hashes come from one
// sv_hash64 launch per run, read by both passes: that kernel spreads a
// row's whole length over an 8-lane group, which one lane per row cannot do
// without divergence.  Only a row whose hash equals a member's walks its
// bytes.  The kernels are instantiated on HAS_SET and the program selects
// the instantiation.
//
//   sv_set_build    grid-stride insert of the member indices into a zeroed
//                   slot table, once per filter stage
#include <hip/hip_runtime.h>
#include "host.h"
#include "ops.h"

#include "common.h"
#include "compact.h"
#include "filter_clause.h"
#include "sv_arena.h"

#define SVF_MAX_CONST 64                       // bytes per constant
#define SVF_CONST_WORDS (SVF_MAX_CONST / 8)
#define SVF_CONSTS_LEN (2 * FILTER_MAX_CLAUSES * SVF_CONST_WORDS)

struct SvProgram {
    int n;
    int need_k;        // some clause reads the key column
    int max_words;     // ceil(longest constant / 8)
    int pad_;
    FilterClause c[FILTER_MAX_CLAUSES];
};

// What the program's set clauses probe: the key column's numeric set, the
// value column's string set.
struct SvSets {
    const u64* ktab;
    u64 kmask;
    SvSet sv;
};

__device__ __forceinline__ int svf_sign(long d) {
    return (d > 0) - (d < 0);
}

// Does row r (of n) survive?  Also hands back its clamped arena range.
template <bool HAS_SET>
__device__ __forceinline__ bool svf_row(const SvProgram& prog,
                                        const SvSets& sets,
                                        const u64* __restrict__ consts,
                                        const long long* __restrict__ keys,
                                        const u8* __restrict__ blob,
                                        long blob_n,
                                        const long* __restrict__ offs,
                                        long r, long n, long* row_b,
                                        long* row_len) {
    const bool valid = r < n;
    bool keep = valid;
    long b = 0, len = 0;
    if (valid) sv_row(offs, r, blob_n, &b, &len);
    *row_b = b;
    *row_len = len;
    if (prog.need_k) {
        const long long k = valid ? keys[r] : 0;
#pragma unroll
        for (int i = 0; i < FILTER_MAX_CLAUSES; ++i) {
            if (i < prog.n && prog.c[i].col == 0) {
                const bool t = filter_clause_num<true, HAS_SET>(
                    prog.c[i], k, sets.ktab, sets.kmask);
                keep = keep && t;
            }
        }
    }
    // per string clause: order against a (ca) and b (cb) so far, 0 while
    // every word agreed; pre: a's bytes matched so far
    int ca[FILTER_MAX_CLAUSES], cb[FILTER_MAX_CLAUSES];
    bool pre[FILTER_MAX_CLAUSES];
#pragma unroll
    for (int i = 0; i < FILTER_MAX_CLAUSES; ++i) {
        ca[i] = 0;
        cb[i] = 0;
        pre[i] = true;
    }
    const u8* end = blob + blob_n;
#pragma unroll 1
    for (int j = 0; j < prog.max_words; ++j) {
        const long rem = len - 8L * j;
        u64 w = 0;
        if (rem > 0)
            w = __builtin_bswap64(sv_load_word(
                blob + b + 8L * j, rem < 8 ? (int)rem : 8, blob, end));
#pragma unroll
        for (int i = 0; i < FILTER_MAX_CLAUSES; ++i) {
            if (i < prog.n && prog.c[i].col == 1) {
                const int la = (int)prog.c[i].a - 8 * j;   // bytes of a left
                if (la > 0) {
                    const u64 cw = consts[2 * i * SVF_CONST_WORDS + j];
                    if (ca[i] == 0 && w != cw) ca[i] = w < cw ? -1 : 1;
                    const u64 m = la >= 8 ? ~0ULL : ~(~0ULL >> (8 * la));
                    pre[i] = pre[i] && ((w ^ cw) & m) == 0;
                }
                const int lb = (int)prog.c[i].b - 8 * j;
                if (prog.c[i].op == FO_BETWEEN && lb > 0) {
                    const u64 cw =
                        consts[(2 * i + 1) * SVF_CONST_WORDS + j];
                    if (cb[i] == 0 && w != cw) cb[i] = w < cw ? -1 : 1;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < FILTER_MAX_CLAUSES; ++i) {
        if (i < prog.n && prog.c[i].col == 1) {
            const int op = prog.c[i].op;
            const int ra = ca[i] ? ca[i] : svf_sign(len - prog.c[i].a);
            bool t;
            if (HAS_SET && op >= FO_ISIN) {
                // keep: the row is valid, and the probe is spared for a
                // row that another clause already dropped
                t = keep && sv_set_has(sets.sv, sets.sv.row_hash[r], blob,
                                       end, b, len) == (op == FO_ISIN);
            } else if (op == FO_STARTSWITH) {
                t = pre[i] && len >= prog.c[i].a;
            } else if (op == FO_BETWEEN) {
                const int rb = cb[i] ? cb[i] : svf_sign(len - prog.c[i].b);
                t = ra >= 0 && rb <= 0;
            } else {
                t = filter_cmp<int>(op, ra, 0, 0);
            }
            keep = keep && t;
        }
    }
    return keep;
}

template <bool HAS_SET>
__global__ void __launch_bounds__(COMPACT_BLOCK)
sv_filter_count_kernel(const long long* __restrict__ keys,
                       const u8* __restrict__ blob, long blob_n,
                       const long* __restrict__ offs, long n, SvProgram prog,
                       SvSets sets, const u64* __restrict__ consts,
                       int* __restrict__ block_counts) {
    const long base = compact_first_row();
    int cnt = 0;
#pragma unroll 1
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        long b, len;
        const bool p = svf_row<HAS_SET>(prog, sets, consts, keys, blob,
                                        blob_n, offs, base + (long)s * WAVE,
                                        n, &b, &len);
        cnt += __popcll(__ballot(p));
    }
    compact_store_total(compact_wave_counts(cnt), block_counts);
}

template <bool HAS_SET>
__global__ void __launch_bounds__(COMPACT_BLOCK)
sv_filter_scatter_kernel(const long long* __restrict__ keys,
                         const u8* __restrict__ blob, long blob_n,
                         const long* __restrict__ offs, long n,
                         SvProgram prog, SvSets sets,
                         const u64* __restrict__ consts,
                         const long* __restrict__ block_off,
                         long long* __restrict__ out_k,
                         long* __restrict__ out_src,
                         long* __restrict__ out_len, long n_out) {
    const long base = compact_first_row();
    // The strip loop is not unrolled (its body is the whole clause
    // program), so the pass's ballots wait in LDS, not in registers that a
    // dynamic index would turn into scratch.
    __shared__ u64 strip_bal[COMPACT_WAVES][COMPACT_STRIPS];
    int cnt = 0;
#pragma unroll 1
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        long b, len;
        const bool p = svf_row<HAS_SET>(prog, sets, consts, keys, blob,
                                        blob_n, offs, base + (long)s * WAVE,
                                        n, &b, &len);
        const u64 bal = __ballot(p);
        if (compact_lane() == 0) strip_bal[compact_wave()][s] = bal;
        cnt += __popcll(bal);
    }
    long pos = compact_wave_pos(compact_wave_counts(cnt), block_off);
#pragma unroll 1
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        const long r = base + (long)s * WAVE;
        pos = compact_emit(strip_bal[compact_wave()][s], pos, n_out,
                           [&](long o) {                // r < n: it survived
            long b, len;
            sv_row(offs, r, blob_n, &b, &len);
            out_k[o] = keys[r];
            out_src[o] = b;
            out_len[o] = len;
        });
    }
}

__global__ void sv_set_build_kernel(const u64* __restrict__ hashes, long m,
                                    int* __restrict__ slots, u64 mask) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += stride)
        sv_set_insert(slots, mask, hashes[i], i);
}

namespace {
// For an FD_STR clause a and b are the byte lengths of its constants, whose
// words are in ``consts``.
// ``sets``: what the program's set clauses probe; has_set: whether it
// holds any.  ``sv_set`` is empty, or the string set's (member blob,
// member offs, member hashes, slot table, row hashes).
SvProgram make_program(Args& a, const std::vector<int64_t>& prog,
                       const c10::optional<torch::Tensor>& set_k,
                       const std::vector<torch::Tensor>& sv_set, long n,
                       SvSets* sets, bool* has_set) {
    SvProgram p = {};
    *sets = SvSets{};
    *has_set = false;
    p.n = filter_parse_clauses(prog, p.c);
    for (int i = 0; i < p.n; ++i) {
        const FilterClause& c = p.c[i];
        if (c.col == 0) {
            p.need_k = 1;
            if (filter_is_set_op(c.op)) {
                FilterSets ks = {};
                filter_take_set(a, set_k, 0, c.a, &ks);
                sets->ktab = ks.tab[0];
                sets->kmask = ks.mask[0];
                *has_set = true;
            }
            continue;
        }
        TORCH_CHECK(c.dom == FD_STR,
                    "sv_filter clause: the value column is str");
        if (filter_is_set_op(c.op)) {
            TORCH_CHECK(sv_set.size() == 5,
                        "sv_filter clause: a str set clause, no set given");
            SvSet& sv = sets->sv;
            sv.blob = a.dev<const u8>(sv_set[0], "sv_set[0] (member blob)");
            sv.blob_n = sv_set[0].numel();
            sv.offs = a.dev_min<const long>(sv_set[1],
                                            "sv_set[1] (member offs)", 1);
            sv.m = sv_set[1].numel() - 1;
            sv.hashes = a.dev<const u64>(sv_set[2],
                                         "sv_set[2] (member hashes)", sv.m);
            sv.slots = a.table<const int>(sv_set[3], "sv_set[3] (slot table)",
                                          &sv.mask, set_capacity_for(sv.m));
            sv.row_hash = a.dev<const u64>(sv_set[4],
                                           "sv_set[4] (row hashes)", n);
            *has_set = true;
            continue;
        }
        TORCH_CHECK(c.a >= 0 && c.a <= SVF_MAX_CONST && c.b >= 0 &&
                    c.b <= SVF_MAX_CONST,
                    "sv_filter clause: constant longer than ",
                    SVF_MAX_CONST, " bytes");
        const long long longest =
            c.op == FO_BETWEEN ? std::max(c.a, c.b) : c.a;
        p.max_words = std::max(p.max_words, (int)((longest + 7) / 8));
    }
    return p;
}

// The columns both passes read (``keys`` may be absent when no clause
// reads it and the caller wants no keys back), the program and its tiling.
struct SvInputs {
    const long long* keys = nullptr;
    const u8* blob;
    const long* offs;
    const u64* consts;
    long blob_n, n, nblocks;
    SvProgram prog;
    SvSets sets;
    bool has_set;
    SvInputs(Args& a, const c10::optional<torch::Tensor>& k,
             const torch::Tensor& b, const torch::Tensor& o,
             const std::vector<int64_t>& pr, const torch::Tensor& cs,
             const c10::optional<torch::Tensor>& set_k,
             const std::vector<torch::Tensor>& sv_set, bool want_keys) {
        blob = a.dev<const u8>(b, "blob");
        blob_n = b.numel();
        offs = a.dev_min<const long>(o, "offs", 1);
        n = o.numel() - 1;
        TORCH_CHECK(n < (1L << 31), "offs: row count exceeds i32");
        prog = make_program(a, pr, set_k, sv_set, n, &sets, &has_set);
        consts = a.dev<const u64>(cs, "consts", SVF_CONSTS_LEN);
        if (k.has_value()) keys = a.dev<const long long>(*k, "keys", n);
        TORCH_CHECK(k.has_value() || !(want_keys || prog.need_k),
                    "keys: the program reads keys, none given");
        nblocks = tiles_for(n, COMPACT_TILE);
    }
};
}  // namespace

long sv_filter_tile() { return COMPACT_TILE; }
long sv_filter_max_const() { return SVF_MAX_CONST; }

// Survivors per tile of COMPACT_TILE rows: i32[ceil(n / COMPACT_TILE)].
torch::Tensor sv_filter_count(c10::optional<torch::Tensor> keys,
                              torch::Tensor blob, torch::Tensor offs,
                              std::vector<int64_t> prog,
                              torch::Tensor consts,
                              c10::optional<torch::Tensor> set_k,
                              std::vector<torch::Tensor> sv_set) {
    Args a;
    const SvInputs in(a, keys, blob, offs, prog, consts, set_k, sv_set,
                      false);
    auto counts = torch::empty({in.nblocks}, like(offs, torch::kInt32));
    if (in.nblocks > 0)
        hipLaunchKernelGGL(
            in.has_set ? sv_filter_count_kernel<true>
                       : sv_filter_count_kernel<false>,
            dim3((unsigned)in.nblocks), dim3(COMPACT_BLOCK), 0, a.stream(),
            in.keys, in.blob, in.blob_n, in.offs, in.n, in.prog, in.sets,
            in.consts, a.dev<int>(counts, "counts"));
    return counts;
}

// block_off: exclusive i64 scan of sv_filter_count's result for the same
// columns and program; the three outputs hold exactly the survivor total.
void sv_filter_scatter(torch::Tensor keys, torch::Tensor blob,
                       torch::Tensor offs, std::vector<int64_t> prog,
                       torch::Tensor consts, torch::Tensor block_off,
                       torch::Tensor out_k, torch::Tensor out_src,
                       torch::Tensor out_len,
                       c10::optional<torch::Tensor> set_k,
                       std::vector<torch::Tensor> sv_set) {
    Args a;
    const SvInputs in(a, keys, blob, offs, prog, consts, set_k, sv_set,
                      true);
    const long* off = a.dev<const long>(block_off, "block_off", in.nblocks);
    const long n_out = out_k.numel();
    long long* ok = a.dev<long long>(out_k, "out_k");
    long* os = a.dev<long>(out_src, "out_src", n_out);
    long* ol = a.dev<long>(out_len, "out_len", n_out);
    if (in.nblocks == 0 || n_out == 0) return;
    hipLaunchKernelGGL(
        in.has_set ? sv_filter_scatter_kernel<true>
                   : sv_filter_scatter_kernel<false>,
        dim3((unsigned)in.nblocks), dim3(COMPACT_BLOCK), 0, a.stream(),
        in.keys, in.blob, in.blob_n, in.offs, in.n, in.prog, in.sets,
        in.consts, off, ok, os, ol, n_out);
}

// Member indices into ``slots``, which the caller zeroed: i32, a power of
// two of at least set_capacity(m) slots.  ``hashes``: sv_hash64 of the
// members under the hash mask the rows will be hashed with.
void sv_set_build(torch::Tensor hashes, torch::Tensor slots) {
    Args a;
    const u64* h = a.dev<const u64>(hashes, "hashes");
    const long m = hashes.numel();
    TORCH_CHECK(m <= SET_MAX_MEMBERS, "hashes: more than 2**30 members");
    u64 mask;
    int* sl = a.table<int>(slots, "slots", &mask, set_capacity_for(m));
    if (m == 0) return;
    hipLaunchKernelGGL(sv_set_build_kernel, dim3(grid_for(m)), dim3(256),
        0, a.stream(), h, m, sl, mask);
}
