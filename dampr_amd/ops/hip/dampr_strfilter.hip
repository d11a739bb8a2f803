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
#include <hip/hip_runtime.h>
#include "host.h"

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

__device__ __forceinline__ int svf_sign(long d) {
    return (d > 0) - (d < 0);
}

// Does row r (of n) survive?  Also hands back its clamped arena range.
__device__ __forceinline__ bool svf_row(const SvProgram& prog,
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
                const bool t = filter_clause_num<true>(prog.c[i], k);
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
            if (op == FO_STARTSWITH) {
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

__global__ void __launch_bounds__(COMPACT_BLOCK)
sv_filter_count_kernel(const long long* __restrict__ keys,
                       const u8* __restrict__ blob, long blob_n,
                       const long* __restrict__ offs, long n, SvProgram prog,
                       const u64* __restrict__ consts,
                       int* __restrict__ block_counts) {
    const long base = compact_first_row();
    int cnt = 0;
#pragma unroll 1
    for (int s = 0; s < COMPACT_STRIPS; ++s) {
        long b, len;
        const bool p = svf_row(prog, consts, keys, blob, blob_n, offs,
                               base + (long)s * WAVE, n, &b, &len);
        cnt += __popcll(__ballot(p));
    }
    compact_store_total(compact_wave_counts(cnt), block_counts);
}

__global__ void __launch_bounds__(COMPACT_BLOCK)
sv_filter_scatter_kernel(const long long* __restrict__ keys,
                         const u8* __restrict__ blob, long blob_n,
                         const long* __restrict__ offs, long n,
                         SvProgram prog, const u64* __restrict__ consts,
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
        const bool p = svf_row(prog, consts, keys, blob, blob_n, offs,
                               base + (long)s * WAVE, n, &b, &len);
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

namespace {
// For an FD_STR clause a and b are the byte lengths of its constants, whose
// words are in ``consts``.
SvProgram make_program(const std::vector<int64_t>& prog) {
    SvProgram p = {};
    p.n = filter_parse_clauses(prog, p.c);
    for (int i = 0; i < p.n; ++i) {
        const FilterClause& c = p.c[i];
        if (c.col == 0) {
            p.need_k = 1;
            continue;
        }
        TORCH_CHECK(c.dom == FD_STR,
                    "sv_filter clause: the value column is str");
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

// Returns the row count.  ``keys`` may be absent when no clause reads it.
long check_inputs(const c10::optional<torch::Tensor>& keys,
                  const torch::Tensor& blob, const torch::Tensor& offs,
                  const torch::Tensor& consts, const SvProgram& p,
                  bool want_keys) {
    TORCH_CHECK(blob.is_cuda() && blob.dtype() == torch::kUInt8 &&
                blob.is_contiguous(), "blob: contiguous u8 device tensor");
    TORCH_CHECK(is_dev_i64(offs) && offs.numel() >= 1,
                "offs: contiguous i64 device tensor of n+1 entries");
    TORCH_CHECK(is_dev_i64(consts) && consts.numel() == SVF_CONSTS_LEN,
                "consts: contiguous i64 device tensor of ", SVF_CONSTS_LEN,
                " words");
    const long n = offs.numel() - 1;
    TORCH_CHECK(n < (1L << 31), "sv_filter: row count exceeds i32");
    if (keys.has_value())
        TORCH_CHECK(is_dev_i64(*keys) && keys->numel() == n,
                    "keys: contiguous i64 device tensor of n entries");
    TORCH_CHECK(keys.has_value() || !(want_keys || p.need_k),
                "sv_filter: the program reads keys, none given");
    return n;
}
}  // namespace

long sv_filter_tile() { return COMPACT_TILE; }
long sv_filter_max_const() { return SVF_MAX_CONST; }

// Survivors per tile of COMPACT_TILE rows: i32[ceil(n / COMPACT_TILE)].
torch::Tensor sv_filter_count(c10::optional<torch::Tensor> keys,
                              torch::Tensor blob, torch::Tensor offs,
                              std::vector<int64_t> prog,
                              torch::Tensor consts) {
    const SvProgram p = make_program(prog);
    const long n = check_inputs(keys, blob, offs, consts, p, false);
    const long nblocks = (n + COMPACT_TILE - 1) / COMPACT_TILE;
    auto counts = torch::empty({nblocks},
        torch::TensorOptions().dtype(torch::kInt32).device(offs.device()));
    if (nblocks > 0)
        hipLaunchKernelGGL(sv_filter_count_kernel, dim3((unsigned)nblocks),
            dim3(COMPACT_BLOCK), 0, cur_stream(),
            keys.has_value() ? (const long long*)keys->data_ptr() : nullptr,
            (const u8*)blob.data_ptr(), (long)blob.numel(),
            offs.data_ptr<long>(), n, p, (const u64*)consts.data_ptr(),
            counts.data_ptr<int>());
    return counts;
}

// block_off: exclusive i64 scan of sv_filter_count's result for the same
// columns and program; the three outputs hold exactly the survivor total.
void sv_filter_scatter(torch::Tensor keys, torch::Tensor blob,
                       torch::Tensor offs, std::vector<int64_t> prog,
                       torch::Tensor consts, torch::Tensor block_off,
                       torch::Tensor out_k, torch::Tensor out_src,
                       torch::Tensor out_len) {
    const SvProgram p = make_program(prog);
    const long n = check_inputs(keys, blob, offs, consts, p, true);
    const long nblocks = (n + COMPACT_TILE - 1) / COMPACT_TILE;
    TORCH_CHECK(is_dev_i64(block_off) && block_off.numel() == nblocks,
                "block_off: contiguous i64 device tensor, one per tile");
    TORCH_CHECK(is_dev_i64(out_k) && is_dev_i64(out_src) &&
                is_dev_i64(out_len) && out_src.numel() == out_k.numel() &&
                out_len.numel() == out_k.numel(),
                "out_k, out_src, out_len: contiguous i64 device tensors of "
                "one length");
    if (nblocks == 0 || out_k.numel() == 0) return;
    hipLaunchKernelGGL(sv_filter_scatter_kernel, dim3((unsigned)nblocks),
        dim3(COMPACT_BLOCK), 0, cur_stream(),
        (const long long*)keys.data_ptr(), (const u8*)blob.data_ptr(),
        (long)blob.numel(), offs.data_ptr<long>(), n, p,
        (const u64*)consts.data_ptr(), block_off.data_ptr<long>(),
        (long long*)out_k.data_ptr(), out_src.data_ptr<long>(),
        out_len.data_ptr<long>(), (long)out_k.numel());
}
