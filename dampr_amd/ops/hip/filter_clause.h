// The clause encoding the row filters share (dampr_filter.hip over numeric
// value columns, dampr_strfilter.hip over var-len string value columns).
#pragma once

#include "common.h"
#include "host.h"
#include "set_table.h"

#define FILTER_MAX_CLAUSES 8

// domains: how a clause reads its column
#define FD_I64 0       // 64-bit word as a signed integer
#define FD_F64 1       // 64-bit word as an IEEE double
#define FD_FKEY 2      // encode_f64_sortable(double): decode, then as FD_F64
#define FD_STR 3       // arena row as unsigned bytes (dampr_strfilter.hip)
// ops
#define FO_GT 0
#define FO_GE 1
#define FO_LT 2
#define FO_LE 3
#define FO_EQ 4
#define FO_NE 5
#define FO_BETWEEN 6   // a <= x && x <= b
#define FO_STARTSWITH 7   // FD_STR only: a is a prefix of x
#define FO_ISIN 8      // x is a member of its column's set (set_table.h)
#define FO_NOTIN 9

struct FilterClause {
    int col;           // 0: key column, 1: value column
    int dom;
    int op;
    int pad_;
    long long a;       // constant(s): i64, or the bits of a double; FD_STR:
    long long b;       // the constants' byte lengths.  FO_ISIN / FO_NOTIN
                       // over a numeric domain: a counts the non-zero
                       // members (the host sizes the table by it), b != 0
                       // says that the word 0 is a member; FD_STR: both 0
};

// The numeric set a column's FO_ISIN / FO_NOTIN clause probes: at most one
// per column, so the table travels beside the clauses, indexed by column.
struct FilterSets {
    const u64* tab[2];
    u64 mask[2];
};

template <typename T>
__device__ __forceinline__ bool filter_cmp(int op, T x, T a, T b) {
    switch (op) {
        case FO_GT: return x > a;
        case FO_GE: return x >= a;
        case FO_LT: return x < a;
        case FO_LE: return x <= a;
        case FO_EQ: return x == a;
        case FO_NE: return x != a;
        default:    return a <= x && x <= b;
    }
}

// The inverse of stores.encode_f64_sortable: two bit operations.
__device__ __forceinline__ long long fkey_decode_bits(long long e) {
    return e < 0 ? (e ^ (long long)0x8000000000000000ULL) : ~e;
}

// One numeric clause (FD_I64 / FD_F64 / FD_FKEY) over its column's raw
// 64-bit word.  KEY: the word is known to come from the key column, which
// has no FD_F64 domain, so the program need not be asked.  HAS_SET: the
// program holds a set clause, whose column's table is (tab, mask); a
// program without one is compiled without the probe.
template <bool KEY = false, bool HAS_SET = false>
__device__ __forceinline__ bool filter_clause_num(
        const FilterClause& c, long long raw,
        const u64* __restrict__ tab = nullptr, u64 mask = 0) {
    if (HAS_SET && c.op >= FO_ISIN) {
        u64 w = (u64)raw;
        bool hit = true;
        if (c.dom != FD_I64)
            hit = set_word_f64((KEY || c.dom == FD_FKEY)
                                   ? fkey_decode_bits(raw) : raw, &w);
        if (hit) hit = w ? set_has_u64(tab, mask, w) : c.b != 0;
        return hit == (c.op == FO_ISIN);
    }
    if (c.dom == FD_I64) return filter_cmp<long long>(c.op, raw, c.a, c.b);
    const long long bits =
        (KEY || c.dom == FD_FKEY) ? fkey_decode_bits(raw) : raw;
    return filter_cmp<double>(c.op, __longlong_as_double(bits),
                              __longlong_as_double(c.a),
                              __longlong_as_double(c.b));
}

inline bool filter_is_set_op(int op) {
    return op == FO_ISIN || op == FO_NOTIN;
}

// Host: column col's numeric set table for the kernels, checked.  A table
// is i64 words, a power of two of them, at least set_capacity_for(the
// clause's member count): half empty, so every probe meets an empty slot.
inline void filter_take_set(Args& a,
                            const c10::optional<torch::Tensor>& tab, int col,
                            long long members, FilterSets* sets) {
    TORCH_CHECK(tab.has_value(), "filter clause: a set clause on column ",
                col, ", no table given");
    TORCH_CHECK(members >= 0 && members <= SET_MAX_MEMBERS,
                "filter clause: a set of 0..2**30 members");
    sets->tab[col] = a.table<const u64>(*tab, col ? "set_v" : "set_k",
                                        &sets->mask[col],
                                        set_capacity_for((long)members));
}

// Host: the flat program, 5 int64 per clause (col, dom, op, a, b), into
// out[FILTER_MAX_CLAUSES]; returns the clause count.  Checks what holds for
// every filter; each filter adds what its value column requires.
inline int filter_parse_clauses(const std::vector<int64_t>& prog,
                                FilterClause* out) {
    TORCH_CHECK(prog.size() % 5 == 0 && prog.size() >= 5 &&
                prog.size() <= 5 * FILTER_MAX_CLAUSES,
                "filter program: 1..", FILTER_MAX_CLAUSES,
                " clauses of (col, dom, op, a, b)");
    const int n = (int)(prog.size() / 5);
    for (int i = 0; i < n; ++i) {
        const int64_t* c = &prog[5 * i];
        TORCH_CHECK(c[0] == 0 || c[0] == 1, "filter clause: col is 0 or 1");
        TORCH_CHECK(c[1] >= FD_I64 && c[1] <= FD_STR,
                    "filter clause: unknown domain");
        TORCH_CHECK(c[2] >= FO_GT && c[2] <= FO_NOTIN,
                    "filter clause: unknown op");
        TORCH_CHECK(c[1] == FD_STR || c[2] != FO_STARTSWITH,
                    "filter clause: startswith is a str op");
        // the key column is always i64 words: raw ints or encoded doubles
        TORCH_CHECK(c[0] == 1 || c[1] == FD_I64 || c[1] == FD_FKEY,
                    "filter clause: the key column is i64 or fkey");
        out[i].col = (int)c[0];
        out[i].dom = (int)c[1];
        out[i].op = (int)c[2];
        out[i].a = c[3];
        out[i].b = c[4];
        for (int j = 0; j < i; ++j)
            TORCH_CHECK(!(filter_is_set_op(out[i].op) &&
                          filter_is_set_op(out[j].op) &&
                          out[i].col == out[j].col),
                        "filter program: two set clauses on one column");
    }
    return n;
}
