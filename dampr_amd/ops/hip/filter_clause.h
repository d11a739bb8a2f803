// The clause encoding the row filters share (dampr_filter.hip over numeric
// value columns, dampr_strfilter.hip over var-len string value columns).
#pragma once

#include "common.h"
#include "host.h"

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

struct FilterClause {
    int col;           // 0: key column, 1: value column
    int dom;
    int op;
    int pad_;
    long long a;       // constant(s): i64, or the bits of a double; FD_STR:
    long long b;       // the constants' byte lengths
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
// has no FD_F64 domain, so the program need not be asked.
template <bool KEY = false>
__device__ __forceinline__ bool filter_clause_num(const FilterClause& c,
                                                  long long raw) {
    if (c.dom == FD_I64) return filter_cmp<long long>(c.op, raw, c.a, c.b);
    const long long bits =
        (KEY || c.dom == FD_FKEY) ? fkey_decode_bits(raw) : raw;
    return filter_cmp<double>(c.op, __longlong_as_double(bits),
                              __longlong_as_double(c.a),
                              __longlong_as_double(c.b));
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
        TORCH_CHECK(c[2] >= FO_GT && c[2] <= FO_STARTSWITH,
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
    }
    return n;
}
