// The clause encoding the row filters share (dampr_filter.hip over numeric
// value columns, dampr_strfilter.hip over var-len string value columns).
#pragma once

#include "common.h"

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
