// The host layer every dampr_amd extension source shares: the launch
// stream, the grid size, and the checked accessors that turn a tensor
// argument into the typed pointer a kernel takes.  (They need ATen, so they
// stay out of the device headers; bindings.cpp does not include this file.)
// A .hip source still names <hip/hip_runtime.h> itself: torch's extension
// builder writes a patched copy of any kernel source that does not.
//
// A wrapper declares one `Args a;`, takes every pointer through a.dev /
// a.col / a.table and launches on a.stream().  No raw data_ptr cast, no
// longhand check: what the host knows without a device sync is checked
// here, and every message starts with the argument's parameter name.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"

inline int grid_for(long work, int block = 256, int cap = 4096) {
    long g = (work + block - 1) / block;
    return (int)std::min<long>(std::max<long>(g, 1), cap);
}

// Tiles of `span` elements that cover n.
inline long tiles_for(long n, long span) { return (n + span - 1) / span; }

// Options of a result of `dtype` on t's device.
inline torch::TensorOptions like(const torch::Tensor& t,
                                 at::ScalarType dtype) {
    return torch::TensorOptions().dtype(dtype).device(t.device());
}

// Is `s` what callers pass for a kernel parameter of element type T?  i64
// for the 64-bit integers (u64 words travel as i64), f64 for double, i32 for
// int, i32 or u32 for u32 (mark_counts returns u32, index columns are i32),
// u8 for bytes.
template <typename T>
inline bool dtype_fits(at::ScalarType s) {
    using U = std::remove_const_t<T>;
    if (std::is_floating_point<U>::value)
        return sizeof(U) == 8 && s == at::kDouble;
    if (sizeof(U) == 8) return s == at::kLong;
    if (sizeof(U) == 4)
        return s == at::kInt || (std::is_unsigned<U>::value &&
                                 s == at::kUInt32);
    return sizeof(U) == 1 && s == at::kByte;
}

template <typename T>
inline const char* dtype_name() {
    using U = std::remove_const_t<T>;
    return std::is_floating_point<U>::value ? "f64"
         : sizeof(U) == 8 ? "i64"
         : sizeof(U) == 4 ? (std::is_unsigned<U>::value ? "i32/u32" : "i32")
                          : "u8";
}

// The checked arguments of one wrapper call.  An argument's form (element
// type, contiguity, length) is checked where its pointer is taken; whether
// all of them live on the device is asked once, by stream(), so a malformed
// argument is reported by name before anything about devices, and a call
// that returns early on n == 0 launches nothing and asks nothing.  A
// contiguous view at a storage offset is as good as a whole tensor.
class Args {
  public:
    // Contiguous tensor of T; of exactly n entries where n >= 0.
    template <typename T>
    T* dev(const torch::Tensor& t, const char* name, long n = -1) {
        TORCH_CHECK(dtype_fits<T>(t.scalar_type()) && t.is_contiguous() &&
                    (n < 0 || t.numel() == n),
                    name, ": expected a contiguous ", dtype_name<T>(),
                    " tensor", of(n), ", got ", t.scalar_type(), "[",
                    t.numel(), "]", t.is_contiguous() ? "" : ", strided");
        note(t, name);
        return static_cast<T*>(t.data_ptr());
    }

    // As dev, of at least n entries.
    template <typename T>
    T* dev_min(const torch::Tensor& t, const char* name, long n) {
        TORCH_CHECK(t.numel() >= n, name, ": expected at least ", n,
                    " entries, got ", t.numel());
        return dev<T>(t, name);
    }

    // A value column: i64 or f64, moved as raw 64-bit words.
    long long* col(const torch::Tensor& t, const char* name, long n = -1) {
        return t.scalar_type() == at::kDouble
            ? reinterpret_cast<long long*>(dev<double>(t, name, n))
            : dev<long long>(t, name, n);
    }

    // An open-addressing table of T slots, a power of two of them and at
    // least `at_least`; *mask = slots - 1.
    template <typename T = u64>
    T* table(const torch::Tensor& t, const char* name, u64* mask,
             long at_least = 1) {
        const long cap = t.numel();
        TORCH_CHECK(cap >= at_least && (cap & (cap - 1)) == 0, name,
                    ": expected a table of a power of two of at least ",
                    at_least, " slots, got ", cap);
        *mask = (u64)cap - 1;
        return dev<T>(t, name);
    }

    // The launch stream; refuses when an argument is not a device tensor.
    hipStream_t stream() const {
        TORCH_CHECK(host_arg_ == nullptr, host_arg_,
                    ": expected a device tensor");
        return at::hip::getCurrentHIPStream().stream();
    }

  private:
    static std::string of(long n) {
        return n < 0 ? std::string()
                     : " of " + std::to_string(n) + " entries";
    }
    void note(const torch::Tensor& t, const char* name) {
        if (!t.is_cuda() && host_arg_ == nullptr) host_arg_ = name;
    }
    const char* host_arg_ = nullptr;
};

// Kernels read their inputs while they write their outputs.
inline void check_distinct(const torch::Tensor& out, const char* out_name,
                           const torch::Tensor& in, const char* in_name) {
    TORCH_CHECK(out.data_ptr() != in.data_ptr(), out_name,
                ": must not alias ", in_name);
}
