// Host-side helpers every dampr_amd extension source shares (they need
// ATen, so they stay out of the device headers).  A .hip source still names
// <hip/hip_runtime.h> itself: torch's extension builder writes a patched
// copy of any kernel source that does not.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

inline hipStream_t cur_stream() {
    return at::hip::getCurrentHIPStream().stream();
}

inline bool is_dev_i64(const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() && t.dtype() == torch::kInt64;
}
