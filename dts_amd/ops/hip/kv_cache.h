// Host-side dtype dispatch for the paged KV cache: bf16, or opt-in FP8
// (OCP e4m3fn codes, scale 1.0).
#pragma once

#include <torch/extension.h>

// true for an FP8 cache, false for a bf16 one. K and V of different dtypes,
// or any other dtype, is an error: the kernels reinterpret the pointers.
static inline bool kv_cache_is_fp8(const torch::Tensor& k_cache,
                                   const torch::Tensor& v_cache) {
  TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type(),
              "k_cache and v_cache must have the same dtype; got ",
              k_cache.scalar_type(), " and ", v_cache.scalar_type());
  const bool fp8 = k_cache.scalar_type() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || k_cache.scalar_type() == torch::kBFloat16,
              "KV cache must be bfloat16 or float8_e4m3fn; got ",
              k_cache.scalar_type());
  return fp8;
}
