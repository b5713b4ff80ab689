// Host-side dtype dispatch for the paged KV cache: bf16, or opt-in FP8
// (OCP e4m3fn codes, optionally with a power-of-two scale per kv-head).
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

// Optional per-head scales of an FP8 cache: fp32, contiguous [2, Hkv] on the
// cache's device (row 0 = K, row 1 = V). Returns the device pointer the
// kernels index by kv-head, or nullptr for None (scale 1.0). A scale tensor
// with a bf16 cache is an error: that cache has nothing to scale.
static inline const float* kv_scale_ptr(
    const c10::optional<torch::Tensor>& kv_scale, const torch::Tensor& k_cache,
    bool fp8) {
  if (!kv_scale.has_value()) return nullptr;
  const torch::Tensor& s = *kv_scale;
  TORCH_CHECK(fp8, "kv_scale needs an FP8 (float8_e4m3fn) KV cache; got ",
              k_cache.scalar_type());
  TORCH_CHECK(s.scalar_type() == torch::kFloat32,
              "kv_scale must be float32; got ", s.scalar_type());
  TORCH_CHECK(s.dim() == 2 && s.size(0) == 2 && s.size(1) == k_cache.size(1),
              "kv_scale must be [2, Hkv] = [2, ", k_cache.size(1), "]; got ",
              s.sizes());
  TORCH_CHECK(s.is_contiguous(), "kv_scale must be contiguous");
  TORCH_CHECK(s.device() == k_cache.device(),
              "kv_scale must be on the cache's device");
  return (const float*)s.data_ptr();
}
