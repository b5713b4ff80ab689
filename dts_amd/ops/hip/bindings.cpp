// Python bindings for the dts_amd MI355X kernels.
#include <torch/extension.h>

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor w, double eps);
void fused_add_rmsnorm(torch::Tensor x, torch::Tensor residual,
                       torch::Tensor w, double eps);
void silu_mul(torch::Tensor out, torch::Tensor in);
void layernorm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
               torch::Tensor b, double eps);
void rope_kv_append(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                    torch::Tensor positions, torch::Tensor cos_t,
                    torch::Tensor sin_t, torch::Tensor k_cache,
                    torch::Tensor v_cache, torch::Tensor slots,
                    c10::optional<torch::Tensor> kv_scale);
void kv_append(torch::Tensor k, torch::Tensor v, torch::Tensor k_cache,
               torch::Tensor v_cache, torch::Tensor slots,
               c10::optional<torch::Tensor> kv_scale);
void attn_decode_paged(torch::Tensor out, torch::Tensor q,
                       torch::Tensor kcache, torch::Tensor vcache,
                       torch::Tensor block_tables, torch::Tensor kv_lens,
                       double scale, c10::optional<torch::Tensor> kv_scale);
void attn_prefill_paged(torch::Tensor out, torch::Tensor q, torch::Tensor cu_q,
                        torch::Tensor q_pos, torch::Tensor kcache,
                        torch::Tensor vcache, torch::Tensor block_tables,
                        torch::Tensor kv_lens, double scale, int64_t swz,
                        c10::optional<torch::Tensor> kv_scale);
void top_p_sample(torch::Tensor out, torch::Tensor logits, torch::Tensor temps,
                  torch::Tensor top_ps, torch::Tensor seeds);
void derive_seeds(torch::Tensor out, torch::Tensor bases,
                  torch::Tensor positions);
void top_p_sample_v2(torch::Tensor out, torch::Tensor logits,
                     torch::Tensor temps, torch::Tensor top_ps,
                     torch::Tensor seeds, torch::Tensor ws_max,
                     torch::Tensor ws_bins, torch::Tensor ws_slice,
                     torch::Tensor ws_tau);
void sample_filtered(torch::Tensor out, torch::Tensor logits,
                     torch::Tensor temps, torch::Tensor top_ps,
                     torch::Tensor top_ks, torch::Tensor min_ps,
                     torch::Tensor seeds);
void sample_filtered_v2(torch::Tensor out, torch::Tensor logits,
                        torch::Tensor temps, torch::Tensor top_ps,
                        torch::Tensor top_ks, torch::Tensor min_ps,
                        torch::Tensor seeds, torch::Tensor ws_max,
                        torch::Tensor ws_bins, torch::Tensor ws_slice,
                        torch::Tensor ws_tau, torch::Tensor ws_cnt,
                        torch::Tensor ws_xk);
void gemv_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w);
void gemm_skinny_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                      int64_t tiles_per_wg, int64_t unroll);
void gemm_skinny_swiglu_bf16(torch::Tensor out, torch::Tensor x,
                             torch::Tensor w);
void moe_grouped_linear(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                        torch::Tensor counts, torch::Tensor offsets);
void gemm_skinny_w8_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w_q,
                         torch::Tensor scale, int64_t tiles_per_wg,
                         int64_t unroll);
void gemm_skinny_swiglu_w8_bf16(torch::Tensor out, torch::Tensor x,
                                torch::Tensor w_q, torch::Tensor scale);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &rmsnorm, "RMSNorm (bf16, CDNA4)");
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm,
        "fused residual add + RMSNorm (in-place, bf16)");
  m.def("silu_mul", &silu_mul, "SwiGLU activation (bf16)");
  m.def("layernorm", &layernorm, "LayerNorm (bf16, GPT-2 path)");
  m.def("rope_kv_append", &rope_kv_append,
        "fused rotate-half RoPE + paged KV append (bf16 q/k/v; bf16 or FP8 "
        "e4m3fn cache; kv_scale: optional fp32 [2, Hkv] power-of-two scales "
        "of an FP8 cache, row 0 = K, row 1 = V)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("positions"),
        py::arg("cos"), py::arg("sin"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("slots"),
        py::arg("kv_scale") = py::none());
  m.def("kv_append", &kv_append,
        "paged KV append without RoPE (bf16 k/v; bf16 or FP8 e4m3fn cache; "
        "kv_scale as for rope_kv_append)",
        py::arg("k"), py::arg("v"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("slots"), py::arg("kv_scale") = py::none());
  m.def("attn_decode_paged", &attn_decode_paged,
        "paged GQA decode attention (bf16 q/out, bf16 or FP8 e4m3fn cache; "
        "kv_scale as for rope_kv_append)",
        py::arg("out"), py::arg("q"), py::arg("kcache"), py::arg("vcache"),
        py::arg("block_tables"), py::arg("kv_lens"), py::arg("scale"),
        py::arg("kv_scale") = py::none());
  m.def("attn_prefill_paged", &attn_prefill_paged,
        "paged causal prefill attention (bf16 MFMA; bf16 or FP8 e4m3fn cache; "
        "kv_scale as for rope_kv_append)",
        py::arg("out"), py::arg("q"), py::arg("cu_q"), py::arg("q_pos"),
        py::arg("kcache"), py::arg("vcache"), py::arg("block_tables"),
        py::arg("kv_lens"),
        py::arg("scale"), py::arg("swz") = -1,
        py::arg("kv_scale") = py::none());
  m.def("top_p_sample", &top_p_sample,
        "fused temperature softmax + top-p sampling (sort-free)");
  m.def("derive_seeds", &derive_seeds,
        "stateless (seed, position) mix for chained decode");
  m.def("top_p_sample_v2", &top_p_sample_v2,
        "gridded top-p sampler (vocab sliced across workgroups)");
  m.def("sample_filtered", &sample_filtered,
        "top-k -> top-p -> min-p sampling, one workgroup per row");
  m.def("sample_filtered_v2", &sample_filtered_v2,
        "gridded top-k -> top-p -> min-p sampling (radix-select top-k)");
  m.def("gemv_bf16", &gemv_bf16,
        "skinny-batch (M<=8) bf16 weight-streaming GEMV");
  m.def("gemm_skinny_bf16", &gemm_skinny_bf16,
        "skinny-M (M<=16) bf16 MFMA weight-streaming GEMM; tiles_per_wg "
        "pins the N-tiles per workgroup (1/2/4), unroll the k-chunks in "
        "flight (4/8; 8 needs K % 1024 == 0); 0 = auto",
        py::arg("out"), py::arg("x"), py::arg("w"),
        py::arg("tiles_per_wg") = 0, py::arg("unroll") = 0);
  m.def("gemm_skinny_swiglu_bf16", &gemm_skinny_swiglu_bf16,
        "skinny-M gate_up GEMM with fused SwiGLU epilogue: "
        "out[M,I] = silu(x Wg^T) * (x Wu^T), w = [Wg; Wu]");
  m.def("moe_grouped_linear", &moe_grouped_linear,
        "grouped per-expert skinny GEMM (capture-safe MoE decode)");
  m.def("gemm_skinny_w8_bf16", &gemm_skinny_w8_bf16,
        "W8A16 skinny-M (M<=16) GEMM: FP8 e4m3fn weights [N,K] with an fp32 "
        "per-row scale [N], bf16 x/out, fp32 accumulation; tiles_per_wg and "
        "unroll as for gemm_skinny_bf16",
        py::arg("out"), py::arg("x"), py::arg("w_q"), py::arg("scale"),
        py::arg("tiles_per_wg") = 0, py::arg("unroll") = 0);
  m.def("gemm_skinny_swiglu_w8_bf16", &gemm_skinny_swiglu_w8_bf16,
        "W8A16 gate_up GEMM with fused SwiGLU epilogue: w_q = [Wg; Wu], "
        "gate rows scale by scale[n], up rows by scale[I+n]");
}
