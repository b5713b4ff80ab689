"""Opt-in FP8 (OCP e4m3fn) weight-only quantisation of the Llama projections.

A quantised linear keeps TWO copies of its weight:

* ``weight_q`` [N, K] FP8 + ``weight_scale`` [N] fp32 — streamed by the
  W8A16 skinny GEMM for decode batches (M <= 16 on the GPU), half the bytes
  of the bf16 weight;
* the exact dequantised matrix, written IN PLACE over the existing
  ``weight`` parameter — used by everything else (prefill through hipBLASLt,
  CPU).

The per-row scale is a power of two, ``2^ceil(log2(amax / 448))``, so
``w_q.float() * scale`` has the 4 significant bits of an e4m3 value and is
exactly representable in bf16: both copies hold the SAME matrix, and a
quantised model is simply the bf16 model with those weights. The decode
kernel is an acceleration, not a second model. Restricting the scale to a
power of two costs nothing measurable (relative error 0.0266 against
0.0264 with free scales on randn weights).

Cost: 1.5x weight memory for the quantised projections. Dequantising into a
scratch buffer per prefill call instead is the route for models where that
does not fit (70B); see docs/ROADMAP.md.
"""

from __future__ import annotations

import torch

E4M3_MAX = 448.0
FP8_DTYPE = torch.float8_e4m3fn


def quantize_fp8_rowwise(w: torch.Tensor) -> tuple:
    """[N, K] float weight -> (w_q [N, K] float8_e4m3fn, scale [N] fp32)
    with scale[n] = 2^ceil(log2(amax[n] / 448)); an all-zero row gets 1."""
    assert w.dim() == 2, w.shape
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    # amax/448 = m * 2^e with m in [0.5, 1): ceil(log2) is e, or e-1 when
    # the ratio is itself a power of two. Integer exponent arithmetic, so
    # the scale is a power of two by construction, not by rounding luck.
    m, e = torch.frexp(amax / E4M3_MAX)
    e = torch.where(m == 0.5, e - 1, e).clamp_(min=-126)
    scale = torch.ldexp(torch.ones_like(amax), e)
    scale = torch.where(amax > 0, scale, torch.ones_like(scale))
    # dividing by a power of two is exact; the clamp keeps the cast away
    # from the NaN codes 0x7f / 0xff (e4m3fn has no infinities)
    w_q = (wf / scale[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(FP8_DTYPE)
    return w_q.contiguous(), scale.contiguous()


def dequantize_fp8_rowwise(w_q: torch.Tensor, scale: torch.Tensor, dtype) -> torch.Tensor:
    return (w_q.float() * scale[:, None]).to(dtype)


def quantized_linears(model):
    """The four per-layer projections of a LlamaModel, in layer order."""
    for layer in model.layers:
        yield layer.attn.qkv_proj
        yield layer.attn.o_proj
        yield layer.mlp.gate_up_proj
        yield layer.mlp.down_proj


def quantize_model_(model, mode: str = "fp8"):
    """Quantise a LlamaModel in place after its weights are loaded or
    random-initialised. lm_head and embed stay in the model dtype (about
    1 GB of 16 for Llama-3-8B, and the logits are the most sensitive part)."""
    if mode != "fp8":
        raise ValueError(f"unknown weight quantisation {mode!r} (supported: 'fp8')")
    if getattr(model, "arch", None) != "llama":
        raise NotImplementedError(
            "fp8 weight quantisation covers the Llama family only, not "
            f"{getattr(model, 'arch', type(model).__name__)!r}"
        )
    if model.tp.size > 1:
        raise NotImplementedError(
            "fp8 weight quantisation with tensor parallelism (tp.size > 1) "
            "is not implemented"
        )
    with torch.no_grad():
        for lin in quantized_linears(model):
            w_q, scale = quantize_fp8_rowwise(lin.weight)
            lin.register_buffer("weight_q", w_q, persistent=False)
            lin.register_buffer("weight_scale", scale, persistent=False)
            # in place, so existing references to the parameter stay valid
            lin.weight.copy_(dequantize_fp8_rowwise(w_q, scale, lin.weight.dtype))
    model.weight_quant = mode
    return model
