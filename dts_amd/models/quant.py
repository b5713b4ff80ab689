"""Opt-in weight-only quantisation of the Llama projections: FP8 (OCP
e4m3fn, per-row scales) or MXFP4 (OCP e2m1 in blocks of 32 with e8m0
scales). The FP8 design is described first; MXFP4 follows it point for point
(see the MXFP4 section below).

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


# ---------------------------------------------------------------------------
# MXFP4: e2m1 elements, blocks of 32 along K, one e8m0 scale byte per block
# ---------------------------------------------------------------------------
# ``weight_q`` is uint8 [N, K/2] (element 2i in the low nibble of byte i,
# 2i+1 in the high nibble: the float4_e2m1fn_x2 convention) and
# ``weight_scale`` uint8 [N, K/32] (e8m0: 2^(b-127)). A block scale is a
# power of two by definition and an e2m1 value has two significant bits, so
# code * scale is exactly a bf16 value: as for FP8, both copies hold the SAME
# matrix. Cost: 1.25x weight memory for the quantised projections. On randn
# weights the relative Frobenius error is 0.115 (FP8: 0.027); no accuracy
# evaluation on trained weights exists.

E2M1_MAX = 6.0
MX_BLOCK = 32
# 2 * |value| -> code; the grid is {0, .5, 1, 1.5, 2, 3, 4, 6}
_E2M1_CODE_OF_TWICE = (0, 1, 2, 3, 4, 0, 5, 0, 6, 0, 0, 0, 7)


def quantize_mxfp4_rowwise(w: torch.Tensor) -> tuple:
    """[N, K] float weight, K % 32 == 0 -> (w_q uint8 [N, K/2], scale uint8
    [N, K/32]) with block scale 2^ceil(log2(amax_block / 6)), exponent
    clamped to [-125, 125] (0.5 * scale stays a normal bf16, 6 * scale
    finite; byte 0xFF, the e8m0 NaN, is never emitted); an all-zero block
    gets 2^0. Elements round to nearest, ties to the even mantissa bit."""
    assert w.dim() == 2 and w.shape[1] % MX_BLOCK == 0, w.shape
    N, K = w.shape
    wf = w.detach().float().view(N, K // MX_BLOCK, MX_BLOCK)
    amax = wf.abs().amax(dim=2)
    # same integer exponent arithmetic as quantize_fp8_rowwise
    m, e = torch.frexp(amax / E2M1_MAX)
    e = torch.where(m == 0.5, e - 1, e).clamp_(-125, 125)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    v = (wf.abs() / torch.ldexp(torch.ones_like(amax), e)[:, :, None]).clamp_(max=E2M1_MAX)
    # the grid's step is 0.5 below 2, 1 below 4, 2 above; torch.round is
    # half-to-even, and an even multiple of the step is the even mantissa
    step = torch.where(v < 2, 0.5, torch.where(v < 4, 1.0, 2.0))
    q = torch.round(v / step) * step
    lut = torch.tensor(_E2M1_CODE_OF_TWICE, dtype=torch.uint8, device=w.device)
    code = lut[(q * 2).long()] | (((wf < 0) & (q > 0)).to(torch.uint8) << 3)
    code = code.view(N, K // 2, 2)
    w_q = code[:, :, 0] | (code[:, :, 1] << 4)
    return w_q.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4(w_q: torch.Tensor, scale: torch.Tensor, dtype) -> torch.Tensor:
    from dts_amd.ops import torch_ref

    return torch_ref.dequantize_mxfp4(w_q, scale, dtype)


_MODES = {
    # mode: (quantiser, dequantiser)
    "fp8": (quantize_fp8_rowwise, dequantize_fp8_rowwise),
    "mxfp4": (quantize_mxfp4_rowwise, dequantize_mxfp4),
}


def quantized_linears(model):
    """The four per-layer projections of a LlamaModel, in layer order."""
    for layer in model.layers:
        yield layer.attn.qkv_proj
        yield layer.attn.o_proj
        yield layer.mlp.gate_up_proj
        yield layer.mlp.down_proj


def quantize_model_(model, mode: str = "fp8"):
    """Quantise a LlamaModel in place ("fp8" or "mxfp4") after its weights
    are loaded or random-initialised. lm_head and embed stay in the model
    dtype (about 1 GB of 16 for Llama-3-8B, and the logits are the most
    sensitive part). The linears tell the two formats apart by the dtype
    of weight_q (float8_e4m3fn / uint8)."""
    if mode not in _MODES:
        raise ValueError(
            f"unknown weight quantisation {mode!r} (supported: 'fp8', 'mxfp4')"
        )
    if getattr(model, "arch", None) != "llama":
        raise NotImplementedError(
            f"{mode} weight quantisation covers the Llama family only, not "
            f"{getattr(model, 'arch', type(model).__name__)!r}"
        )
    if model.tp.size > 1:
        raise NotImplementedError(
            f"{mode} weight quantisation with tensor parallelism (tp.size > 1) "
            "is not implemented"
        )
    quantize, dequantize = _MODES[mode]
    with torch.no_grad():
        for lin in quantized_linears(model):
            w_q, scale = quantize(lin.weight)
            lin.register_buffer("weight_q", w_q, persistent=False)
            lin.register_buffer("weight_scale", scale, persistent=False)
            # in place, so existing references to the parameter stay valid
            lin.weight.copy_(dequantize(w_q, scale, lin.weight.dtype))
    model.weight_quant = mode
    return model
