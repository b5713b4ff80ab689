"""Dense, per-sequence fp64 forward of Llama, Mixtral and GPT-2.

Written from the published definitions of the three architectures. A model
object is passed in only to read its parameters and its spec; none of the
project's forward code, ops, paging or batching is used. The single import
from the project is ``torch_ref.quantize_kv_fp8``, the written specification
of the FP8 KV store, which the kernel tests pin byte for byte.

Two modes run from the same code:

* ``exact`` (``mode=None``): fp64 throughout. This is THE forward.
* ``rounded(dtype)`` (``mode=torch.bfloat16`` / ``torch.float32``): every
  tensor the served model materialises in ``dtype`` is rounded to ``dtype``
  here as well (and kept in fp64 between those points). ``rounded - exact``
  is the reference's own measure of the noise the storage format causes;
  the tests bound a model's error by a multiple of it.

Rounding points modelled (read off the kernels, not guessed):

* embedding (sum), every norm output, every linear(+bias) output, the
  rotated q and k, the attention output, ``silu_mul`` / GELU output, every
  residual add (``fused_add_rmsnorm`` normalises the ROUNDED sum);
* prefill attention multiplies probabilities ROUNDED to ``dtype`` with V
  (MFMA) while the row sum is kept unrounded; decode attention keeps the
  probabilities in fp32. ``prefill_masks`` says which positions of a
  sequence went through prefill (default: all);
* MoE: the router reads the normalised activations in fp32 (no rounding of
  its logits); each expert's gate_up, ``silu_mul`` and down outputs are
  rounded, the weighted sum over the top-k is rounded once;
* dot products accumulate in fp32. Against bf16 storage that is 2^16 times
  finer than the rounding of the result and is left out; against fp32
  storage (the CPU tests) it is the dominant rounding point and is
  modelled as one fp32 accumulator per output element (``_Rounder.mm``);
* FP8 KV cache (``kv_scales`` given): K after RoPE and V are stored as
  ``quantize_kv_fp8(x, scale)`` and read back as ``code * scale``, in
  ``rounded`` mode only. ``exact`` never quantises.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from dts_amd.ops.torch_ref import quantize_kv_fp8

F64 = torch.float64


def _p(t) -> torch.Tensor:
    return t.detach().to("cpu").to(F64)


class _Rounder:
    def __init__(self, mode: Optional[torch.dtype]):
        self.mode = mode

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if self.mode is None:
            return x
        return x.to(self.mode).to(F64)

    def mm(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """x [T, K] @ w [N, K]^T, unrounded output. Dot products accumulate
        in fp32 everywhere. Under bf16 storage that accumulator is 2^16
        times finer than the rounding of the result and is not modelled;
        under fp32 storage it IS the dominant rounding point, so it is
        modelled the way a CPU GEMM micro-kernel works: one fp32
        accumulator per output element, one product added per k."""
        if self.mode is not torch.float32:
            return x @ w.T
        xf, wt = x.to(torch.float32), w.to(torch.float32).T.contiguous()
        acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
        for k in range(x.shape[1]):
            acc.addcmul_(xf[:, k : k + 1], wt[k : k + 1])
        return acc.to(F64)


# ---------------------------------------------------------------------------
# parameters
# ---------------------------------------------------------------------------

def read_params(model) -> dict:
    """fp64 CPU copies of the model's parameters, in published naming."""
    arch = model.arch
    spec = model.spec
    P: dict = {"arch": arch, "layers": []}
    if arch in ("llama", "mixtral"):
        qs, ks = spec.num_heads * spec.head_dim, spec.num_kv_heads * spec.head_dim
        P["embed"] = _p(model.embed)
        P["norm"] = _p(model.final_norm_w)
        P["lm_head"] = _p(model.lm_head.weight)
        for layer in model.layers:
            qkv = _p(layer.attn.qkv_proj.weight)
            L = {
                "ln1": _p(layer.input_norm_w),
                "ln2": _p(layer.post_norm_w),
                "wq": qkv[:qs],
                "wk": qkv[qs : qs + ks],
                "wv": qkv[qs + ks : qs + 2 * ks],
                "wo": _p(layer.attn.o_proj.weight),
            }
            assert qkv.shape[0] == qs + 2 * ks
            inter = spec.intermediate_size
            if arch == "llama":
                gu = _p(layer.mlp.gate_up_proj.weight)
                L["w_gate"], L["w_up"] = gu[:inter], gu[inter:]
                L["w_down"] = _p(layer.mlp.down_proj.weight)
            else:
                L["router"] = _p(layer.moe.router_w)
                gu = _p(layer.moe.gate_up_w)
                L["w_gate"], L["w_up"] = gu[:, :inter], gu[:, inter:]
                L["w_down"] = _p(layer.moe.down_w)
            P["layers"].append(L)
    elif arch == "gpt2":
        h = spec.hidden_size
        P["wte"], P["wpe"] = _p(model.wte), _p(model.wpe)
        P["lnf_w"], P["lnf_b"] = _p(model.lnf_w), _p(model.lnf_b)
        for layer in model.layers:
            qkv_w, qkv_b = _p(layer.qkv_w), _p(layer.qkv_b)
            P["layers"].append(
                {
                    "ln1_w": _p(layer.ln1_w), "ln1_b": _p(layer.ln1_b),
                    "ln2_w": _p(layer.ln2_w), "ln2_b": _p(layer.ln2_b),
                    "wq": qkv_w[:h], "wk": qkv_w[h : 2 * h], "wv": qkv_w[2 * h :],
                    "bq": qkv_b[:h], "bk": qkv_b[h : 2 * h], "bv": qkv_b[2 * h :],
                    "wo": _p(layer.o_w), "bo": _p(layer.o_b),
                    "w_fc": _p(layer.fc_w), "b_fc": _p(layer.fc_b),
                    "w_proj": _p(layer.proj_w), "b_proj": _p(layer.proj_b),
                }
            )
    else:
        raise ValueError(arch)
    return P


# ---------------------------------------------------------------------------
# building blocks (fp64)
# ---------------------------------------------------------------------------

def rope_tables(head_dim: int, n_pos: int, theta: float):
    """cos/sin [n_pos, D/2] in fp64: angle = pos * theta^(-2i/D)."""
    i = torch.arange(0, head_dim, 2, dtype=F64)
    inv_freq = torch.pow(torch.tensor(float(theta), dtype=F64), -i / head_dim)
    ang = torch.outer(torch.arange(n_pos, dtype=F64), inv_freq)
    return ang.cos(), ang.sin()


def _rotate_half(x, cos, sin):
    """x [T, H, D]; dims (i, i + D/2) rotate together."""
    d2 = x.shape[-1] // 2
    x1, x2 = x[..., :d2], x[..., d2:]
    c, s = cos[:, None, :], sin[:, None, :]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def _rmsnorm(x, w, eps):
    return x / torch.sqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def _layernorm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).pow(2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x**3)))


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def _causal_attention(q, k, v, scale, r, prefill_mask):
    """q [T, Hq, D], k/v [T, Hkv, D] of ONE sequence; query t sees keys
    0..t; query head h reads kv head h // G. Returns [T, Hq, D]."""
    T, Hq, D = q.shape
    G = Hq // k.shape[1]
    out = torch.empty_like(q)
    causal = torch.arange(T)[None, :] <= torch.arange(T)[:, None]
    for h in range(Hq):
        kh, vh = k[:, h // G], v[:, h // G]
        s = r.mm(q[:, h], kh) * scale
        s = s.masked_fill(~causal, float("-inf"))
        e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        denom = e.sum(-1, keepdim=True)
        if r.mode is not None:
            # prefill: P rounded for the P.V product, row sum unrounded
            e = torch.where(prefill_mask[:, None], r(e), e)
        out[:, h] = r.mm(e, vh.T) / denom
    return out


def _kv_store(x, scale, r):
    """What the cache holds of x [T, Hkv, D]. scale: [Hkv] or None."""
    if scale is None or r.mode is None:
        return x
    s = scale.to(torch.float32).reshape(-1, 1)
    code = quantize_kv_fp8(x.to(torch.float32), s)
    return (code.to(torch.float32) * s).to(F64)


# ---------------------------------------------------------------------------
# forwards
# ---------------------------------------------------------------------------

def _forward_llama(P, spec, tokens, r, kv_scales, prefill_mask, is_moe):
    T = len(tokens)
    Hq, Hkv, D = spec.num_heads, spec.num_kv_heads, spec.head_dim
    eps = spec.rms_eps
    cos, sin = rope_tables(D, T, spec.rope_theta)
    out = {"resid": [], "k": [], "v": [], "router_probs": []}
    stream = r(P["embed"][torch.tensor(tokens)])
    for li, L in enumerate(P["layers"]):
        x = r(_rmsnorm(stream, L["ln1"], eps))
        q = r(r.mm(x, L["wq"])).view(T, Hq, D)
        k = r(r.mm(x, L["wk"])).view(T, Hkv, D)
        v = r(r.mm(x, L["wv"])).view(T, Hkv, D)
        q, k = r(_rotate_half(q, cos, sin)), r(_rotate_half(k, cos, sin))
        ksc = None if kv_scales is None else kv_scales[li][0]
        vsc = None if kv_scales is None else kv_scales[li][1]
        k, v = _kv_store(k, ksc, r), _kv_store(v, vsc, r)
        out["k"].append(k)
        out["v"].append(v)
        a = r(_causal_attention(q, k, v, 1.0 / math.sqrt(D), r, prefill_mask))
        a = r(r.mm(a.reshape(T, Hq * D), L["wo"]))
        stream = r(stream + a)
        x = r(_rmsnorm(stream, L["ln2"], eps))
        if not is_moe:
            act = r(_silu(r(r.mm(x, L["w_gate"]))) * r(r.mm(x, L["w_up"])))
            m = r(r.mm(act, L["w_down"]))
        else:
            probs = torch.softmax(r.mm(x, L["router"]), dim=-1)
            out["router_probs"].append(probs)
            top_w, top_e = torch.topk(probs, spec.experts_per_token, dim=-1)
            top_w = top_w / top_w.sum(-1, keepdim=True)
            # each expert's SwiGLU MLP on the tokens routed to it ...
            y = {}
            for e in range(spec.num_experts):
                rows = (top_e == e).any(-1).nonzero().flatten()
                xe = x[rows]
                act = r(_silu(r(r.mm(xe, L["w_gate"][e]))) * r(r.mm(xe, L["w_up"][e])))
                ye = r(r.mm(act, L["w_down"][e]))
                y[e] = {int(t): ye[i] for i, t in enumerate(rows)}
            # ... combined per token, per chosen expert
            m = torch.zeros(T, spec.hidden_size, dtype=F64)
            for t in range(T):
                for j in range(spec.experts_per_token):
                    m[t] += top_w[t, j] * y[int(top_e[t, j])][t]
            m = r(m)
        # the residual stream after the layer; the served model keeps it
        # as two tensors until the next norm adds them
        out["resid"].append(m + stream)
        stream = r(m + stream)
    x = r(_rmsnorm(stream, P["norm"], eps))
    out["logits"] = r(r.mm(x, P["lm_head"]))
    return out


def _forward_gpt2(P, spec, tokens, r, kv_scales, prefill_mask):
    T = len(tokens)
    Hq, D = spec.num_heads, spec.head_dim
    eps = spec.layernorm_eps
    out = {"resid": [], "k": [], "v": []}
    h = r(P["wte"][torch.tensor(tokens)] + P["wpe"][torch.arange(T)])
    for li, L in enumerate(P["layers"]):
        x = r(_layernorm(h, L["ln1_w"], L["ln1_b"], eps))
        q = r(r.mm(x, L["wq"]) + L["bq"]).view(T, Hq, D)
        k = r(r.mm(x, L["wk"]) + L["bk"]).view(T, Hq, D)
        v = r(r.mm(x, L["wv"]) + L["bv"]).view(T, Hq, D)
        ksc = None if kv_scales is None else kv_scales[li][0]
        vsc = None if kv_scales is None else kv_scales[li][1]
        k, v = _kv_store(k, ksc, r), _kv_store(v, vsc, r)
        out["k"].append(k)
        out["v"].append(v)
        a = r(_causal_attention(q, k, v, 1.0 / math.sqrt(D), r, prefill_mask))
        h = r(h + r(r.mm(a.reshape(T, Hq * D), L["wo"]) + L["bo"]))
        x = r(_layernorm(h, L["ln2_w"], L["ln2_b"], eps))
        x = r(_gelu_tanh(r(r.mm(x, L["w_fc"]) + L["b_fc"])))
        h = r(h + r(r.mm(x, L["w_proj"]) + L["b_proj"]))
        out["resid"].append(h)
    x = r(_layernorm(h, P["lnf_w"], P["lnf_b"], eps))
    out["logits"] = r(r.mm(x, P["wte"]))  # tied head
    return out


def dense_forward(
    model,
    sequences: list,
    mode: Optional[torch.dtype] = None,
    kv_scales: Optional[torch.Tensor] = None,
    prefill_masks: Optional[list] = None,
    params: Optional[dict] = None,
) -> list:
    """One dict per token sequence with, for every position:
    ``resid[l]`` [T, H], ``logits`` [T, V], ``k[l]`` / ``v[l]`` [T, Hkv, D]
    (K after RoPE), and for Mixtral ``router_probs[l]`` [T, E].

    mode: None = exact fp64, or the dtype of ``rounded``.
    kv_scales: [layers, 2, Hkv] of an FP8 KV cache (``rounded`` only).
    prefill_masks: per sequence, bool [T]: positions computed by prefill.
    """
    P = params if params is not None else read_params(model)
    spec = model.spec
    r = _Rounder(mode)
    if kv_scales is not None:
        kv_scales = kv_scales.detach().cpu()
    results = []
    for si, tokens in enumerate(sequences):
        mask = (
            torch.ones(len(tokens), dtype=torch.bool)
            if prefill_masks is None
            else prefill_masks[si]
        )
        if P["arch"] == "gpt2":
            results.append(_forward_gpt2(P, spec, tokens, r, kv_scales, mask))
        else:
            results.append(
                _forward_llama(
                    P, spec, tokens, r, kv_scales, mask, P["arch"] == "mixtral"
                )
            )
    return results
