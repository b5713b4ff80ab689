"""The host wrappers reject arguments the kernels would misread.

The kernels take raw pointers: an int64 kv_lens read as int32, an fp32
weight read as bf16 or a strided residual addressed densely gives wrong
numbers, not an error. Each case here passes one such argument and expects
a RuntimeError from the wrapper's checks; the same call with the good
argument runs first, so the error is that argument's.

Every bad argument is a view of, or at least as large as, what the kernel
would address, and every index it could misread stays in range: a wrapper
without the check would compute garbage inside allocated memory. No case
depends on a fault to fail.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader

ext = _hip_ext_loader.load()
DEV = "cuda:0"
BF16 = torch.bfloat16
BS = 16


def _bf16(*shape):
    return torch.randn(*shape, device=DEV).to(BF16)


def _as_int32_prefix(t64):
    """int32 view of an int64 tensor, cut to its length: half of the bytes a
    kernel reading int64 would touch, all of them inside the buffer."""
    return t64.view(torch.int32)[: t64.shape[0]]


def _check(fn, good, bad_cases):
    fn(**good)
    torch.cuda.synchronize()
    for name, bad in bad_cases.items():
        with pytest.raises(RuntimeError):
            fn(**{**good, **bad})
        print(f"rejected: {name}")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------

T, H = 6, 256


def _wide():
    """[T, H] non-contiguous view of a [T, 2H] buffer."""
    return _bf16(T, 2 * H)[:, :H]


def test_rmsnorm_contract():
    good = dict(out=_bf16(T, H), x=_bf16(T, H), w=_bf16(H), eps=1e-5)
    _check(lambda out, x, w, eps: ext.rmsnorm(out, x, w, eps), good, {
        "strided out": dict(out=_wide()),
        "fp32 out": dict(out=torch.zeros(T, H, device=DEV)),
        "out of another shape": dict(out=_bf16(T + 1, H)),
        "fp32 w": dict(w=torch.ones(H, device=DEV)),
        "w of length 2H": dict(w=_bf16(2 * H)),
        "strided w": dict(w=_bf16(2 * H)[::2]),
    })


def test_fused_add_rmsnorm_contract():
    good = dict(x=_bf16(T, H), residual=_bf16(T, H), w=_bf16(H), eps=1e-5)
    # H % 8 != 0: a contiguous [T, 12] window of a larger buffer
    x12 = _bf16(T * 12 + 64)[: T * 12].view(T, 12)
    r12 = _bf16(T * 12 + 64)[: T * 12].view(T, 12)
    _check(lambda x, residual, w, eps: ext.fused_add_rmsnorm(x, residual, w, eps), good, {
        "strided residual": dict(residual=_wide()),
        "fp32 residual": dict(residual=torch.zeros(T, H, device=DEV)),
        "residual of another shape": dict(residual=_bf16(T + 1, H)),
        "fp32 w": dict(w=torch.ones(H, device=DEV)),
        "w of length 2H": dict(w=_bf16(2 * H)),
        "H % 8 != 0": dict(x=x12, residual=r12, w=_bf16(16)[:12]),
    })


def test_layernorm_contract():
    good = dict(out=_bf16(T, H), x=_bf16(T, H), w=_bf16(H), b=_bf16(H), eps=1e-5)
    _check(lambda out, x, w, b, eps: ext.layernorm(out, x, w, b, eps), good, {
        "strided out": dict(out=_wide()),
        "fp32 out": dict(out=torch.zeros(T, H, device=DEV)),
        "fp32 w": dict(w=torch.ones(H, device=DEV)),
        "w of length 2H": dict(w=_bf16(2 * H)),
        "fp32 b": dict(b=torch.zeros(H, device=DEV)),
    })


# ---------------------------------------------------------------------------
# rope_kv_append / kv_append
# ---------------------------------------------------------------------------

def _append_args(Hq=4, Hk=2, D=64, n_tok=5, blocks=3):
    fused = _bf16(n_tok, (Hq + 2 * Hk) * D)
    q = fused[:, : Hq * D].view(n_tok, Hq, D)
    k = fused[:, Hq * D : (Hq + Hk) * D].view(n_tok, Hk, D)
    v = fused[:, (Hq + Hk) * D :].view(n_tok, Hk, D)
    pos = torch.arange(n_tok, dtype=torch.long, device=DEV)
    slots = torch.arange(n_tok, dtype=torch.long, device=DEV) * 3
    cos = torch.ones(64, D // 2, device=DEV)
    sin = torch.zeros(64, D // 2, device=DEV)
    kc = torch.zeros(blocks, Hk, BS, D, dtype=BF16, device=DEV)
    vc = torch.zeros(blocks, Hk, BS, D, dtype=BF16, device=DEV)
    return q, k, v, pos, cos, sin, kc, vc, slots


def test_rope_kv_append_contract():
    q, k, v, pos, cos, sin, kc, vc, slots = _append_args()
    good = dict(positions=pos, slots=slots)

    def call(positions, slots):
        ext.rope_kv_append(q, k, v, positions, cos, sin, kc, vc, slots)

    _check(call, good, {
        "int32 positions": dict(positions=_as_int32_prefix(pos)),
        "int32 slots": dict(slots=_as_int32_prefix(slots)),
        "strided slots": dict(slots=torch.zeros(2 * len(slots), dtype=torch.long, device=DEV)[::2]),
    })


def test_kv_append_contract():
    _, k, v, _, _, _, kc, vc, slots = _append_args()
    n_tok, Hk, D = k.shape
    good = dict(k=k, v=v, slots=slots)
    # heads D apart inside rows of 2D: not the dense-head layout
    gappy = _bf16(n_tok, Hk, 2 * D)[:, :, :D]

    def call(k, v, slots):
        ext.kv_append(k, v, kc, vc, slots)

    _check(call, good, {
        "int32 slots": dict(slots=_as_int32_prefix(slots)),
        "k heads not dense": dict(k=gappy),
        "v heads not dense": dict(v=gappy),
        "fp32 k": dict(k=torch.zeros(n_tok, Hk, D, device=DEV)),
        "fp32 v": dict(v=torch.zeros(n_tok, Hk, D, device=DEV)),
    })


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------

def test_attn_decode_contract():
    B, Hq, Hkv, D, W = 3, 8, 2, 128, 4
    kc, vc = _bf16(B * W, Hkv, BS, D), _bf16(B * W, Hkv, BS, D)
    bt = torch.arange(B * W, dtype=torch.int32, device=DEV).view(B, W)
    good = dict(kv_lens=torch.tensor([5, 17, 64], dtype=torch.int32, device=DEV))
    q, out = _bf16(B, Hq, D), _bf16(B, Hq, D)

    def call(kv_lens):
        ext.attn_decode_paged(out, q, kc, vc, bt, kv_lens, 1.0 / math.sqrt(D))

    _check(call, good, {
        # read as int32 this is (5, 0, 17): lengths that are in range
        "int64 kv_lens": dict(kv_lens=torch.tensor([5, 17, 64], device=DEV)),
    })


def test_attn_prefill_contract():
    P, Hq, Hkv, D, W = 2, 8, 2, 128, 4
    kc, vc = _bf16(P * W, Hkv, BS, D), _bf16(P * W, Hkv, BS, D)
    q_lens = [7, 20]
    Tq = sum(q_lens)
    q, out = _bf16(Tq, Hq, D), _bf16(Tq, Hq, D)
    cu_q = torch.tensor([0, 7, 27], dtype=torch.int32, device=DEV)
    q_pos = torch.cat([torch.arange(n) for n in q_lens]).to(DEV)
    good = dict(
        q_pos=q_pos,
        block_tables=torch.arange(P * W, dtype=torch.int32, device=DEV).view(P, W),
        kv_lens=torch.tensor(q_lens, dtype=torch.int32, device=DEV),
    )

    def call(q_pos, block_tables, kv_lens):
        ext.attn_prefill_paged(
            out, q, cu_q, q_pos, kc, vc, block_tables, kv_lens, 1.0 / math.sqrt(D)
        )

    _check(call, good, {
        # read as int32: (7, 0), block ids (0, 0, 1, 0, ...) -- all in range
        "int64 kv_lens": dict(kv_lens=torch.tensor(q_lens, device=DEV)),
        "int64 block_tables": dict(block_tables=good["block_tables"].long()),
        "int32 q_pos": dict(q_pos=_as_int32_prefix(q_pos)),
    })


# ---------------------------------------------------------------------------
# GEMMs
# ---------------------------------------------------------------------------

M, N, K = 4, 32, 512


def _gemm_bad():
    return {
        # twice the bytes the kernel would read as bf16
        "fp32 weight": dict(w=torch.zeros(N, K, device=DEV)),
        "weight of 2K columns": dict(w=_bf16(N, 2 * K)),
    }


def test_gemv_contract():
    good = dict(out=_bf16(M, N), x=_bf16(M, K), w=_bf16(N, K))
    _check(lambda out, x, w: ext.gemv_bf16(out, x, w), good, _gemm_bad())


def test_gemm_skinny_contract():
    good = dict(out=_bf16(M, N), x=_bf16(M, K), w=_bf16(N, K))
    _check(lambda out, x, w: ext.gemm_skinny_bf16(out, x, w), good, _gemm_bad())


def test_gemm_skinny_swiglu_contract():
    good = dict(out=_bf16(M, N // 2), x=_bf16(M, K), w=_bf16(N, K))
    _check(lambda out, x, w: ext.gemm_skinny_swiglu_bf16(out, x, w), good, _gemm_bad())


def test_moe_grouped_linear_contract():
    E_ = 2
    good = dict(
        out=_bf16(M, N), x=_bf16(M, K), w=_bf16(E_, N, K),
        counts=torch.tensor([1, 3], dtype=torch.int32, device=DEV),
        offsets=torch.tensor([0, 1], dtype=torch.int32, device=DEV),
    )
    _check(
        lambda out, x, w, counts, offsets: ext.moe_grouped_linear(out, x, w, counts, offsets),
        good,
        {
            "fp32 weight": dict(w=torch.zeros(E_, N, K, device=DEV)),
            "weight of 2K columns": dict(w=_bf16(E_, N, 2 * K)),
        },
    )
