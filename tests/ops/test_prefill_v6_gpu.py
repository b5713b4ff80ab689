"""Prefill attention v6 (transposed-LDS V reads, next-tile prefetch) against
v5, which it must reproduce bit for bit.

Variants: 6 = transposed reads + next-tile prefetch (the default), 7 =
transposed reads only (the ablation form). One call carries six
sequences (cached prefix, chunk) that cover one q-tile over six kv tiles
ragged on the 16 and 64 boundaries, a pure causal chunk with a ragged last
q-tile, a kv_len that ends on a tile boundary, a single token and exactly one
full q-tile at G=4. grid.x is sized from the total, so tiles past a sequence's
q_len are launched and must exit.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader, torch_ref

ext = _hip_ext_loader.load()

DEV = "cuda:0"
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
BS = 16
SEQS = ((333, 5), (0, 70), (40, 37), (64, 64), (1, 1), (130, 16))
CONFIGS = [(8, 2, 128), (8, 1, 128), (4, 2, 128), (4, 4, 128), (4, 4, 64)]
FP8_CONFIGS = [(8, 2, 128), (4, 4, 64)]
V6_FORMS = [6, 7]
K_EXP = (-7, -3, 1, 4)
V_EXP = (3, -6, -1, -4)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _strided_q(T, Hq, D, g):
    buf = torch.randn(T, Hq * D + 2 * D, generator=g).to(BF16).to(DEV)
    q = buf[:, D : D + Hq * D].view(T, Hq, D)
    assert not q.is_contiguous()
    return q


def _randn_cache(shape, g):
    return torch.randn(shape, generator=g).to(BF16)


def _uniform_code_cache(shape, g):
    c = torch.arange(256, dtype=torch.int32)
    c = c[(c & 0x7F) != 0x7F].to(torch.uint8)
    return c[torch.randint(0, 254, shape, generator=g)].view(FP8)


def _case(Hq, Hkv, D, make_cache, seed):
    g = _gen(seed)
    kv_lens = [p + c for p, c in SEQS]
    q_lens = [c for _, c in SEQS]
    P = len(SEQS)
    max_blocks = (max(kv_lens) + BS - 1) // BS
    NB = P * max_blocks + 2
    kc = make_cache((NB, Hkv, BS, D), g)
    vc = make_cache((NB, Hkv, BS, D), g)
    bt = torch.randperm(NB, generator=g)[: P * max_blocks].view(P, max_blocks)
    bt = bt.to(torch.int32)
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    cu = [0]
    for n in q_lens:
        cu.append(cu[-1] + n)
    cu_q = torch.tensor(cu, dtype=torch.int32)
    q_pos = torch.cat([torch.arange(p, p + c, dtype=torch.long) for p, c in SEQS])
    q = _strided_q(sum(q_lens), Hq, D, g)
    return q, cu_q, q_pos, kc, vc, bt, kvl, 1.0 / math.sqrt(D)


def _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant, kv_scale=None):
    out = torch.empty(q.shape, dtype=BF16, device=DEV)
    ext.attn_prefill_paged(
        out, q, cu_q.to(DEV), q_pos.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV),
        kvl.to(DEV), scale, swz=variant,
        kv_scale=None if kv_scale is None else kv_scale.to(DEV),
    )
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _bf16_case(Hq, Hkv, D):
    """The inputs of tests 1-3 and v5's output on them, computed once."""
    case = _case(Hq, Hkv, D, _randn_cache, 60)
    want = _prefill(*case, 5)
    assert torch.isfinite(want.float()).all()
    return case, want


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("variant", V6_FORMS)
@pytest.mark.parametrize("Hq,Hkv,D", CONFIGS)
def test_v6_equals_v5_bitwise(Hq, Hkv, D, variant):
    case, want = _bf16_case(Hq, Hkv, D)
    got = _prefill(*case, variant)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("variant", V6_FORMS)
@pytest.mark.parametrize("Hq,Hkv,D", CONFIGS)
def test_v6_guards(Hq, Hkv, D, variant):
    """Every slot at a position >= kv_len in a sequence's pages, every
    unowned block, and every block that an unused block-table entry names is
    NaN. All of these are legal addresses: a kernel that formed an address
    from such an entry, or read past kv_len, would pick up NaNs, not fault.
    v5 reads none of them."""
    (q, cu_q, q_pos, kc, vc, bt, kvl, scale), want = _bf16_case(Hq, Hkv, D)
    live = torch.zeros(kc.shape[0], BS, dtype=torch.bool)
    for i, n in enumerate(kvl.tolist()):
        for pos in range(n):
            live[bt[i, pos // BS], pos % BS] = True
    assert not live.all(dim=1).all() and (~live.any(dim=1)).any()
    nan = torch.tensor(float("nan"), dtype=BF16)
    m = live.view(-1, 1, BS, 1)
    kc_p, vc_p = torch.where(m, kc, nan), torch.where(m, vc, nan)
    used = (kvl + BS - 1) // BS
    for i in range(bt.shape[0]):
        for blk in bt[i, used[i] :].tolist():
            assert torch.isnan(kc_p[blk].float()).all()
    got = _prefill(q, cu_q, q_pos, kc_p, vc_p, bt, kvl, scale, variant)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("variant", V6_FORMS)
@pytest.mark.parametrize("Hq,Hkv,D", CONFIGS)
def test_v6_matches_fp32_reference(Hq, Hkv, D, variant):
    (q, cu_q, q_pos, kc, vc, bt, kvl, scale), _ = _bf16_case(Hq, Hkv, D)
    ref = _fp32_reference(Hq, Hkv, D)
    got = _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant).float()
    print(f"max abs diff {(got - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got, ref, atol=2.5e-2, rtol=2.5e-2)


@functools.lru_cache(maxsize=None)
def _fp32_reference(Hq, Hkv, D):
    (q, cu_q, q_pos, kc, vc, bt, kvl, scale), _ = _bf16_case(Hq, Hkv, D)
    return torch_ref.attn_prefill_paged(
        q.cpu().float(), cu_q, q_pos, kc.float(), vc.float(), bt, kvl, scale
    )


def _dequant(cache, head_scale):
    """FP8 [NB, Hkv, BS, D] -> the bf16 cache it denotes (exact)."""
    f = cache.float() * head_scale.view(1, -1, 1, 1)
    b = f.to(BF16)
    assert torch.equal(b.float(), f)
    return b


@pytest.mark.parametrize("variant", V6_FORMS)
@pytest.mark.parametrize("Hq,Hkv,D", FP8_CONFIGS)
def test_v6_fp8_cache(Hq, Hkv, D, variant):
    """Uniformly random finite codes, a different power-of-two scale per
    head and per K / V: v6 on the FP8 cache is v6 on the dequantised bf16
    cache and v5 on the FP8 cache, bit for bit."""
    q, cu_q, q_pos, kc, vc, bt, kvl, scale = _case(Hq, Hkv, D, _uniform_code_cache, 61)
    sc = torch.tensor(
        [[2.0**e for e in K_EXP[:Hkv]], [2.0**e for e in V_EXP[:Hkv]]],
        dtype=torch.float32,
    )
    got = _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant, sc)
    on_bf16 = _prefill(
        q, cu_q, q_pos, _dequant(kc, sc[0]), _dequant(vc, sc[1]), bt, kvl, scale, variant
    )
    v5 = _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, 5, sc)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(_bits(got), _bits(on_bf16))
    assert torch.equal(_bits(got), _bits(v5))
    # and it is not the unscaled result
    assert not torch.equal(got, _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant))
