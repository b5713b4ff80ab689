"""FP8 KV cache with power-of-two per-head scales: the torch references
(the specification of the store, the paged round trip, and what the scales
buy at attention level)."""

import math

import pytest
import torch

from dts_amd.ops import torch_ref
from dts_amd.ops.torch_ref import quantize_kv_fp8
from dts_amd.serving.kv_cache import scales_from_amax

FP8 = torch.float8_e4m3fn
BS = 16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bytes(t):
    return t.view(torch.uint8)


# ---------------------------------------------------------------------------
# quantize_kv_fp8(x, scale)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("e", [-20, -9, -1, 0, 3, 20])
def test_scaled_store_is_store_of_x_over_s(e):
    g = _gen(e + 100)
    u = torch.randint(-24, 16, (64, 3, 32), generator=g)
    x = (torch.randn(64, 3, 32, generator=g) * 2.0**u).to(torch.bfloat16)
    s = torch.tensor(2.0**e)
    got = quantize_kv_fp8(x, s)
    assert got.dtype == FP8
    assert torch.equal(_bytes(got), _bytes(quantize_kv_fp8(x.float() / s)))
    assert not ((_bytes(got) & 0x7F) == 0x7F).any()


def test_per_head_scale_broadcasts():
    g = _gen(1)
    x = torch.randn(10, 4, 16, generator=g)
    s = torch.tensor([2.0**-7, 2.0**-2, 1.0, 2.0**4]).unsqueeze(-1)  # [Hkv, 1]
    got = quantize_kv_fp8(x, s)
    for h in range(4):
        assert torch.equal(
            _bytes(got[:, h]), _bytes(quantize_kv_fp8(x[:, h] / s[h]))
        )


def test_scaled_store_saturates():
    s = torch.tensor(2.0**3)
    x = torch.tensor([448.0 * 8, 449.0 * 8, 1e6, -1e6, float("inf"), -float("inf")])
    got = quantize_kv_fp8(x, s).float() * s
    assert got.tolist() == [3584.0, 3584.0, 3584.0, -3584.0, 3584.0, -3584.0]
    # at unit scale the same inputs all clip at 448
    assert quantize_kv_fp8(x).float().abs().max().item() == 448.0


def test_unit_scale_is_the_unscaled_store():
    g = _gen(2)
    x = torch.randn(50, 2, 64, generator=g) * 100
    assert torch.equal(_bytes(quantize_kv_fp8(x, torch.tensor(1.0))), _bytes(quantize_kv_fp8(x)))
    assert torch.equal(_bytes(quantize_kv_fp8(x, None)), _bytes(quantize_kv_fp8(x)))


# ---------------------------------------------------------------------------
# Paged round trip
# ---------------------------------------------------------------------------

def test_paged_round_trip_distinct_scales_per_head():
    g = _gen(3)
    T, Hkv, D, NB = 37, 3, 32, 4
    kv_scale = torch.tensor([[2.0**-7, 2.0**-2, 2.0**4], [2.0**3, 2.0**-5, 2.0**-1]])
    # values placed so that each head's scale matters: amax ~ 200 * scale
    k = torch.randn(T, Hkv, D, generator=g) * 60 * kv_scale[0].view(1, Hkv, 1)
    v = torch.randn(T, Hkv, D, generator=g) * 60 * kv_scale[1].view(1, Hkv, 1)
    kc = torch.zeros(NB, Hkv, BS, D).to(FP8)
    vc = torch.zeros(NB, Hkv, BS, D).to(FP8)
    table = torch.tensor([2, 0, 3])
    pos = torch.arange(T)
    slots = table[pos // BS] * BS + pos % BS
    torch_ref.kv_append(k, v, kc, vc, slots, kv_scale)
    gk, gv = torch_ref.gather_kv(kc, vc, table, T, kv_scale)
    for h in range(Hkv):
        for got, src, s in ((gk, k, kv_scale[0, h]), (gv, v, kv_scale[1, h])):
            want = quantize_kv_fp8(src[:, h] / s).float() * s
            assert torch.equal(got[:, h], want)
            # e4m3 keeps 3 mantissa bits: relative error <= 2^-4 for normals
            rel = (got[:, h] - src[:, h]).abs() / src[:, h].abs().clamp_min(1e-30)
            assert rel[src[:, h].abs() > s * 2.0**-6].max() <= 2.0**-4
    # the block the table does not name is untouched
    assert not _bytes(kc[1]).any() and not _bytes(vc[1]).any()


def test_scale_with_a_non_fp8_cache_raises():
    k = torch.zeros(2, 1, 8)
    kc = torch.zeros(1, 1, BS, 8)
    s = torch.ones(2, 1)
    with pytest.raises(ValueError):
        torch_ref.kv_append(k, k, kc, kc.clone(), torch.arange(2), s)
    with pytest.raises(ValueError):
        torch_ref.gather_kv(kc, kc, torch.tensor([0]), 2, s)


# ---------------------------------------------------------------------------
# What the scales buy: attention-level accuracy
# ---------------------------------------------------------------------------

D, N_KEYS, HQ, HKV = 128, 300, 8, 2


def _recipe(kind):
    """300 keys, D=128. "outlier": one K channel reaching 4300 (saturates at
    448 under unit scale). "tiny_v": V of std 0.004 (subnormal / zero codes
    under unit scale)."""
    g = _gen(7)
    q = torch.randn(1, HQ, D, generator=g)
    k = torch.randn(N_KEYS, HKV, D, generator=g)
    v = torch.randn(N_KEYS, HKV, D, generator=g)
    if kind == "outlier":
        ch = torch.randn(N_KEYS, HKV, generator=g)
        k[:, :, 5] = ch / ch.abs().max() * 4300.0
        q[:, :, 5] = torch.randn(1, HQ, generator=g) * 0.01
    else:
        v = v * 0.004
    return q, k, v


def _paged_attention(q, k, v, kv_scale):
    n_blocks = (N_KEYS + BS - 1) // BS
    kc = torch.zeros(n_blocks, HKV, BS, D).to(FP8)
    vc = torch.zeros(n_blocks, HKV, BS, D).to(FP8)
    torch_ref.kv_append(k, v, kc, vc, torch.arange(N_KEYS), kv_scale)
    bt = torch.arange(n_blocks, dtype=torch.int32).unsqueeze(0)
    kvl = torch.tensor([N_KEYS], dtype=torch.int32)
    return torch_ref.attn_decode_paged(q, kc, vc, bt, kvl, None, kv_scale)


def _calibrated(k, v):
    amax = torch.stack([k.abs().amax(dim=(0, 2)), v.abs().amax(dim=(0, 2))])
    return scales_from_amax(amax, headroom=2.0)


@pytest.mark.parametrize("kind", ["outlier", "tiny_v"])
def test_calibrated_scales_at_least_halve_the_attention_error(kind):
    q, k, v = _recipe(kind)
    exact = torch_ref._sdpa(q, k, v, 1.0 / math.sqrt(D))

    def err(out):
        return ((out - exact).norm() / exact.norm()).item()

    e_unit = err(_paged_attention(q, k, v, None))
    kv_scale = _calibrated(k, v)
    assert ((torch.log2(kv_scale) % 1) == 0).all()
    e_cal = err(_paged_attention(q, k, v, kv_scale))
    print(f"{kind}: unit {e_unit:.4f} calibrated {e_cal:.4f} scales {kv_scale.tolist()}")
    assert e_cal <= 0.5 * e_unit
