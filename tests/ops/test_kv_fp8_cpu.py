"""FP8 (e4m3fn, scale 1.0) KV cache: the store specification
(torch_ref.quantize_kv_fp8) over every bf16 value, and the CPU reference
append / attention on an FP8 cache."""

import math

import torch

from dts_amd.ops import torch_ref

FP8 = torch.float8_e4m3fn


def _all_non_nan_bf16():
    bits = torch.arange(65536, dtype=torch.int32)
    is_nan = ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)
    bits = bits[~is_nan]
    assert bits.numel() == 65282
    return bits.to(torch.int16).view(torch.bfloat16)


def _finite_codes():
    c = torch.arange(256, dtype=torch.int32)
    c = c[(c & 0x7F) != 0x7F].to(torch.uint8)
    assert c.numel() == 254
    return c


class TestQuantizeKvFp8:
    def test_never_nan(self):
        code = torch_ref.quantize_kv_fp8(_all_non_nan_bf16()).view(torch.uint8)
        assert not ((code & 0x7F) == 0x7F).any()

    def test_saturates(self):
        x = _all_non_nan_bf16()
        code = torch_ref.quantize_kv_fp8(x).view(torch.uint8)
        xf = x.float()
        assert (code[xf >= 448] == 0x7E).all()
        assert (code[xf <= -448] == 0xFE).all()
        inf = torch.tensor([float("inf"), -float("inf")], dtype=torch.bfloat16)
        assert torch_ref.quantize_kv_fp8(inf).view(torch.uint8).tolist() == [0x7E, 0xFE]
        # values the plain cast turns into NaN
        big = torch.tensor([465.0, 500.0, 3e38])
        assert torch_ref.quantize_kv_fp8(big).view(torch.uint8).tolist() == [0x7E] * 3

    def test_idempotent_on_finite_codes(self):
        codes = _finite_codes()
        for deq in (codes.view(FP8).float(), codes.view(FP8).to(torch.bfloat16)):
            again = torch_ref.quantize_kv_fp8(deq).view(torch.uint8)
            assert torch.equal(again, codes)
        # and every finite code is a bf16 value: dequantisation is exact
        f = codes.view(FP8).float()
        assert torch.equal(f.to(torch.bfloat16).float(), f)

    def test_relative_error_half_ulp(self):
        x = _all_non_nan_bf16().float()
        x = x[(x.abs() >= 2.0**-6) & (x.abs() <= 448)]
        deq = torch_ref.quantize_kv_fp8(x).float()
        rel = ((deq - x).abs() / x.abs()).max().item()
        print(f"max relative error {rel:.4f}")
        assert rel <= 2.0**-4


def test_kv_append_writes_codes_at_slots_only():
    torch.manual_seed(0)
    T, Hk, D, BS, NB = 11, 2, 8, 4, 6
    k = torch.randn(T, Hk, D) * 8
    v = torch.randn(T, Hk, D) * 8
    k[0, 0, :4] = torch.tensor([449.0, 500.0, -1e4, float("inf")])
    v[1, 1, :2] = torch.tensor([-float("inf"), 465.0])
    slots = torch.randperm(NB * BS)[:T]
    kc = torch.full((NB, Hk, BS, D), 0x55, dtype=torch.uint8).view(FP8)
    vc = torch.full((NB, Hk, BS, D), 0x55, dtype=torch.uint8).view(FP8)
    torch_ref.kv_append(k, v, kc, vc, slots)
    for cache, src in ((kc, k), (vc, v)):
        flat = cache.view(torch.uint8).permute(0, 2, 1, 3).reshape(NB * BS, Hk, D)
        want = torch_ref.quantize_kv_fp8(src).view(torch.uint8)
        assert torch.equal(flat[slots], want)
        untouched = torch.ones(NB * BS, dtype=torch.bool)
        untouched[slots] = False
        assert (flat[untouched] == 0x55).all()
        assert not ((flat & 0x7F) == 0x7F).any()


def _fp8_paged_cache(NB, Hkv, BS, D, gen):
    shape = (NB, Hkv, BS, D)
    u = torch.randint(-8, 4, shape, generator=gen)
    return torch_ref.quantize_kv_fp8(torch.randn(shape, generator=gen) * 2.0**u)


def test_attention_refs_equal_on_fp32_copy():
    g = torch.Generator().manual_seed(3)
    Hq, Hkv, D, BS = 4, 2, 16, 4
    kv_lens = [1, 7, 13]
    max_blocks = 4
    NB = 3 * max_blocks
    kc = _fp8_paged_cache(NB, Hkv, BS, D, g)
    vc = _fp8_paged_cache(NB, Hkv, BS, D, g)
    bt = torch.randperm(NB, generator=g).view(3, max_blocks).to(torch.int32)
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    q = torch.randn(3, Hq, D, generator=g)
    got = torch_ref.attn_decode_paged(q, kc, vc, bt, kvl, scale)
    ref = torch_ref.attn_decode_paged(q, kc.float(), vc.float(), bt, kvl, scale)
    assert torch.equal(got, ref)
    assert torch.isfinite(got).all()

    q_lens, ctx = [1, 4, 6], [0, 3, 7]
    cu_q = torch.tensor([0, 1, 5, 11], dtype=torch.int32)
    q_pos = torch.cat([torch.arange(c, c + n) for n, c in zip(q_lens, ctx)])
    qp = torch.randn(11, Hq, D, generator=g)
    got = torch_ref.attn_prefill_paged(qp, cu_q, q_pos, kc, vc, bt, kvl, scale)
    ref = torch_ref.attn_prefill_paged(
        qp, cu_q, q_pos, kc.float(), vc.float(), bt, kvl, scale
    )
    assert torch.equal(got, ref)
    assert torch.isfinite(got).all()
