"""FP8 KV cache with power-of-two per-head scales on the GPU: append, decode
and prefill attention.

Every head, and K and V of a head, carry a different power of two, so a
kernel that reads another head's scale, or K's row for V, fails. The store
is pinned byte for byte against torch_ref.quantize_kv_fp8(x, scale) over
every bf16 value. The load is pinned exactly where the arithmetic allows it:
a decode that selects one key per query, a prefill with a single key per
query over all 254 finite codes, and prefill against the same variant on the
dequantised bf16 cache (code * 2^e is exactly a bf16 value).
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader, torch_ref
from dts_amd.serving.kv_cache import scales_from_amax

ext = _hip_ext_loader.load()
quantize_kv_fp8 = torch_ref.quantize_kv_fp8  # the specification of the store

DEV = "cuda:0"
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
BS = 16
SENTINEL = 0x55
CONFIGS = [(8, 2, 128), (8, 1, 128), (2, 2, 128), (4, 4, 64)]  # Hq, Hkv, D
K_EXP = (-7, -3, 1, 4, 2, -5, 0, -1)
V_EXP = (3, -6, -1, -4, -7, 4, 1, -2)


def _scales(Hkv):
    """[2, Hkv] fp32: distinct powers of two per head and per K / V."""
    return torch.tensor(
        [[2.0**e for e in K_EXP[:Hkv]], [2.0**e for e in V_EXP[:Hkv]]],
        dtype=torch.float32,
    )


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _finite_codes():
    c = torch.arange(256, dtype=torch.int32)
    c = c[(c & 0x7F) != 0x7F].to(torch.uint8)
    assert c.numel() == 254
    return c


def _all_non_nan_bf16():
    bits = torch.arange(65536, dtype=torch.int32)
    is_nan = ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)
    bits = bits[~is_nan]
    assert bits.numel() == 65282
    return bits.to(torch.int16).view(BF16)


def _sentinel_cache(NB, Hk, D):
    return torch.full((NB, Hk, BS, D), SENTINEL, dtype=torch.uint8, device=DEV).view(FP8)


def _by_slot(cache):
    """[NB, Hk, BS, D] cache -> [NB*BS, Hk, D] bytes on the CPU."""
    c = cache.view(torch.uint8) if cache.dtype == FP8 else cache
    return c.permute(0, 2, 1, 3).reshape(-1, c.shape[1], c.shape[3]).cpu()


def _check_append(cache, src, slots, head_scale):
    """head_scale: [Hk] or None."""
    got = _by_slot(cache)
    s = None if head_scale is None else head_scale.view(-1, 1)
    want = quantize_kv_fp8(src.cpu(), s).view(torch.uint8)
    assert torch.equal(got[slots], want)
    untouched = torch.ones(got.shape[0], dtype=torch.bool)
    untouched[slots] = False
    assert (got[untouched] == SENTINEL).all()


def _dequant(cache, head_scale):
    """FP8 [NB, Hkv, BS, D] -> the bf16 cache it denotes (exact)."""
    f = cache.float() * head_scale.view(1, -1, 1, 1)
    b = f.to(BF16)
    assert torch.equal(b.float(), f)
    return b


# ---------------------------------------------------------------------------
# Append
# ---------------------------------------------------------------------------

def _strided_kv(T, Hk, D, k_flat, v_flat):
    """k, v as row-strided views of one fused buffer (as the models pass)."""
    buf = torch.zeros(T, (2 * Hk + 1) * D, dtype=BF16)
    buf[:, : Hk * D] = k_flat.view(T, Hk * D)
    buf[:, (Hk + 1) * D :] = v_flat.view(T, Hk * D)
    buf = buf.to(DEV)
    k = buf[:, : Hk * D].view(T, Hk, D)
    v = buf[:, (Hk + 1) * D :].view(T, Hk, D)
    assert not k.is_contiguous() and not v.is_contiguous()
    return k, v


def test_kv_append_every_bf16_value_exact():
    T, Hk, D, NB = 64, 8, 128, 6
    g = _gen(0)
    vals = _all_non_nan_bf16()
    k = torch.zeros(T * Hk * D, dtype=BF16)
    k[: vals.numel()] = vals
    # every value meets every head's scale: rotate the heads per token
    k = k.view(T, Hk, D)
    v = k.flatten()[torch.randperm(k.numel(), generator=g)].view(T, Hk, D)
    slots = torch.randperm(NB * BS, generator=g)[:T]
    sc = _scales(Hk)
    for shift in range(0, Hk, 3):
        ks, vs = _strided_kv(T, Hk, D, k.roll(shift, 1).contiguous(), v.roll(shift, 1).contiguous())
        kc, vc = _sentinel_cache(NB, Hk, D), _sentinel_cache(NB, Hk, D)
        ext.kv_append(ks, vs, kc, vc, slots.to(DEV), sc.to(DEV))
        _check_append(kc, ks, slots, sc[0])
        _check_append(vc, vs, slots, sc[1])


@pytest.mark.parametrize("which", ["none", "ones"])
def test_append_none_and_ones_give_the_unscaled_bytes(which):
    T, Hk, D, NB = 64, 8, 128, 6
    g = _gen(1)
    vals = _all_non_nan_bf16()
    k = torch.zeros(T * Hk * D, dtype=BF16)
    k[: vals.numel()] = vals
    v = k[torch.randperm(k.numel(), generator=g)]
    k, v = _strided_kv(T, Hk, D, k, v)
    slots = torch.randperm(NB * BS, generator=g)[:T]
    sc = None if which == "none" else torch.ones(2, Hk, device=DEV)
    kc, vc = _sentinel_cache(NB, Hk, D), _sentinel_cache(NB, Hk, D)
    ext.kv_append(k, v, kc, vc, slots.to(DEV), sc)
    _check_append(kc, k, slots, None)
    _check_append(vc, v, slots, None)
    # the RoPE binding too (D=64 cache rows, positional and keyword form)
    T2, Hq, Hk2, D2, NB2 = 5, 4, 4, 64, 3
    qkv0 = (torch.randn(T2, (Hq + 2 * Hk2) * D2, generator=g) * 40).to(BF16)
    positions = torch.tensor([7, 3, 400, 0, 19], dtype=torch.long, device=DEV)
    cos, sin = torch_ref.build_rope_cache(D2, 512, 500000.0)
    slots2 = torch.randperm(NB2 * BS, generator=g)[:T2]
    sc2 = None if which == "none" else torch.ones(2, Hk2, device=DEV)
    qkv = qkv0.clone().to(DEV)
    q = qkv[:, : Hq * D2].view(T2, Hq, D2)
    k2 = qkv[:, Hq * D2 : (Hq + Hk2) * D2].view(T2, Hk2, D2)
    v2 = qkv[:, (Hq + Hk2) * D2 :].view(T2, Hk2, D2)
    kc2, vc2 = _sentinel_cache(NB2, Hk2, D2), _sentinel_cache(NB2, Hk2, D2)
    ext.rope_kv_append(
        q, k2, v2, positions, cos.to(DEV), sin.to(DEV), kc2, vc2, slots2.to(DEV),
        kv_scale=sc2,
    )
    _check_append(kc2, k2, slots2, None)  # k2 now holds the rotated values
    _check_append(vc2, v2, slots2, None)


def test_rope_kv_append_every_bf16_value_strided_views():
    """V goes straight through, so it carries every bf16 value; K is checked
    against the rotated bf16 values the call leaves in k (what a bf16 cache
    would hold)."""
    T, Hq, Hk, D, NB = 64, 8, 8, 128, 6
    g = _gen(2)
    vals = _all_non_nan_bf16()
    vflat = torch.zeros(T * Hk * D, dtype=BF16)
    vflat[: vals.numel()] = vals
    vflat = vflat[torch.randperm(vflat.numel(), generator=g)]
    u = torch.randint(-12, 10, (T, Hk * D), generator=g)
    qkv0 = torch.zeros(T, (Hq + 2 * Hk) * D, dtype=BF16)
    qkv0[:, : Hq * D] = torch.randn(T, Hq * D, generator=g).to(BF16)
    qkv0[:, Hq * D : (Hq + Hk) * D] = (
        torch.randn(T, Hk * D, generator=g) * 2.0**u
    ).to(BF16)
    qkv0[:, (Hq + Hk) * D :] = vflat.view(T, Hk * D)
    positions = torch.randint(0, 512, (T,), generator=g).to(DEV)
    cos, sin = torch_ref.build_rope_cache(D, 512, 500000.0)
    slots = torch.randperm(NB * BS, generator=g)[:T]
    sc = _scales(Hk)

    def run(kc, vc, scale):
        qkv = qkv0.clone().to(DEV)
        q = qkv[:, : Hq * D].view(T, Hq, D)
        k = qkv[:, Hq * D : (Hq + Hk) * D].view(T, Hk, D)
        v = qkv[:, (Hq + Hk) * D :].view(T, Hk, D)
        assert not k.is_contiguous()
        ext.rope_kv_append(
            q, k, v, positions, cos.to(DEV), sin.to(DEV), kc, vc, slots.to(DEV), scale
        )
        return qkv.cpu(), k.cpu(), v.cpu()

    kc16 = torch.zeros((NB, Hk, BS, D), dtype=BF16, device=DEV)
    vc16 = kc16.clone()
    qkv16, _, _ = run(kc16, vc16, None)
    kc8, vc8 = _sentinel_cache(NB, Hk, D), _sentinel_cache(NB, Hk, D)
    qkv8, k_rot, v_in = run(kc8, vc8, sc.to(DEV))
    # q, k after the call are bit-equal to the bf16-cache run's
    assert torch.equal(qkv16.view(torch.int16), qkv8.view(torch.int16))
    assert torch.equal(_by_slot(kc16)[slots].view(torch.int16), k_rot.view(torch.int16))
    _check_append(kc8, k_rot, slots, sc[0])
    _check_append(vc8, v_in, slots, sc[1])


# ---------------------------------------------------------------------------
# Decode
# ---------------------------------------------------------------------------

def _uniform_code_cache(shape, g):
    return _finite_codes()[torch.randint(0, 254, shape, generator=g)].view(FP8)


def _strided_q(T, Hq, D, g):
    buf = torch.randn(T, Hq * D + 2 * D, generator=g).to(BF16).to(DEV)
    q = buf[:, D : D + Hq * D].view(T, Hq, D)
    assert T == 1 or not q.is_contiguous()  # one row has no row stride
    return q


def _decode(q, kc, vc, bt, kvl, scale, kv_scale=None):
    out = torch.empty(q.shape, dtype=BF16, device=DEV)
    ext.attn_decode_paged(
        out, q, kc.to(DEV), vc.to(DEV), bt.to(DEV), kvl.to(DEV), scale,
        None if kv_scale is None else kv_scale.to(DEV),
    )
    return out.cpu().float()


def test_decode_selection_exact_with_scales():
    """The unit-scale selection test with two kv-heads of different scales:
    each query selects one key with a score margin of (16/ks)*(32*ks)/
    sqrt(128) = 45.25 whatever the K scale ks, so every other key weighs
    exp(-45.25) = 2.2e-20 or less; their worst-case sum, 253 * 2.2e-20 *
    448 * vs, cannot move a bf16 result by half an ulp of the smallest code
    (2^-9 * vs). A non-zero selected value comes back as exactly code * vs;
    a zero one is held to 1e-14 * vs."""
    D, G, Hkv, KV, B = 128, 4, 2, 254, 32
    sc = _scales(Hkv)
    codes = _finite_codes()
    n_pages = (KV + BS - 1) // BS
    j = torch.arange(n_pages * BS)
    NB = n_pages + 3
    perm = torch.randperm(NB, generator=_gen(20))[:n_pages]
    kc = torch.full((NB, Hkv, BS, D), SENTINEL, dtype=torch.uint8).view(FP8)
    vc = kc.clone()
    vrows = []
    for h in range(Hkv):
        vr = codes[((7 * j[:, None] + torch.arange(D)[None, :] + 31 * h) % 254)]
        krows = torch.zeros(n_pages * BS, D)
        krows[j, j % 128] = torch.where(j < 128, 32.0, -32.0)
        krows = quantize_kv_fp8(krows)  # the CODES are +-32: K = +-32 * ks
        kc.view(torch.uint8)[perm, h] = krows.view(torch.uint8).view(n_pages, BS, D)
        vc.view(torch.uint8)[perm, h] = vr.view(n_pages, BS, D)
        vrows.append(vr.view(FP8).float())
    bt = perm.to(torch.int32).repeat(B, 1)
    kvl = torch.full((B,), KV, dtype=torch.int32)
    key = (torch.arange(B * Hkv * G) * 3) % KV  # [B, Hkv, G] flattened
    q = torch.zeros(B * Hkv * G, D)
    q[torch.arange(q.shape[0]), key % 128] = torch.where(key < 128, 16.0, -16.0)
    head = (torch.arange(B * Hkv * G) // G) % Hkv
    q = q / sc[0][head].unsqueeze(-1)
    q = q.view(B, Hkv * G, D).to(BF16).to(DEV)
    got = _decode(q, kc, vc, bt, kvl, 1.0 / math.sqrt(D), sc).view(B * Hkv * G, D)
    for h in range(Hkv):
        rows = head == h
        want = vrows[h][key[rows]] * sc[1, h]
        g_h = got[rows]
        nz = want != 0
        assert nz.any() and (~nz).any()
        assert torch.equal(g_h[nz], want[nz])
        assert (g_h[~nz].abs() <= 1e-14 * sc[1, h]).all()


# a partial page, a page boundary, a partial second page, 7 pages over 7
# splits, and 34 pages over 8 splits (the last one empty)
@pytest.mark.parametrize("kv_lens", [(530,), (9, 16, 17), (100, 1, 33)])
@pytest.mark.parametrize("Hq,Hkv,D", CONFIGS)
def test_decode_matches_bf16_kernel_on_dequantised_cache(Hq, Hkv, D, kv_lens):
    g = _gen(11)
    B = len(kv_lens)
    max_blocks = (max(kv_lens) + BS - 1) // BS
    NB = B * max_blocks
    kc = _uniform_code_cache((NB, Hkv, BS, D), g)
    vc = _uniform_code_cache((NB, Hkv, BS, D), g)
    bt = torch.randperm(NB, generator=g).view(B, max_blocks).to(torch.int32)
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    q = _strided_q(B, Hq, D, g)
    scale = 1.0 / math.sqrt(D)
    sc = _scales(Hkv)
    got = _decode(q, kc, vc, bt, kvl, scale, sc)
    ref = _decode(q, _dequant(kc, sc[0]), _dequant(vc, sc[1]), bt, kvl, scale)
    assert torch.isfinite(ref).all()
    print(f"max abs diff {(got - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got, ref, atol=2e-2, rtol=2e-2)
    # all-ones scales are the unscaled kernel
    ones = _decode(q, kc, vc, bt, kvl, scale, torch.ones(2, Hkv))
    none = _decode(q, kc, vc, bt, kvl, scale)
    assert torch.equal(ones, none)


# ---------------------------------------------------------------------------
# Prefill
# ---------------------------------------------------------------------------

PREFILL_SEQS = ((40, 37), (0, 70))  # (cached prefix, chunk): 77 crosses a 64-key tile
PREFILL_CONFIGS = [(8, 2, 128), (4, 4, 64)]


def _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant, kv_scale=None):
    out = torch.empty(q.shape, dtype=BF16, device=DEV)
    ext.attn_prefill_paged(
        out, q, cu_q.to(DEV), q_pos.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV),
        kvl.to(DEV), scale, swz=variant,
        kv_scale=None if kv_scale is None else kv_scale.to(DEV),
    )
    return out.cpu()


@pytest.mark.parametrize("variant", [0, 4, 5])
@pytest.mark.parametrize("Hq,Hkv,D", PREFILL_CONFIGS)
def test_prefill_equals_same_variant_on_dequantised_cache(Hq, Hkv, D, variant):
    g = _gen(30)
    kv_lens = [p + c for p, c in PREFILL_SEQS]
    q_lens = [c for _, c in PREFILL_SEQS]
    P = len(kv_lens)
    max_blocks = (max(kv_lens) + BS - 1) // BS
    NB = P * max_blocks + 2
    kc = _uniform_code_cache((NB, Hkv, BS, D), g)
    vc = _uniform_code_cache((NB, Hkv, BS, D), g)
    bt = torch.randperm(NB, generator=g)[: P * max_blocks].view(P, max_blocks)
    bt = bt.to(torch.int32)
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    cu_q = torch.tensor([0, q_lens[0], sum(q_lens)], dtype=torch.int32)
    q_pos = torch.cat(
        [torch.arange(p, p + c, dtype=torch.long) for p, c in PREFILL_SEQS]
    )
    q = _strided_q(sum(q_lens), Hq, D, g)
    scale = 1.0 / math.sqrt(D)
    sc = _scales(Hkv)
    got = _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant, sc)
    ref = _prefill(
        q, cu_q, q_pos, _dequant(kc, sc[0]), _dequant(vc, sc[1]), bt, kvl, scale, variant
    )
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    # and it is not the unscaled result
    assert not torch.equal(got, _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant))


@pytest.mark.parametrize("variant", [0, 4, 5])
def test_prefill_tile_load_every_code_times_scale(variant):
    """Pins the scale operand of the converting tile load. Sequences of one
    key and one query: p = 1 and l = 1 exactly, so out = V row as LDS holds
    it. Three kv-heads with V scales 2^-9, 2^-1, 2^3 (K scales differ), two
    sequences whose rows cover the 254 finite codes."""
    Hkv, D = 3, 128
    sc = torch.tensor([[2.0**4, 2.0**-6, 2.0**1], [2.0**-9, 2.0**-1, 2.0**3]])
    codes = _finite_codes()
    rows = torch.stack([codes[:128], codes[126:]])  # [2, 128]
    NB = 4
    vc = torch.full((NB, Hkv, BS, D), SENTINEL, dtype=torch.uint8)
    kc = _uniform_code_cache((NB, Hkv, BS, D), _gen(40))
    blocks = [3, 1]
    for s, b in enumerate(blocks):
        for h in range(Hkv):
            vc[b, h, 0] = rows[s].roll(h)  # a different row per head
    vc = vc.view(FP8)
    bt = torch.tensor(blocks, dtype=torch.int32).view(2, 1)
    kvl = torch.tensor([1, 1], dtype=torch.int32)
    cu_q = torch.tensor([0, 1, 2], dtype=torch.int32)
    q_pos = torch.zeros(2, dtype=torch.long)
    q = _strided_q(2, Hkv, D, _gen(41))
    got = _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, 0.1, variant, sc).float()
    seen = set()
    for s in range(2):
        for h in range(Hkv):
            row = rows[s].roll(h)
            want = row.view(FP8).float() * sc[1, h]
            assert torch.equal(got[s, h], want), (s, h)
            seen |= set(row.tolist())
    assert seen == set(codes.tolist())


# ---------------------------------------------------------------------------
# What the scales buy, on the kernels
# ---------------------------------------------------------------------------

N_KEYS = 300


def _recipe(kind, Hq, Hkv, D):
    g = _gen(7)
    q = torch.randn(1, Hq, D, generator=g)
    k = torch.randn(N_KEYS, Hkv, D, generator=g)
    v = torch.randn(N_KEYS, Hkv, D, generator=g)
    if kind == "outlier":  # one K channel reaching 4300: saturates at 448
        ch = torch.randn(N_KEYS, Hkv, generator=g)
        k[:, :, 5] = ch / ch.abs().max() * 4300.0
        q[:, :, 5] = torch.randn(1, Hq, generator=g) * 0.01
    else:  # V of std 0.004: subnormal and zero codes at unit scale
        v = v * 0.004
    return q.to(BF16), k.to(BF16), v.to(BF16)


@pytest.mark.parametrize("kind", ["outlier", "tiny_v"])
def test_calibrated_scales_at_least_halve_the_kernel_error(kind):
    Hq, Hkv, D = 8, 2, 128
    q, k, v = _recipe(kind, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    exact = torch_ref._sdpa(q.float(), k.float(), v.float(), scale)
    n_blocks = (N_KEYS + BS - 1) // BS
    bt = torch.arange(n_blocks, dtype=torch.int32).unsqueeze(0)
    kvl = torch.tensor([N_KEYS], dtype=torch.int32)
    amax = torch.stack([k.float().abs().amax(dim=(0, 2)), v.float().abs().amax(dim=(0, 2))])
    calibrated = scales_from_amax(amax, headroom=2.0)
    # the query as the last position of a prefill over the same cache
    cu_q = torch.tensor([0, 1], dtype=torch.int32)
    q_pos = torch.tensor([N_KEYS - 1], dtype=torch.long)
    errs = {}
    for name, sc in (("unit", None), ("calibrated", calibrated)):
        kc, vc = _sentinel_cache(n_blocks, Hkv, D), _sentinel_cache(n_blocks, Hkv, D)
        ext.kv_append(
            k.to(DEV), v.to(DEV), kc, vc, torch.arange(N_KEYS, device=DEV),
            None if sc is None else sc.to(DEV),
        )
        outs = {"decode": _decode(q.to(DEV), kc, vc, bt, kvl, scale, sc)}
        for variant in (0, 5):
            outs[f"prefill{variant}"] = _prefill(
                q.to(DEV), cu_q, q_pos, kc, vc, bt, kvl, scale, variant, sc
            ).float()
        for kern, out in outs.items():
            errs[name, kern] = ((out - exact).norm() / exact.norm()).item()
    print(kind, {f"{a}/{b}": round(e, 4) for (a, b), e in errs.items()})
    for kern in ("decode", "prefill0", "prefill5"):
        assert errs["calibrated", kern] <= 0.5 * errs["unit", kern]


# ---------------------------------------------------------------------------
# Host-side checks: nothing is launched
# ---------------------------------------------------------------------------

class TestRejected:
    Hq, Hkv, D, NB = 8, 2, 128, 2

    def _args(self, dtype):
        q = torch.zeros(4, self.Hq, self.D, dtype=BF16, device=DEV)
        kc = torch.zeros(self.NB, self.Hkv, BS, self.D, dtype=dtype).to(DEV)
        vc = kc.clone()
        cu_q = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
        q_pos = torch.arange(4, dtype=torch.long, device=DEV)
        bt = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
        kvl = torch.tensor([4], dtype=torch.int32, device=DEV)
        return torch.empty_like(q), q, cu_q, q_pos, kc, vc, bt, kvl, 0.1

    def _all_four(self, dtype, sc, match):
        out, q, cu_q, q_pos, kc, vc, bt, kvl, scale = self._args(dtype)
        k = torch.zeros(4, self.Hkv, self.D, dtype=BF16, device=DEV)
        slots = torch.arange(4, dtype=torch.long, device=DEV)
        cos, sin = torch_ref.build_rope_cache(self.D, 8, 10000.0)
        with pytest.raises(RuntimeError, match=match):
            ext.attn_prefill_paged(out, q, cu_q, q_pos, kc, vc, bt, kvl, scale, kv_scale=sc)
        with pytest.raises(RuntimeError, match=match):
            ext.attn_decode_paged(out[:1], q[:1], kc, vc, bt, kvl, scale, sc)
        with pytest.raises(RuntimeError, match=match):
            ext.kv_append(k, k.clone(), kc, vc, slots, sc)
        with pytest.raises(RuntimeError, match=match):
            ext.rope_kv_append(
                q, k, k.clone(), slots, cos.to(DEV), sin.to(DEV), kc, vc, slots, sc
            )
        assert not kc.view(torch.uint8).any() and not vc.view(torch.uint8).any()

    def test_scale_with_bf16_cache_raises(self):
        self._all_four(BF16, torch.ones(2, self.Hkv, device=DEV), "FP8")

    def test_wrong_shape_raises(self):
        self._all_four(FP8, torch.ones(self.Hkv, 2, 1, device=DEV), r"\[2, Hkv\]")
        self._all_four(FP8, torch.ones(2, self.Hkv + 1, device=DEV), r"\[2, Hkv\]")
        self._all_four(FP8, torch.ones(2 * self.Hkv, device=DEV), r"\[2, Hkv\]")

    def test_wrong_dtype_raises(self):
        self._all_four(FP8, torch.ones(2, self.Hkv, device=DEV, dtype=BF16), "float32")

    def test_non_contiguous_or_host_scale_raises(self):
        self._all_four(FP8, torch.ones(self.Hkv, 2, device=DEV).t(), "contiguous")
        self._all_four(FP8, torch.ones(2, self.Hkv), "device")
