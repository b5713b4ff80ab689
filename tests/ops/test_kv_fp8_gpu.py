"""FP8 (e4m3fn, scale 1.0) paged KV cache on the GPU: append, decode and
prefill attention.

The store is pinned byte for byte against torch_ref.quantize_kv_fp8 over
every bf16 value. The load is pinned exactly where the arithmetic allows it
(a decode that selects one key per query, prefill against the same kernel on
the dequantised cache) and held to the existing bf16 tolerances against
torch_ref elsewhere. Shapes are the smallest that cover every (G, D)
instantiation, a partial page, a page boundary, more than one split and a
chunk that crosses a 64-key tile.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader, torch_ref

ext = _hip_ext_loader.load()
quantize_kv_fp8 = torch_ref.quantize_kv_fp8  # the specification of the store

DEV = "cuda:0"
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
BS = 16
SENTINEL = 0x55
CONFIGS = [(8, 2, 128), (8, 1, 128), (2, 2, 128), (4, 4, 64)]  # Hq, Hkv, D


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


def _check_append(cache, src, slots):
    got = _by_slot(cache)
    want = quantize_kv_fp8(src.cpu()).view(torch.uint8)
    assert torch.equal(got[slots], want)
    untouched = torch.ones(got.shape[0], dtype=torch.bool)
    untouched[slots] = False
    assert (got[untouched] == SENTINEL).all()


# ---------------------------------------------------------------------------
# Append
# ---------------------------------------------------------------------------

def test_kv_append_every_bf16_value_exact():
    T, Hk, D, NB = 64, 8, 128, 6
    g = _gen(0)
    vals = _all_non_nan_bf16()
    k = torch.zeros(T * Hk * D, dtype=BF16)
    k[: vals.numel()] = vals
    v = k[torch.randperm(k.numel(), generator=g)]
    k, v = k.view(T, Hk, D).to(DEV), v.view(T, Hk, D).to(DEV)
    slots = torch.randperm(NB * BS, generator=g)[:T]
    kc, vc = _sentinel_cache(NB, Hk, D), _sentinel_cache(NB, Hk, D)
    ext.kv_append(k, v, kc, vc, slots.to(DEV))
    _check_append(kc, k, slots)
    _check_append(vc, v, slots)


def test_kv_append_d64():
    T, Hk, D, NB = 64, 4, 64, 6
    g = _gen(1)
    u = torch.randint(-10, 10, (T, Hk, D), generator=g)
    k = (torch.randn(T, Hk, D, generator=g) * 2.0**u).to(BF16).to(DEV)
    v = (torch.randn(T, Hk, D, generator=g) * 2.0**u).to(BF16).to(DEV)
    slots = torch.randperm(NB * BS, generator=g)[:T]
    kc, vc = _sentinel_cache(NB, Hk, D), _sentinel_cache(NB, Hk, D)
    ext.kv_append(k, v, kc, vc, slots.to(DEV))
    _check_append(kc, k, slots)
    _check_append(vc, v, slots)


def test_rope_kv_append_strided_views_matches_bf16_cache():
    T, Hq, Hk, D, NB = 5, 8, 2, 128, 3
    g = _gen(2)
    qkv0 = (torch.randn(T, (Hq + 2 * Hk) * D, generator=g) * 4).to(BF16)
    positions = torch.tensor([7, 3, 400, 0, 19], dtype=torch.long, device=DEV)
    cos, sin = torch_ref.build_rope_cache(D, 512, 500000.0)
    cos, sin = cos.to(DEV), sin.to(DEV)
    slots = torch.randperm(NB * BS, generator=g)[:T]

    def run(kc, vc):
        qkv = qkv0.clone().to(DEV)
        q = qkv[:, : Hq * D].view(T, Hq, D)
        k = qkv[:, Hq * D : (Hq + Hk) * D].view(T, Hk, D)
        v = qkv[:, (Hq + Hk) * D :].view(T, Hk, D)
        assert not k.is_contiguous()
        ext.rope_kv_append(q, k, v, positions, cos, sin, kc, vc, slots.to(DEV))
        return qkv.cpu()

    bf_sentinel = torch.tensor(-3.0, dtype=BF16)
    kc16 = torch.full((NB, Hk, BS, D), bf_sentinel.item(), dtype=BF16, device=DEV)
    vc16 = kc16.clone()
    qkv16 = run(kc16, vc16)
    kc8, vc8 = _sentinel_cache(NB, Hk, D), _sentinel_cache(NB, Hk, D)
    qkv8 = run(kc8, vc8)

    # q and k after the call (and the untouched v) are bit-equal
    assert torch.equal(qkv16.view(torch.int16), qkv8.view(torch.int16))
    assert not torch.equal(qkv16, qkv0)  # the rotation did happen
    untouched = torch.ones(NB * BS, dtype=torch.bool)
    untouched[slots] = False
    for c16, c8 in ((kc16, kc8), (vc16, vc8)):
        s16, s8 = _by_slot(c16), _by_slot(c8)
        assert torch.equal(s8[slots], quantize_kv_fp8(s16[slots]).view(torch.uint8))
        assert (s8[untouched] == SENTINEL).all()
        assert (s16[untouched] == bf_sentinel).all()


# ---------------------------------------------------------------------------
# Decode
# ---------------------------------------------------------------------------

# the first key alone, a full page, a partial second page, 7 pages over 7
# splits, and 34 pages: 5 per split over splits 0..5, 4 in split 6, and an
# empty split 7 (the -inf partial the combine must skip)
KV_LENS = (1, 16, 17, 100, 530)


def _randn_pow2_cache(shape, g):
    """quantize(randn * 2^u), u per element in [-8, 3]: subnormal and large
    codes both occur."""
    u = torch.randint(-8, 4, shape, generator=g)
    return quantize_kv_fp8(torch.randn(shape, generator=g) * 2.0**u)


def _uniform_code_cache(shape, g):
    return _finite_codes()[torch.randint(0, 254, shape, generator=g)].view(FP8)


def _strided_q(T, Hq, D, g):
    buf = torch.randn(T, Hq * D + 2 * D, generator=g).to(BF16).to(DEV)
    q = buf[:, D : D + Hq * D].view(T, Hq, D)
    assert not q.is_contiguous()
    return q


def _decode_case(Hq, Hkv, D, make_cache, seed):
    g = _gen(seed)
    B = len(KV_LENS)
    max_blocks = (max(KV_LENS) + BS - 1) // BS
    NB = B * max_blocks
    kc = make_cache((NB, Hkv, BS, D), g)
    vc = make_cache((NB, Hkv, BS, D), g)
    bt = torch.randperm(NB, generator=g).view(B, max_blocks).to(torch.int32)
    kvl = torch.tensor(KV_LENS, dtype=torch.int32)
    q = _strided_q(B, Hq, D, g)
    return q, kc, vc, bt, kvl, 1.0 / math.sqrt(D)


def _decode(q, kc, vc, bt, kvl, scale):
    out = torch.empty(q.shape, dtype=BF16, device=DEV)
    ext.attn_decode_paged(out, q, kc.to(DEV), vc.to(DEV), bt.to(DEV), kvl.to(DEV), scale)
    return out.cpu().float()


@pytest.mark.parametrize("Hq,Hkv,D", CONFIGS)
def test_decode_matches_reference(Hq, Hkv, D):
    q, kc, vc, bt, kvl, scale = _decode_case(Hq, Hkv, D, _randn_pow2_cache, 10)
    ref = torch_ref.attn_decode_paged(q.cpu().float(), kc, vc, bt, kvl, scale)
    got = _decode(q, kc, vc, bt, kvl, scale)
    print(f"max abs diff {(got - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got, ref, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("Hq,Hkv,D", CONFIGS)
def test_decode_matches_bf16_kernel(Hq, Hkv, D):
    """Every finite code, uniformly: a wrong K code changes which key wins
    the softmax. Not bit equality — the compiler may contract the fp32 sums
    of the two instantiations differently."""
    q, kc, vc, bt, kvl, scale = _decode_case(Hq, Hkv, D, _uniform_code_cache, 11)
    got = _decode(q, kc, vc, bt, kvl, scale)
    ref = _decode(q, kc.to(BF16), vc.to(BF16), bt, kvl, scale)
    assert torch.isfinite(ref).all()
    print(f"max abs diff {(got - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got, ref, atol=2e-2, rtol=2e-2)


def test_decode_selection_exact():
    """Each of 256 queries selects one of the 254 keys with a score margin
    of 16*32/sqrt(128) = 45.25, so every other key weighs exp(-45.25) =
    2.2e-20 or less. Their worst-case sum, 253 * 2.2e-20 * 448 = 2.5e-15,
    cannot move a bf16 result by half an ulp even for the smallest code
    (2^-9, half an ulp 2^-18), so a non-zero selected value must come back
    exactly. Where the selected code is +-0 the same sum is all there is: it
    is held to 1e-14 instead of to equality with zero."""
    D, G, Hkv, KV, B = 128, 4, 1, 254, 64
    codes = _finite_codes()
    n_pages = (KV + BS - 1) // BS
    j = torch.arange(n_pages * BS)
    vrows = codes[((7 * j[:, None] + torch.arange(D)[None, :]) % 254)].view(FP8)
    krows = torch.zeros(n_pages * BS, D)
    krows[j, j % 128] = torch.where(j < 128, 32.0, -32.0)
    krows = quantize_kv_fp8(krows)
    NB = n_pages + 3
    perm = torch.randperm(NB, generator=_gen(20))[:n_pages]
    kc = torch.full((NB, Hkv, BS, D), SENTINEL, dtype=torch.uint8).view(FP8)
    vc = kc.clone()
    kc.view(torch.uint8)[perm, 0] = krows.view(torch.uint8).view(n_pages, BS, D)
    vc.view(torch.uint8)[perm, 0] = vrows.view(torch.uint8).view(n_pages, BS, D)
    bt = perm.to(torch.int32).repeat(B, 1)
    kvl = torch.full((B,), KV, dtype=torch.int32)
    key = torch.arange(B * G) % KV
    q = torch.zeros(B * G, D)
    q[torch.arange(B * G), key % 128] = torch.where(key < 128, 16.0, -16.0)
    q = q.view(B, G, D).to(BF16).to(DEV)
    got = _decode(q, kc, vc, bt, kvl, 1.0 / math.sqrt(D)).view(B * G, D)
    want = vrows.float()[key]
    assert set(vrows.view(torch.uint8)[:KV].flatten().tolist()) == set(codes.tolist())
    nz = want != 0
    assert torch.equal(got[nz], want[nz])
    assert (got[~nz].abs() <= 1e-14).all()


# ---------------------------------------------------------------------------
# Prefill
# ---------------------------------------------------------------------------

PREFILL_SEQS = ((40, 37), (0, 70))  # (cached prefix, chunk)
PREFILL_CONFIGS = [(8, 2, 128), (4, 4, 64)]


def _prefill_case(Hq, Hkv, D, make_cache, seed):
    g = _gen(seed)
    kv_lens = [p + c for p, c in PREFILL_SEQS]
    q_lens = [c for _, c in PREFILL_SEQS]
    P = len(kv_lens)
    max_blocks = (max(kv_lens) + BS - 1) // BS
    NB = P * max_blocks + 2
    kc = make_cache((NB, Hkv, BS, D), g)
    vc = make_cache((NB, Hkv, BS, D), g)
    bt = torch.randperm(NB, generator=g)[: P * max_blocks].view(P, max_blocks)
    bt = bt.to(torch.int32)
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    cu_q = torch.tensor([0, q_lens[0], sum(q_lens)], dtype=torch.int32)
    q_pos = torch.cat(
        [torch.arange(p, p + c, dtype=torch.long) for p, c in PREFILL_SEQS]
    )
    q = _strided_q(sum(q_lens), Hq, D, g)
    return q, cu_q, q_pos, kc, vc, bt, kvl, 1.0 / math.sqrt(D)


def _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant):
    out = torch.empty(q.shape, dtype=BF16, device=DEV)
    ext.attn_prefill_paged(
        out, q, cu_q.to(DEV), q_pos.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV),
        kvl.to(DEV), scale, swz=variant,
    )
    return out.cpu()


@pytest.mark.parametrize("variant", [0, 4, 5])
@pytest.mark.parametrize("Hq,Hkv,D", PREFILL_CONFIGS)
def test_prefill_equals_same_variant_on_bf16_cache(Hq, Hkv, D, variant):
    """The converted tile in LDS is the bf16 tile and the code after the
    load is the same: bit equality, over uniformly random finite codes."""
    q, cu_q, q_pos, kc, vc, bt, kvl, scale = _prefill_case(
        Hq, Hkv, D, _uniform_code_cache, 30
    )
    got = _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant)
    ref = _prefill(q, cu_q, q_pos, kc.to(BF16), vc.to(BF16), bt, kvl, scale, variant)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("variant", [0, 4, 5])
@pytest.mark.parametrize("Hq,Hkv,D", PREFILL_CONFIGS)
def test_prefill_matches_reference(Hq, Hkv, D, variant):
    q, cu_q, q_pos, kc, vc, bt, kvl, scale = _prefill_case(
        Hq, Hkv, D, _randn_pow2_cache, 31
    )
    ref = torch_ref.attn_prefill_paged(
        q.cpu().float(), cu_q, q_pos, kc, vc, bt, kvl, scale
    )
    got = _prefill(q, cu_q, q_pos, kc, vc, bt, kvl, scale, variant).float()
    print(f"max abs diff {(got - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got, ref, atol=2.5e-2, rtol=2.5e-2)


# ---------------------------------------------------------------------------
# Host-side checks: nothing is launched
# ---------------------------------------------------------------------------

class TestRejected:
    Hq, Hkv, D, NB = 8, 2, 128, 2

    def _prefill_args(self, kdt, vdt):
        q = torch.zeros(4, self.Hq, self.D, dtype=BF16, device=DEV)
        kc = torch.zeros(self.NB, self.Hkv, BS, self.D, dtype=kdt).to(DEV)
        vc = torch.zeros(self.NB, self.Hkv, BS, self.D, dtype=vdt).to(DEV)
        cu_q = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
        q_pos = torch.arange(4, dtype=torch.long, device=DEV)
        bt = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
        kvl = torch.tensor([4], dtype=torch.int32, device=DEV)
        return torch.empty_like(q), q, cu_q, q_pos, kc, vc, bt, kvl, 0.1

    @pytest.mark.parametrize("variant", [1, 2, 3])
    def test_ablation_variants_reject_fp8(self, variant):
        with pytest.raises(RuntimeError, match="FP8"):
            ext.attn_prefill_paged(*self._prefill_args(FP8, FP8), swz=variant)

    @pytest.mark.parametrize("kdt,vdt", [(FP8, BF16), (BF16, FP8)])
    def test_mixed_dtypes_raise(self, kdt, vdt):
        out, q, cu_q, q_pos, kc, vc, bt, kvl, scale = self._prefill_args(kdt, vdt)
        with pytest.raises(RuntimeError, match="same dtype"):
            ext.attn_prefill_paged(out, q, cu_q, q_pos, kc, vc, bt, kvl, scale)
        with pytest.raises(RuntimeError, match="same dtype"):
            ext.attn_decode_paged(out[:1], q[:1], kc, vc, bt, kvl, scale)
        k = torch.zeros(4, self.Hkv, self.D, dtype=BF16, device=DEV)
        slots = torch.arange(4, dtype=torch.long, device=DEV)
        with pytest.raises(RuntimeError, match="same dtype"):
            ext.kv_append(k, k.clone(), kc, vc, slots)
        cos, sin = torch_ref.build_rope_cache(self.D, 8, 10000.0)
        with pytest.raises(RuntimeError, match="same dtype"):
            ext.rope_kv_append(
                q, k, k.clone(), slots, cos.to(DEV), sin.to(DEV), kc, vc, slots
            )
        assert not kc.view(torch.uint8).any() and not vc.view(torch.uint8).any()

    def test_other_cache_dtype_raises(self):
        out, q, cu_q, q_pos, kc, vc, bt, kvl, scale = self._prefill_args(
            torch.float16, torch.float16
        )
        with pytest.raises(RuntimeError, match="bfloat16 or float8_e4m3fn"):
            ext.attn_decode_paged(out[:1], q[:1], kc, vc, bt, kvl, scale)
