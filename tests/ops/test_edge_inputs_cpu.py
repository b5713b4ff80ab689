"""The constructions of tests/ops/_edge_inputs.py, proven on the reference
alone: every builder runs through torch_ref or fp64 here and the properties
the GPU tests rely on are asserted (selection exact, causal probes exact and
sensitive to a shifted mask, integer sums <= 256, nucleus stable in top_p,
the fp32 references inside one bf16 ulp of fp64)."""

import pytest
import torch

from dts_amd.ops import torch_ref
from tests.ops import _edge_inputs as E

BF16 = torch.bfloat16


# ---------------------------------------------------------------------------
# ulp measure
# ---------------------------------------------------------------------------

def test_bf16_ulp_is_the_format_spacing():
    r = torch.tensor([1.0, 1.99, 2.0, 0.75, -3.0, 100.0, 2.0**-126, 1e-40, 0.0])
    want = torch.tensor(
        [2.0**-7, 2.0**-7, 2.0**-6, 2.0**-8, 2.0**-6, 2.0**-1]
        + [2.0**-133] * 3, dtype=torch.float64,
    )
    assert torch.equal(E.bf16_ulp(r.double()), want)
    # one bf16 step from a power of two is one ulp up, half an ulp down
    one = torch.tensor([1.0], dtype=BF16)
    up = (E.bits(one) + 1).view(BF16)
    assert E.ulp_err(up, one.double()) == 1.0


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("T,H", E.NORM_SHAPES)
def test_norm_references_within_one_ulp(T, H):
    x, r, w = E.norm_inputs(T, H)
    err = E.ulp_err(torch_ref.rmsnorm(x, w, E.EPS), E.rmsnorm64(x, w))
    s = E.add_residual(x, r)
    y, new_r = torch_ref.fused_add_rmsnorm(x, r, w, E.EPS)
    err_f = E.ulp_err(y, E.rmsnorm64(s, w))
    print(f"rmsnorm {err:.5f} ulp, fused {err_f:.5f} ulp")
    assert torch.equal(new_r, s)
    assert err <= 1.0 and err_f <= 1.0


def _layernorm_reference_err(T, H, mean):
    x, w, b = E.layernorm_inputs(T, H, mean)
    assert torch.equal(x.double().mean(dim=1), torch.full((T,), mean).double())
    ref = E.layernorm64(x, w, b)
    err = E.ulp_err(torch_ref.layernorm(x, w, b, E.EPS), ref)
    print(f"layernorm ({T}, {H}) mean={mean} {err:.5f} ulp")
    return x, w, b, ref, err


@pytest.mark.parametrize("T,H", E.NORM_SHAPES)
def test_layernorm_reference_within_one_ulp(T, H):
    assert _layernorm_reference_err(T, H, 0.0)[-1] <= 1.0


def test_layernorm_mean_100_needs_the_two_pass_form():
    mean = E.LN_OFFSET_MEAN
    x, w, b, ref, err = _layernorm_reference_err(*E.LN_OFFSET_SHAPE, mean)
    assert err <= 1.0
    assert (x.double().std(dim=1) - 1).abs().max() < 0.1
    # the one-pass variance E[x^2] - mean^2 loses digits at this mean even
    # with torch's pairwise fp32 sums; the two-pass form does not
    xf = x.float()
    var1 = xf.pow(2).mean(dim=1, keepdim=True) - xf.mean(dim=1, keepdim=True) ** 2
    bad = ((xf - mean) * torch.rsqrt(var1 + E.EPS) * w.float() + b.float()).to(BF16)
    print(f"one-pass variance: {E.ulp_err(bad, ref):.3f} ulp")
    assert E.ulp_err(bad, ref) > err + 0.1


def test_silu_builders():
    gu = E.silu_exhaustive_inputs()
    assert gu.shape == (512, 1024)
    g, u = gu.chunk(2, dim=-1)
    pairs = torch.stack([E.bits(g).flatten().int() & 0xFFFF, E.bits(u).flatten().int()])
    assert pairs.unique(dim=1).shape[1] == 4 * 65536
    ref, finite, nan, inf, zero, zero_bits = E.silu_expectation(gu)
    assert finite.sum() > 190000 and nan.any() and inf.any() and zero.any()
    got = torch_ref.silu_mul(gu)  # torch's fp32 silu
    err = E.ulp_err(got[finite], ref[finite])
    print(f"silu_mul exhaustive {err:.5f} ulp on {int(finite.sum())} finite")
    assert err <= 1.0
    assert torch.isnan(got[nan].float()).all()
    assert torch.equal(got[inf].float(), ref[inf].float().to(BF16).float())
    assert torch.equal(E.bits(got)[zero], zero_bits[zero])
    assert set(zero_bits[zero].tolist()) == {0, -32768}
    sweep = E.silu_sweep_inputs()
    assert E.ulp_err(torch_ref.silu_mul(sweep), E.silu_mul64(sweep)) <= 1.0


# ---------------------------------------------------------------------------
# rope + append
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("Hq,Hk", E.ROPE_HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_rope_reference_within_bound(D, Hq, Hk):
    fused, pos, cos, sin, slots = E.rope_inputs(D, Hq, Hk)
    assert slots.unique().numel() == E.ROPE_T and slots.max() < E.ROPE_BLOCKS * E.BS
    q, k, v = E.split_qkv(fused.clone(), Hq, Hk, D)
    assert not q.is_contiguous() and not v.is_contiguous() or Hq + 2 * Hk == 1
    rq, rk = torch_ref.rope_apply(q, k, pos, cos, sin)
    for got, x in ((rq, q), (rk, k)):
        ref, slack = E.rope64(x, pos, cos, sin)
        err = E.ulp_err(got, ref, slack)
        print(f"rope {err:.5f} ulp over the cancellation slack")
        assert err <= 1.0
    kc, vc = E.sentinel_cache(Hk, D), E.sentinel_cache(Hk, D)
    torch_ref.kv_append(rk, v, kc, vc, slots)
    assert torch.equal(E.cache_rows(vc, slots), v)
    assert torch.equal(E.cache_rows(kc, slots), rk)
    for c in (kc, vc):
        rest = E.untouched_rows(c, slots)
        assert rest.shape[0] == E.ROPE_BLOCKS * E.BS - E.ROPE_T
        assert (rest == E.SENTINEL).all()
    assert not (fused == E.SENTINEL).any()


# ---------------------------------------------------------------------------
# decode selection
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("Hq,Hkv,D", E.DECODE_CONFIGS)
def test_decode_selection_reference_exact(Hq, Hkv, D):
    q, kc, vc, bt, kvl, scale, want = E.decode_selection_inputs(Hq, Hkv, D)
    assert 16 * 32 * scale >= 45.25 and E.SEL_PAGES == 33
    assert not q.is_contiguous() and q.stride(1) == D
    assert bt.unique().numel() == bt.numel() < kc.shape[0]
    for lens in (kvl, E.selection_short_lens(Hq, q.shape[0])):
        got = torch_ref.attn_decode_paged(q, kc, vc, bt, lens, scale)
        assert (got.float() - want.float()).abs().max() == 0
    # the poisoned caches differ from the clean ones only in dead slots
    for lens in (kvl, E.guard_lens(q.shape[0])):
        kp, vp = E.poison_dead(kc, vc, bt, lens)
        live = E.live_slots(kc.shape[0], bt, lens).view(-1, 1, E.BS, 1)
        assert torch.equal(torch.isnan(kp.float()), ~live.expand_as(kp))
        assert torch.equal(torch.isnan(vp.float()), ~live.expand_as(vp))
        assert int(live.sum()) == int(lens.sum())


def test_decode_fp8_poison_is_nan_code():
    g = E.gen(1)
    B, Hkv, D = 4, 2, 128
    W = E.SEL_PAGES + E.SEL_SPARE
    bt = torch.randperm(B * W + 3, generator=g)[: B * W].view(B, W).to(torch.int32)
    kc = E.uniform_code_cache((B * W + 3, Hkv, E.BS, D), g)
    assert torch.isfinite(kc.float()).all()
    lens = E.guard_lens(B)
    kp, vp = E.poison_dead(kc, kc, bt, lens)
    live = E.live_slots(kc.shape[0], bt, lens).view(-1, 1, E.BS, 1).expand_as(kp)
    assert (kp.view(torch.uint8)[~live] == 0x7F).all()
    assert torch.equal(kp.view(torch.uint8)[live], kc.view(torch.uint8)[live])


# ---------------------------------------------------------------------------
# prefill causal probes
# ---------------------------------------------------------------------------

def test_probe_positions_cover_every_boundary():
    assert E.probe_positions(0, 70) == [0, 15, 16, 31, 32, 47, 48, 63, 64, 69]
    assert E.probe_positions(40, 37) == [40, 47, 48, 63, 64, 76]
    assert E.probe_positions(130, 16) == [130, 143, 144, 145]
    assert E.probe_positions(63, 2) == [63, 64]


@pytest.mark.parametrize("G,D", E.PREFILL_GD)
def test_prefill_probes_reference_exact_and_mask_sensitive(G, D):
    q, cu_q, q_pos, kc, vc, bt, kvl, scale, probes = E.prefill_probe_inputs(G, D)
    assert len(probes) == 2 * 22
    out = torch_ref.attn_prefill_paged(q, cu_q, q_pos, kc, vc, bt, kvl, scale)
    shifted = torch_ref.attn_prefill_paged(q, cu_q, q_pos + 1, kc, vc, bt, kvl, scale)
    n_sensitive = 0
    for row, head, v, s, p in probes:
        assert torch.equal(out[row, head], v)
        if p + 1 < int(kvl[s]):
            # one position too many and the +64 key takes over
            assert not torch.equal(shifted[row, head], v)
            n_sensitive += 1
        else:
            # the tempting key of a sequence's last position sits in slot
            # kv_len of the last page: a live address past kv_len
            blk = int(bt[s, (p + 1) // E.BS])
            assert kc[blk, :, (p + 1) % E.BS].float().abs().max() == 64.0
    assert n_sensitive == len(probes) - 2 * len(E.PREFILL_SEQS)
    assert torch.isfinite(out.float()).all()


# ---------------------------------------------------------------------------
# exact GEMMs
# ---------------------------------------------------------------------------

def test_ternary_sums_stay_exact():
    for K in (512, 1536, 2048):
        x, w, want = E.gemm_inputs(16, 272, K)
        assert set(x.float().unique().tolist()) == {-1.0, 0.0, 1.0}
        print(f"K={K} max |sum| {want.float().abs().max().item():.0f}")
        assert want.float().abs().max() <= 256
        assert torch.equal((x.float() @ w.float().T).to(BF16), want)
    xs = E.strided_rows(x)
    assert torch.equal(xs, x) and xs.stride(0) == x.shape[1] + 16
    assert xs.storage_offset() * 2 % 16 == 0 and xs.stride(0) * 2 % 16 == 0


def test_moe_builder_matches_reference_and_leaves_a_gap():
    x, w, counts, offsets, want, gap = E.moe_inputs()
    assert counts.tolist() == [0, 1, 15, 16, 17, 33, 0, 5] and len(gap) == 3
    ref = torch_ref.moe_grouped_linear(x, w, counts, offsets)
    owned = torch.ones(x.shape[0], dtype=torch.bool)
    owned[gap] = False
    assert torch.equal(ref[owned], want[owned])
    assert (want[gap] == E.SENTINEL).all() and not (want[owned] == E.SENTINEL).any()


# ---------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("V", sorted(set(E.V1_VOCABS + E.V2_VOCABS)))
def test_sampler_builders(V):
    x, idx = E.boundary_logits(V)
    assert torch.equal(torch.argmax(x, dim=1), idx)
    for r in range(0, E.SAMPLER_ROWS, 5):
        ids, _ = E.reference_nucleus(x[r], 1.0, 0.5)
        assert ids.tolist() == [int(idx[r])]
    if V in E.V2_VOCABS:
        edges = {s * V // 16 for s in range(17)}
        assert set(idx.tolist()) == {e for e in edges if e < V} | {e - 1 for e in edges if e > 0}

    logits, top_p, ids, pn = E.nucleus_case(V)
    assert len(ids) == 8 and abs(float(pn.sum()) - 1) < 1e-12
    y = logits.double()[ids]
    assert (y[:-1] - y[1:]).min() >= 0.1  # >= 3 bins of 30/1024 apart
    rest = torch.ones(V, dtype=torch.bool)
    rest[ids] = False
    assert logits[rest].max() <= -0.25 * 8 + 1e-6
    assert set(logits[logits < -20].tolist()) <= {-25.0, -40.0, float("-inf")}
    # torch_ref draws inside the nucleus too
    g = torch.Generator().manual_seed(0)
    draws = torch_ref.top_p_sample(
        logits.repeat(64, 1), torch.ones(64), torch.full((64,), top_p), [g] * 64
    )
    assert set(draws.tolist()) <= set(ids.tolist())

    lg, temps, top_ps, allowed = E.mixed_rows(V)
    assert (temps > 0).tolist() == [False, True] * 16
    assert {len(a) for a in allowed[1::2]} == set(range(2, 13))
    assert top_ps.unique().numel() > 8
    ref = torch_ref.top_p_sample(lg, temps, top_ps, [g] * 32)
    for r in range(E.SAMPLER_ROWS):
        assert int(ref[r]) in allowed[r]

    one, where = E.single_entry_rows(V)
    assert torch.equal(torch_ref.top_p_sample(one, torch.zeros(32), torch.ones(32)), where)
    assert torch.equal(
        torch_ref.top_p_sample(one, torch.ones(32), torch.full((32,), 0.9), [g] * 32), where
    )
