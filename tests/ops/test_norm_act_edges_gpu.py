"""rmsnorm, fused_add_rmsnorm, layernorm and silu_mul against fp64 at the
shapes where the kernels branch: more rows than the 2048-workgroup grid
(each workgroup loops `row += gridDim.x` up to three times), a ragged second
column pass (H = 256*8 + 8), H = 8 (most threads idle), a silu_mul sweep that
runs twice with a ragged tail, and every bf16 gate pattern.

Measure: |got - ref64| <= ulp(ref64), ulp(r) = 2^(floor(log2|r|) - 7) -- one
fp32 evaluation (relative error << 2^-9) and one round-to-nearest-even.
Inputs and references: tests/ops/_edge_inputs.py, proven on torch_ref in
test_edge_inputs_cpu.py.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader
from tests.ops import _edge_inputs as E

ext = _hip_ext_loader.load()
DEV = "cuda:0"
BF16 = torch.bfloat16


def _rmsnorm(x, w):
    out = torch.empty_like(x, device=DEV)
    ext.rmsnorm(out, x.to(DEV), w.to(DEV), E.EPS)
    return out.cpu()


def _fused(x, r, w):
    xd, rd = x.to(DEV), r.to(DEV)
    ext.fused_add_rmsnorm(xd, rd, w.to(DEV), E.EPS)
    return xd.cpu(), rd.cpu()


def _layernorm(x, w, b):
    out = torch.empty_like(x, device=DEV)
    ext.layernorm(out, x.to(DEV), w.to(DEV), b.to(DEV), E.EPS)
    return out.cpu()


def _silu_mul(gu):
    out = torch.empty(gu.shape[0], gu.shape[1] // 2, dtype=BF16, device=DEV)
    ext.silu_mul(out, gu.to(DEV))
    return out.cpu()


def _assert_ulp(name, got, ref, bound=1.0):
    assert torch.isfinite(got.float()).all()
    err = E.ulp_err(got, ref)
    print(f"{name}: max error {err:.5f} ulp")
    assert err <= bound


@pytest.mark.parametrize("T,H", E.NORM_SHAPES)
def test_rmsnorm_one_ulp(T, H):
    x, _, w = E.norm_inputs(T, H)
    _assert_ulp(f"rmsnorm ({T}, {H})", _rmsnorm(x, w), E.rmsnorm64(x, w))


@pytest.mark.parametrize("T,H", E.NORM_SHAPES)
def test_fused_add_rmsnorm_one_ulp_and_exact_residual(T, H):
    x, r, w = E.norm_inputs(T, H)
    y, new_r = _fused(x, r, w)
    want_r = E.add_residual(x, r)
    assert torch.equal(E.bits(new_r), E.bits(want_r))
    _assert_ulp(f"fused_add_rmsnorm ({T}, {H})", y, E.rmsnorm64(want_r, w))


@pytest.mark.parametrize("T,H", E.NORM_SHAPES)
def test_layernorm_one_ulp(T, H):
    x, w, b = E.layernorm_inputs(T, H)
    _assert_ulp(f"layernorm ({T}, {H})", _layernorm(x, w, b), E.layernorm64(x, w, b))


def test_layernorm_row_mean_100():
    """Row mean 100, std 1: x^2 is 10^4 times the variance. The reference is
    the two-pass form."""
    T, H = E.LN_OFFSET_SHAPE
    x, w, b = E.layernorm_inputs(T, H, E.LN_OFFSET_MEAN)
    _assert_ulp("layernorm mean 100", _layernorm(x, w, b), E.layernorm64(x, w, b))


@pytest.mark.parametrize("T,H", [(4100, 2056), (5, 768)])
def test_norm_rows_are_independent(T, H):
    """A NaN row between finite rows leaves every other row bit-equal to the
    run without it. At T = 4100 the NaN row's workgroup goes on to row
    1001 + 2048 with the same LDS reduction buffer."""
    x, r, w = E.norm_inputs(T, H)
    lx, lw, lb = E.layernorm_inputs(T, H)
    bad = 1001 if T > 1001 else T // 2
    keep = torch.ones(T, dtype=torch.bool)
    keep[bad] = False

    def poisoned(t):
        t = t.clone()
        t[bad] = float("nan")
        return t

    for name, clean, dirty in (
        ("rmsnorm", _rmsnorm(x, w), _rmsnorm(poisoned(x), w)),
        ("fused", _fused(x, r, w)[0], _fused(poisoned(x), r, w)[0]),
        ("fused residual", _fused(x, r, w)[1], _fused(poisoned(x), r, w)[1]),
        ("layernorm", _layernorm(lx, lw, lb), _layernorm(poisoned(lx), lw, lb)),
    ):
        assert torch.isnan(dirty[bad].float()).all(), name
        assert torch.isfinite(clean.float()).all(), name
        assert torch.equal(E.bits(dirty[keep]), E.bits(clean[keep])), name


def test_silu_mul_second_sweep_and_ragged_tail():
    gu = E.silu_sweep_inputs()
    _assert_ulp(f"silu_mul {E.SILU_SWEEP}", _silu_mul(gu), E.silu_mul64(gu))


def test_silu_mul_every_gate_pattern():
    """All 65536 bf16 gates x up in {1, -3, 2^-20, 240}: one ulp where the
    result is finite, NaN and +-inf exactly where fp64 (rounded to bf16's
    range) gives them, and for finite gates <= -89 -- fp32 exp(-g) is +inf,
    so g / (1 + inf) is exactly -0 -- the signed zero -0 * up. fp64 gives
    about -g * e^g there (2e-37 at g = -89); no fp32 evaluation of this
    formula, torch's included, returns that."""
    gu = E.silu_exhaustive_inputs()
    ref, finite, nan, inf, zero, zero_bits = E.silu_expectation(gu)
    got = _silu_mul(gu)
    _assert_ulp(
        f"silu_mul exhaustive ({int(finite.sum())} finite)", got[finite], ref[finite]
    )
    assert torch.isnan(got[nan].float()).all()
    assert torch.equal(got[inf].float(), ref[inf].float().to(BF16).float())
    assert torch.equal(E.bits(got)[zero], zero_bits[zero])
