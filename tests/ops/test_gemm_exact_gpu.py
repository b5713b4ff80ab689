"""gemv_bf16, gemm_skinny_bf16 (+ fused SwiGLU) and moe_grouped_linear in exact
integer arithmetic.

x and w are dense draws from {-1, 0, 1}: every product and partial sum is an
integer below 2^24, exact in fp32 in any order, and |sum| <= 256 is exact in
bf16 (the builder asserts it). So the answer does not depend on how a kernel
splits K and the comparison is torch.equal: one skipped k-chunk, one row of
the wrong expert or one tile written twice changes integers. Inputs:
tests/ops/_edge_inputs.py, proven in test_edge_inputs_cpu.py.
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


def _strided_out(M, N):
    """[M, N] view of a sentinel-filled buffer with a larger row stride."""
    buf = torch.full((M, N + 3), E.SENTINEL, dtype=BF16, device=DEV)
    return buf, buf[:, 1 : 1 + N]


def _assert_exact(buf, out, want):
    got = out.cpu()
    wrong = (E.bits(got) != E.bits(want)).nonzero()
    assert torch.equal(E.bits(got), E.bits(want)), (
        f"{wrong.shape[0]} wrong, first {wrong[:6].tolist()}"
    )
    # nothing outside the view was written
    assert (buf[:, 0] == E.SENTINEL).all() and (buf[:, out.shape[1] + 1 :] == E.SENTINEL).all()


@pytest.mark.parametrize("K", [512, 1536])
@pytest.mark.parametrize("N", [1, 3, 5, 18, 4100])
@pytest.mark.parametrize("M", range(1, 9))
def test_gemv_exact(M, N, K):
    x, w, want = E.gemm_inputs(M, N, K)
    buf, out = _strided_out(M, N)
    ext.gemv_bf16(out, _dev_strided(x), w.to(DEV))
    _assert_exact(buf, out, want)


def _skinny_cases():
    for K in (512, 2048):
        for unroll in (4, 8) if K % 1024 == 0 else (4,):
            for tiles in (1, 2, 4):
                for N in (16, 100, 272):
                    for M in (1, 7, 9, 16):
                        yield M, N, K, tiles, unroll


@pytest.mark.parametrize("M,N,K,tiles,unroll", list(_skinny_cases()))
def test_skinny_exact(M, N, K, tiles, unroll):
    x, w, want = E.gemm_inputs(M, N, K)
    xs = _dev_strided(x)
    buf, out = _strided_out(M, N)
    ext.gemm_skinny_bf16(out, xs, w.to(DEV), tiles, unroll)
    _assert_exact(buf, out, want)


def _dev_strided(x):
    xs = E.strided_rows(x)
    dev = xs.to(DEV)
    if dev.is_contiguous():  # the copy packed the view: rebuild it
        big = torch.zeros(x.shape[0], x.shape[1] + 16, dtype=x.dtype, device=DEV)
        dev = big[:, 8 : 8 + x.shape[1]]
        dev.copy_(x)
    assert not dev.is_contiguous() or x.shape[0] == 1
    assert dev.data_ptr() % 16 == 0 and dev.stride(0) * 2 % 16 == 0
    return dev


@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("inter", [16, 48, 144])
@pytest.mark.parametrize("M", [1, 7, 9, 16])
def test_skinny_swiglu_is_silu_mul_of_the_exact_gemm(M, inter, K):
    x, w, want = E.gemm_inputs(M, 2 * inter, K)
    act = torch.empty(M, inter, dtype=BF16, device=DEV)
    ext.silu_mul(act, want.to(DEV))
    # silu_mul itself against fp64 on these integers; at K = 2048 some gates
    # are <= -89, where the fp32 formula gives a signed zero (see
    # _edge_inputs.silu_expectation)
    ref, finite, nan, inf, zero, zero_bits = E.silu_expectation(want)
    assert not nan.any() and not inf.any()
    assert E.ulp_err(act.cpu()[finite], ref[finite]) <= 1.0
    assert torch.equal(E.bits(act.cpu())[zero], zero_bits[zero])
    out = torch.full((M, inter), E.SENTINEL, dtype=BF16, device=DEV)
    ext.gemm_skinny_swiglu_bf16(out, _dev_strided(x), w.to(DEV))
    assert torch.equal(E.bits(out.cpu()), E.bits(act.cpu()))


def test_moe_grouped_exact_with_unowned_rows():
    """Segments of 0, 1, 15, 16, 17 and 33 rows (one, two and three 16-row
    passes, ragged and not), N = 40 (a ragged third n-tile) and a 3-row gap
    that no expert owns: owned rows are exact, gap rows keep the sentinel."""
    x, w, counts, offsets, want, gap = E.moe_inputs()
    out = torch.full(tuple(want.shape), E.SENTINEL, dtype=BF16, device=DEV)
    ext.moe_grouped_linear(
        out, x.to(DEV), w.to(DEV), counts.to(DEV), offsets.to(DEV)
    )
    got = out.cpu()
    assert (got[gap] == E.SENTINEL).all()
    assert torch.equal(E.bits(got), E.bits(want))
