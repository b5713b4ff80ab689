"""moe_grouped_gemm(block=128), the 128-row LDS-shared grouped MoE GEMM: exact
on ternary operands (tests/ops/_edge_inputs.py), the 64-row kernel's bits."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader
from tests.ops._edge_inputs import (
    SENTINEL, bf16_ulp, bits, exact_product, gen, ternary,
)

ext = _hip_ext_loader.load()
DEV = "cuda:0"
BF16 = torch.bfloat16
# empty, one row, BM - 1, BM, BM + 1, three blocks with a ragged last one
# whose second wave-half is empty; rows 256..258 (after expert 3) are unowned
COUNTS = [0, 1, 127, 128, 129, 0, 259, 5]
OFFSETS = [0, 0, 1, 128, 259, 388, 388, 647]
P, GAP = 652, [256, 257, 258]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _run(x, w, swiglu, block, counts=COUNTS, offsets=OFFSETS):
    n = w.shape[1] // 2 if swiglu else w.shape[1]
    out = torch.full((x.shape[0], n), SENTINEL, dtype=BF16, device=DEV)
    ext.moe_grouped_gemm(out, x.to(DEV), w.to(DEV), _i32(counts), _i32(offsets),
                         swiglu=swiglu, block=block)
    return out


@pytest.mark.parametrize("K", [512, 576])
@pytest.mark.parametrize("rows_w,swiglu", [(40, False), (272, False), (32, True), (288, True)])
def test_exact_with_unowned_rows(rows_w, swiglu, K):
    """SwiGLU (I = 16, 144): ext.silu_mul of the exact [P, 2I] product."""
    g = gen(61 + rows_w * 101 + K)
    x, w = ternary((P, K), g), ternary((len(COUNTS), rows_w, K), g)
    want = torch.full((P, rows_w), SENTINEL, dtype=BF16)
    for e, (c, off) in enumerate(zip(COUNTS, OFFSETS)):
        if c:
            want[off : off + c] = exact_product(x[off : off + c], w[e])
    want = want.to(DEV)
    if swiglu:
        exact, want = want, torch.empty(P, rows_w // 2, dtype=BF16, device=DEV)
        ext.silu_mul(want, exact)
        want[GAP] = SENTINEL
    out = _run(x, w, swiglu, 128)
    assert torch.equal(bits(out.cpu()), bits(want.cpu()))  # gap rows: sentinel


@pytest.mark.parametrize("swiglu", [False, True])
def test_bits_of_the_64_row_kernel(swiglu):
    g = gen(67)
    x = torch.randn(P, 1536, generator=g).to(BF16)
    w = torch.randn(len(COUNTS), 288, 1536, generator=g).to(BF16)
    owned = [p for p in range(P) if p not in GAP]
    wide, narrow = (_run(x, w, swiglu, b).cpu()[owned] for b in (128, 64))
    assert torch.equal(bits(wide), bits(narrow))


def test_randn_against_fp64():
    """test_moe_gemm_gpu's bound: half a bf16 ulp (the final rounding) + 2 K
    2^-24 (|x| @ |w|^T) (fp32 sums in any order, doubled for the MFMA's adds)"""
    K, N, counts, offsets, g = 1536, 144, [130, 0, 9], [0, 130, 130], gen(71)
    x = torch.randn(139, K, generator=g).to(BF16)
    w = torch.randn(3, N, K, generator=g).to(BF16)
    out = _run(x, w, False, 128, counts, offsets)
    for e, (c, o) in enumerate(zip(counts, offsets)):
        got, xe, we = out[o : o + c].cpu().double(), x[o : o + c].double(), w[e].double()
        ref = xe @ we.T
        bound = bf16_ulp(torch.maximum(got.abs(), ref.abs())) / 2
        bound = bound + 2 * K * 2.0**-24 * (xe.abs() @ we.abs().T)
        assert ((got - ref).abs() <= bound).all()


def test_block_rejected_before_launch():
    x, w = torch.ones(4, 64, dtype=BF16), torch.ones(2, 32, 64, dtype=BF16)
    for block in (64, 128):
        assert (_run(x, w, False, block, [4, 0], [0, 0]) == 64).all()
    out = torch.full((4, 32), SENTINEL, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError):
        ext.moe_grouped_gemm(out, x.to(DEV), w.to(DEV), _i32([4, 0]), _i32([0, 0]), block=96)
    assert (out == SENTINEL).all()
