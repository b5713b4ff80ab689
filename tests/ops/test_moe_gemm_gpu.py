"""moe_grouped_gemm (tiled grouped MoE GEMM, 64 x 64 blocks, K-steps of 64).
Exact cases use ternary operands (tests/ops/_edge_inputs.py): every sum is an
integer exact in fp32 and bf16, so the comparison is on bit patterns."""

import functools

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
COUNTS = [0, 1, 63, 64, 65, 0, 131, 5]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _exact_case(rows_w, K):
    """x, w, counts, offsets, exact product (sentinel in the gap rows), gap"""
    g = gen(47 + rows_w * 101 + K)
    offsets, o = [], 0
    for e, c in enumerate(COUNTS):
        offsets.append(o)
        o += c
        if e == 3:  # three rows that no expert owns
            gap = list(range(o, o + 3))
            o += 3
    x, w = ternary((o, K), g), ternary((len(COUNTS), rows_w, K), g)
    want = torch.full((o, rows_w), SENTINEL, dtype=BF16)
    for e, (c, off) in enumerate(zip(COUNTS, offsets)):
        if c:
            want[off : off + c] = exact_product(x[off : off + c], w[e])
    return x.to(DEV), w.to(DEV), _i32(COUNTS), _i32(offsets), want.to(DEV), gap


@pytest.mark.parametrize("K", [512, 576])
@pytest.mark.parametrize("rows_w,swiglu", [(40, False), (144, False), (32, True), (96, True)])
def test_exact_with_unowned_rows(rows_w, swiglu, K):
    """SwiGLU (I = 16, 48): ext.silu_mul of the exact [P, 2I] product."""
    x, w, counts, offsets, want, gap = _exact_case(rows_w, K)
    if swiglu:
        exact, want = want, torch.empty(want.shape[0], rows_w // 2, dtype=BF16, device=DEV)
        ext.silu_mul(want, exact)
        want[gap] = SENTINEL
    out = torch.full_like(want, SENTINEL)
    ext.moe_grouped_gemm(out, x, w, counts, offsets, swiglu=swiglu)
    assert torch.equal(bits(out.cpu()), bits(want.cpu()))  # gap rows: sentinel


def test_result_does_not_depend_on_placement():
    """Five rows alone and as rows 60..64 of a 131-row segment elsewhere."""
    K, N, g = 512, 64, gen(53)
    w = torch.randn(2, N, K, generator=g).to(BF16).to(DEV)
    rows = torch.randn(5, K, generator=g).to(BF16).to(DEV)
    alone = torch.empty(5, N, dtype=BF16, device=DEV)
    ext.moe_grouped_gemm(alone, rows, w, _i32([0, 5]), _i32([0, 0]))
    x = torch.randn(3 + 131, K, generator=g).to(BF16).to(DEV)
    x[3 + 60 : 3 + 65] = rows
    out = torch.empty(3 + 131, N, dtype=BF16, device=DEV)
    ext.moe_grouped_gemm(out, x, w, _i32([3, 131]), _i32([0, 3]))
    assert torch.equal(bits(out[3 + 60 : 3 + 65].cpu()), bits(alone.cpu()))


def test_randn_against_fp64():
    """|got - ref| <= ulp_bf16(max(|got|, |ref|)) / 2 (the one final
    rounding) + 2 K 2^-24 (|x| @ |w|^T) (fp32 accumulation in any order,
    doubled for the MFMA's internal adds)."""
    K, N, counts, offsets, g = 1536, 48, [70, 0, 9], [0, 70, 70], gen(59)
    x = torch.randn(79, K, generator=g).to(BF16)
    w = torch.randn(3, N, K, generator=g).to(BF16)
    out = torch.empty(79, N, dtype=BF16, device=DEV)
    ext.moe_grouped_gemm(out, x.to(DEV), w.to(DEV), _i32(counts), _i32(offsets))
    for e, (c, o) in enumerate(zip(counts, offsets)):
        got, xe, we = out[o : o + c].cpu().double(), x[o : o + c].double(), w[e].double()
        ref = xe @ we.T
        bound = bf16_ulp(torch.maximum(got.abs(), ref.abs())) / 2
        bound = bound + 2 * K * 2.0**-24 * (xe.abs() @ we.abs().T)
        assert ((got - ref).abs() <= bound).all()


def _args(K=64, E=2, swiglu=False):
    z = functools.partial(torch.zeros, dtype=BF16, device=DEV)
    return dict(out=z(4, 16 if swiglu else 32) + SENTINEL, x=z(4, K), w=z(E, 32, K),
                counts=_i32([4] + [0] * (E - 1)), offsets=_i32([0] * E), swiglu=swiglu)


REJECTED = {
    "fp32_weight": lambda a: a.update(w=a["w"].float()),
    "weight_k": lambda a: a.update(w=a["w"][:, :, :32].contiguous()),
    "int64_counts": lambda a: a.update(counts=a["counts"].long()),
    "strided_x": lambda a: a.update(x=a["x"].repeat(1, 2)[:, :64]),
    "E65": lambda a: a.update(_args(E=65)),
    "K520": lambda a: a.update(_args(K=520)),
    "out_width_plain": lambda a: a.update(out=a["out"][:, :16].contiguous()),
    "out_width_swiglu": lambda a: a.update(_args(swiglu=True), out=a["out"]),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_rejected_before_launch(name):
    a = _args()
    ext.moe_grouped_gemm(**a)  # the unmodified arguments are accepted
    a["out"].fill_(SENTINEL)
    REJECTED[name](a)
    with pytest.raises(RuntimeError):
        ext.moe_grouped_gemm(**a)
    assert (a["out"] == SENTINEL).all()
