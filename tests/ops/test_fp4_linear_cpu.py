"""MXFP4 quantiser, dequantiser and the CPU side of ops.linear_w4a16."""

import pytest
import torch

from dts_amd import ops
from dts_amd.models.quant import dequantize_mxfp4, quantize_mxfp4_rowwise
from dts_amd.ops.torch_ref import E2M1_GRID

GRID = torch.tensor(E2M1_GRID)


@pytest.fixture(scope="module", params=[1.0 / 64, 1.0])
def case(request):
    w = torch.randn(64, 1024, generator=torch.Generator().manual_seed(7)) * request.param
    w[3, 32:64] = 0.0  # an all-zero block
    w_q, scale = quantize_mxfp4_rowwise(w)
    block_scale = torch.ldexp(torch.ones(()), scale.int() - 127).repeat_interleave(32, dim=1)
    return w, w_q, scale, block_scale, dequantize_mxfp4(w_q, scale, torch.float32)


def test_quantiser_properties(case):
    w, w_q, scale, block_scale, deq = case
    assert w_q.dtype == scale.dtype == torch.uint8
    assert w_q.shape == (64, 512) and scale.shape == (64, 32)
    # a byte IS a power of two; inside the clamp, never the NaN byte
    assert scale.min() >= 2 and scale.max() <= 252 and scale[3, 1] == 127
    assert torch.all(w.abs() / block_scale <= 6.0)  # no element clamps
    assert torch.all((deq - w).abs() <= block_scale)
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)  # exact in bf16
    assert torch.equal(deq[3, 32:64], torch.zeros(32))
    # a fixed point of quantise -> dequantise, on values
    assert torch.equal(dequantize_mxfp4(*quantize_mxfp4_rowwise(deq), torch.float32), deq)


@pytest.mark.parametrize("e", [-125, -3, 0, 10, 125])
def test_every_representable_value_round_trips(e):
    vals = torch.ldexp(torch.cat([GRID, -GRID]), torch.tensor(e))
    w = torch.cat([vals, vals]).view(1, 32)  # 6 * 2^e present: the scale is 2^e
    w_q, scale = quantize_mxfp4_rowwise(w)
    assert scale.item() == e + 127
    assert torch.equal(dequantize_mxfp4(w_q, scale, torch.float32), w)


@pytest.mark.parametrize(
    "v,want",
    [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0),
     (5.0, 4.0), (-2.5, -2.0), (-5.0, -4.0), (2.6, 3.0), (4.9, 4.0), (5.1, 6.0)],
)
def test_ties_go_to_even(v, want):
    s = 0.25
    w = torch.zeros(1, 32)
    w[0, 0], w[0, 1] = 6.0 * s, v * s  # the 6 pins the block scale to s
    deq = dequantize_mxfp4(*quantize_mxfp4_rowwise(w), torch.float32)
    assert deq[0, 1].item() == want * s


def test_nibble_order_by_hand():
    """Element 2i in the low nibble of byte i: 0x72 is (1.0, 6.0), 0xC1 is
    (0.5, -2.0); scale byte 128 doubles them."""
    w_q = torch.zeros(1, 16, dtype=torch.uint8)
    w_q[0, 0], w_q[0, 1] = 0x72, 0xC1
    deq = dequantize_mxfp4(w_q, torch.tensor([[128]], dtype=torch.uint8), torch.float32)
    assert deq[0, :4].tolist() == [2.0, 12.0, 1.0, -4.0]
    assert torch.equal(quantize_mxfp4_rowwise(deq)[0], w_q)


def test_ops_on_cpu_are_the_dequantised_path(case):
    _, w_q, scale, _, deq = case
    x = torch.randn(5, 1024, generator=torch.Generator().manual_seed(8))
    assert torch.equal(ops.linear_w4a16(x, w_q, scale, deq), ops.linear_bf16(x, deq))
    assert torch.equal(ops.linear_swiglu_w4a16(x, w_q, scale, deq), ops.linear_swiglu(x, deq))
