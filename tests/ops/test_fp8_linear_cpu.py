"""FP8 (e4m3fn) weight-only linear: quantiser properties and the CPU
fallbacks of the W8A16 ops (the GPU kernel is in test_fp8_gemm_gpu.py)."""

import pytest
import torch
import torch.nn.functional as F

from dts_amd import ops
from dts_amd.models.quant import (
    dequantize_fp8_rowwise,
    quantize_fp8_rowwise,
)
from dts_amd.ops import torch_ref


@pytest.fixture(scope="module")
def quantised():
    g = torch.Generator().manual_seed(7)
    w = torch.randn(64, 512, generator=g)
    w[5] *= 37.0  # rows of very different magnitude
    w[6] *= 1e-3
    w[9] = 0.0  # an all-zero row
    w[11, 3] = 448.0 * 4  # amax/448 exactly a power of two
    w_q, scale = quantize_fp8_rowwise(w)
    return w, w_q, scale


class TestQuantiser:
    def test_types_and_shapes(self, quantised):
        w, w_q, scale = quantised
        assert w_q.dtype == torch.float8_e4m3fn and w_q.shape == w.shape
        assert w_q.is_contiguous()
        assert scale.dtype == torch.float32 and scale.shape == (w.shape[0],)

    def test_scale_is_power_of_two(self, quantised):
        _, _, scale = quantised
        mant, _ = torch.frexp(scale)
        assert torch.all(scale > 0)
        assert torch.all(mant == 0.5)

    def test_scale_is_the_smallest_that_fits(self, quantised):
        w, _, scale = quantised
        amax = w.abs().amax(dim=1)
        live = amax > 0
        assert torch.all(amax[live] / scale[live] <= 448.0)
        # half the scale would overflow e4m3: scale = 2^ceil(log2(amax/448))
        assert torch.all(amax[live] / (scale[live] / 2) > 448.0)
        assert scale[11] == 4.0

    def test_values_within_range(self, quantised):
        w, _, scale = quantised
        assert torch.all((w / scale[:, None]).abs() <= 448.0)

    def test_no_nan_code(self, quantised):
        _, w_q, _ = quantised
        codes = w_q.view(torch.uint8)
        assert not torch.any((codes & 0x7F) == 0x7F)
        assert not torch.any(torch.isnan(w_q.float()))

    def test_dequantised_survives_bf16_round_trip(self, quantised):
        _, w_q, scale = quantised
        deq = w_q.float() * scale[:, None]
        assert torch.equal(deq.to(torch.bfloat16).float(), deq)
        assert torch.equal(
            dequantize_fp8_rowwise(w_q, scale, torch.bfloat16).float(), deq
        )

    def test_all_zero_row(self, quantised):
        _, w_q, scale = quantised
        assert scale[9] == 1.0
        assert torch.all(w_q[9].float() == 0)

    def test_quantisation_error(self, quantised):
        """Relative Frobenius error below 2^-4, the e4m3 half-ulp bound for
        normal values (3 mantissa bits); randn measures about 0.027."""
        w, w_q, scale = quantised
        deq = w_q.float() * scale[:, None]
        rel = (deq - w).norm() / w.norm()
        print(f"relative quantisation error {rel:.4f}")
        assert rel < 2.0**-4


class TestCPUFallback:
    @pytest.mark.parametrize("M", [1, 4, 33])
    def test_linear_w8a16_is_linear_on_dequantised(self, quantised, M):
        _, w_q, scale = quantised
        w_deq = dequantize_fp8_rowwise(w_q, scale, torch.float32)
        x = torch.randn(M, 512, generator=torch.Generator().manual_seed(M))
        out = ops.linear_w8a16(x, w_q, scale, w_deq)
        assert torch.equal(out, F.linear(x, w_deq))

    def test_oracle_matches_dequantised(self, quantised):
        """torch_ref.linear_w8a16 (scale applied to the sum) against the
        fp64 product with the dequantised matrix."""
        _, w_q, scale = quantised
        w_deq = dequantize_fp8_rowwise(w_q, scale, torch.float64)
        x = torch.randn(4, 512, generator=torch.Generator().manual_seed(3))
        ref = torch_ref.linear_w8a16(x, w_q, scale)
        assert ref.dtype == x.dtype
        # fp32 summation bound per output row: K * eps * max|x| * max|w_row|
        bound = 512 * 2.0**-24 * x.abs().max().double() * w_deq.abs().amax(dim=1)
        err = (ref.double() - x.double() @ w_deq.T).abs()
        assert torch.all(err <= bound + 1e-30)

    @pytest.mark.parametrize("M", [2, 9])
    def test_linear_swiglu_w8a16(self, quantised, M):
        _, w_q, scale = quantised
        w_deq = dequantize_fp8_rowwise(w_q, scale, torch.float32)
        x = torch.randn(M, 512, generator=torch.Generator().manual_seed(M))
        out = ops.linear_swiglu_w8a16(x, w_q, scale, w_deq)
        assert out.shape == (M, 32)
        ref = torch_ref.silu_mul(ops.linear_w8a16(x, w_q, scale, w_deq))
        assert torch.equal(out, ref)
