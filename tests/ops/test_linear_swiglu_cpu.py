"""ops.linear_swiglu off the GPU: it must BE silu_mul(linear_bf16(...)),
and routing LlamaMLP through it must not change a llama-tiny forward."""

import pytest
import torch

from dts_amd import ops
from dts_amd.llm.types import SamplingParams
from dts_amd.models.llama import LlamaMLP
from dts_amd.serving import ServingEngine


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,K,I", [(1, 512, 16), (6, 512, 48), (20, 64, 24), (3, 96, 7)])
def test_linear_swiglu_equals_two_op_path(dtype, M, K, I):
    torch.manual_seed(0)
    x = torch.randn(M, K).to(dtype)
    w = (torch.randn(2 * I, K) / K**0.5).to(dtype)
    w[:I] *= 8.0  # gate pre-activations well into both tails of the sigmoid
    got = ops.linear_swiglu(x, w)
    ref = ops.silu_mul(ops.linear_bf16(x, w))
    assert got.shape == (M, I)
    assert torch.equal(got, ref)


def _old_mlp_forward(self, x):
    # LlamaMLP.forward as it was before linear_swiglu existed
    return self.down_proj(ops.silu_mul(self.gate_up_proj(x)))


def _make_engine():
    return ServingEngine(
        model_name="llama-tiny",
        device="cpu",
        dtype=torch.float32,
        num_blocks=256,
        block_size=4,
        max_batch_tokens=256,
        weight_seed=1,
    )


def test_llama_tiny_forward_unchanged(monkeypatch):
    eng = _make_engine()
    try:
        mlps = [m for m in eng.model.modules() if isinstance(m, LlamaMLP)]
        assert mlps, "llama-tiny has no LlamaMLP layers"
        torch.manual_seed(3)
        x = torch.randn(5, mlps[0].gate_up_proj.weight.shape[1])
        for mlp in mlps:
            assert torch.equal(mlp(x), _old_mlp_forward(mlp, x))

        def gen():
            fut = eng.submit_tokens(
                list(range(3, 24)),
                SamplingParams(max_tokens=12, seed=7, temperature=0.7),
            )
            eng.run_until_idle()
            return fut.result(timeout=30).token_ids

        new = gen()
        monkeypatch.setattr(LlamaMLP, "forward", _old_mlp_forward)
        old = gen()
        assert new == old and len(new) >= 1
    finally:
        eng.stop()
