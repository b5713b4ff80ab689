"""ServingEngine(weight_quant="fp8") on the GPU at Llama-3-8B layer shapes
(two layers): the decode kernel against the dequantised copy, generation,
determinism and graph capture."""

import random

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.llm.types import SamplingParams
from dts_amd.models.quant import quantized_linears
from dts_amd.serving import ServingEngine


@pytest.fixture(scope="module")
def engine():
    eng = ServingEngine(
        model_name="llama-3-8b-2l",
        device="cuda:0",
        dtype=torch.bfloat16,
        kv_memory_bytes=2 << 30,
        weight_seed=0,
        weight_quant="fp8",
    )
    yield eng
    eng.stop()


def _gen(engine, prompt_ids, **kw):
    fut = engine.submit_tokens(list(prompt_ids), SamplingParams(**kw))
    engine.run_until_idle()
    return fut.result(timeout=120)


def test_kernel_matches_dequantised_copy(engine):
    """Each of the eight quantised linears at M = 4 (FP8 skinny kernel)
    against the plain GEMM on the dequantised copy it also holds."""
    lins = list(quantized_linears(engine.model))
    assert len(lins) == 8
    g = torch.Generator(device="cuda:0").manual_seed(3)
    for lin in lins:
        assert lin.weight_q.dtype == torch.float8_e4m3fn
        assert lin.weight_q.is_cuda and lin.weight_q.is_contiguous()
        # both copies hold the same matrix
        assert torch.equal(
            lin.weight.float(), lin.weight_q.float() * lin.weight_scale[:, None]
        )
        x = torch.randn(
            4, lin.weight.shape[1], generator=g, device="cuda:0"
        ).to(torch.bfloat16)
        with torch.inference_mode():
            got = lin(x)
            ref = F.linear(x, lin.weight)
        torch.testing.assert_close(got.float(), ref.float(), atol=3e-2, rtol=3e-2)


def test_generation_is_deterministic_and_captured(engine):
    """Identical batch composition -> identical tokens: run 2 and 3 are
    both fully cache-hit, so they must match exactly."""
    assert engine.cache_stats["weight_quant"] == "fp8"
    prompt = [random.Random(5).randrange(300, 100000) for _ in range(64)]
    cold = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    assert cold.completion_tokens >= 1
    assert cold.finish_reason in ("stop", "length")
    a = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    b = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    assert a.token_ids == b.token_ids
    assert engine.cache_stats["graph_steps"] > 0
