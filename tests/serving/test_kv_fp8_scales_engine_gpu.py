"""ServingEngine(kv_cache_dtype="fp8", kv_scales="calibrate") on the GPU at
Llama-3-8B layer shapes (two layers, random weights): calibration through the
HIP kernels, generation through scaled FP8 prefix pages under graph capture,
and what the scales buy once a projection is rescaled."""

import random

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.llm.types import SamplingParams
from dts_amd.serving import ServingEngine
from dts_amd.serving.batch import ForwardBatch

DEV = "cuda:0"


def _engine(**kw):
    kw.setdefault("kv_memory_bytes", 1 << 28)
    return ServingEngine(
        model_name="llama-3-8b-2l", device=DEV, dtype=torch.bfloat16,
        weight_seed=0, **kw,
    )


def _gen(engine, prompt_ids, **kw):
    fut = engine.submit_tokens(list(prompt_ids), SamplingParams(**kw))
    engine.run_until_idle()
    return fut.result(timeout=120)


@pytest.fixture(scope="module")
def engine():
    eng = _engine(kv_cache_dtype="fp8", kv_scales="calibrate")
    yield eng
    eng.stop()


def test_calibrate_gives_non_unit_powers_of_two(engine):
    s = engine.kv_scales
    assert engine.cache_stats["kv_scales"] == "calibrated"
    assert s.shape == (2, 2, 8) and s.dtype == torch.float32 and s.is_cuda
    assert ((torch.log2(s) % 1) == 0).all()
    assert not (s == 1).all()
    # nothing ran through the engine's own pool or scheduler
    assert engine.steps == 0 and engine.cache_stats["tokens_prefilled"] == 0
    assert not engine.kv_pool.k.view(torch.uint8).any()


def test_generation_is_deterministic_and_captured(engine):
    prompt = [random.Random(5).randrange(300, 100000) for _ in range(64)]
    cold = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    assert cold.completion_tokens >= 1
    hits0 = engine.cache_stats["cache_hit_tokens"]
    a = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    b = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    assert a.token_ids == b.token_ids
    assert engine.cache_stats["cache_hit_tokens"] > hits0
    assert engine.cache_stats["graph_steps"] > 0
    for cache in (engine.kv_pool.k, engine.kv_pool.v):
        codes = cache.view(torch.uint8)
        assert not ((codes & 0x7F) == 0x7F).any()
        assert codes.any()
    with pytest.raises(RuntimeError):
        engine.calibrate_kv_scales([prompt])


@torch.inference_mode()
def _last_logits(eng, tokens):
    table = list(range((len(tokens) + 15) // 16))
    batch = ForwardBatch.single_prefill(tokens, table, 16).to(DEV)
    return eng.model.forward(batch, eng.kv_pool)[0].float().cpu()


def test_calibrated_scales_at_least_halve_the_logits_error_on_v_rescaled_model():
    """v rows x 2^-8, o_proj x 2^8 (exact in bf16, function-preserving):
    V falls into e4m3's subnormals at unit scale."""
    ref = _engine()
    spec = ref.spec
    off = (spec.num_heads + spec.num_kv_heads) * spec.head_dim
    with torch.no_grad():
        for layer in ref.model.layers:
            layer.attn.qkv_proj.weight[off:] *= 2.0**-8
            layer.attn.o_proj.weight *= 2.0**8
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, spec.vocab_size, (256,), generator=g).tolist()
    unit = _engine(model=ref.model, kv_cache_dtype="fp8")
    cal = _engine(model=ref.model, kv_cache_dtype="fp8", kv_scales="calibrate")
    try:
        assert (cal.kv_scales[:, 1] < 2.0**-6).all()
        want = _last_logits(ref, tokens)
        e_unit = ((_last_logits(unit, tokens) - want).norm() / want.norm()).item()
        e_cal = ((_last_logits(cal, tokens) - want).norm() / want.norm()).item()
        print(f"logits error vs bf16 cache: unit {e_unit:.4f} calibrated {e_cal:.4f}")
        assert e_cal <= 0.5 * e_unit
    finally:
        for e in (ref, unit, cal):
            e.stop()
