"""ServingEngine(kv_cache_dtype="fp8") on the GPU at Llama-3-8B layer shapes
(two layers): pool dtype and size, generation through FP8 prefix pages,
determinism and graph capture."""

import random

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.llm.types import SamplingParams
from dts_amd.serving import ServingEngine
from dts_amd.serving.kv_cache import KVCachePool

KV_BYTES = 2 << 30


@pytest.fixture(scope="module")
def engine():
    eng = ServingEngine(
        model_name="llama-3-8b-2l",
        device="cuda:0",
        dtype=torch.bfloat16,
        kv_memory_bytes=KV_BYTES,
        weight_seed=0,
        kv_cache_dtype="fp8",
    )
    yield eng
    eng.stop()


def _gen(engine, prompt_ids, **kw):
    fut = engine.submit_tokens(list(prompt_ids), SamplingParams(**kw))
    engine.run_until_idle()
    return fut.result(timeout=120)


def test_pool_is_fp8_with_twice_the_blocks(engine):
    assert engine.cache_stats["kv_cache_dtype"] == "fp8"
    pool = engine.kv_pool
    assert pool.k.dtype == torch.float8_e4m3fn
    assert pool.v.dtype == torch.float8_e4m3fn
    spec = engine.spec
    bf16_blocks = KVCachePool.blocks_for_memory(
        KV_BYTES, spec.num_layers, spec.num_kv_heads, spec.head_dim, 16, dtype_bytes=2
    )
    assert pool.num_blocks == 2 * bf16_blocks
    assert pool.k.numel() + pool.v.numel() <= KV_BYTES


def test_generation_is_deterministic_and_captured(engine):
    """Runs 2 and 3 hit the prefix cache, so their prefill reads FP8 prefix
    pages; identical batch composition -> identical tokens."""
    prompt = [random.Random(5).randrange(300, 100000) for _ in range(64)]
    cold = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    assert cold.completion_tokens >= 1
    assert cold.finish_reason in ("stop", "length")
    hits0 = engine.cache_stats["cache_hit_tokens"]
    a = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    b = _gen(engine, prompt, max_tokens=8, temperature=0.0, seed=0)
    assert a.token_ids == b.token_ids
    assert engine.cache_stats["cache_hit_tokens"] > hits0
    assert engine.cache_stats["graph_steps"] > 0
    # every cache byte is a finite code (unwritten bytes are 0x00)
    for cache in (engine.kv_pool.k, engine.kv_pool.v):
        codes = cache.view(torch.uint8)
        assert not ((codes & 0x7F) == 0x7F).any()
        assert codes.any()


def _mini(spec_k):
    return ServingEngine(
        model_name="llama-mini-gpu",  # small vocab: greedy decode loops fast
        device="cuda:0",
        dtype=torch.bfloat16,
        kv_memory_bytes=1 << 28,
        weight_seed=7,
        kv_cache_dtype="fp8",
        spec_k=spec_k,
    )


MINI_PROMPT = [300 + (i * 37) % 900 for i in range(32)] * 2


def test_speculative_rows_on_fp8_pages(monkeypatch):
    """Speculative draft rows need no FP8-specific code; this pins that they
    run on an FP8 pool: drafts are accepted, steps shrink, and the stream is
    self-deterministic (the recipe of TestSpecOnGPU: chain off)."""
    monkeypatch.setenv("DTS_NO_CHAIN", "1")
    eng_off = _mini(0)
    try:
        ref = _gen(eng_off, MINI_PROMPT, max_tokens=256, temperature=0.0)
        steps_off = eng_off.steps
    finally:
        eng_off.stop()
    outs = []
    for _ in range(2):
        eng = _mini(4)
        try:
            res = _gen(eng, MINI_PROMPT, max_tokens=256, temperature=0.0)
            assert res.completion_tokens == ref.completion_tokens
            assert eng.spec_draft_tokens > 0 and eng.spec_accepted_tokens > 0
            assert eng.steps < steps_off
            assert eng.cache_stats["graph_steps"] > 0
            outs.append(res.token_ids)
        finally:
            eng.stop()
    assert outs[0] == outs[1]


def test_chained_decode_on_fp8_pages(monkeypatch):
    monkeypatch.delenv("DTS_NO_CHAIN", raising=False)
    outs = []
    for _ in range(2):
        eng = _mini(0)
        try:
            res = _gen(eng, MINI_PROMPT, max_tokens=64, temperature=0.7, seed=3)
            assert res.completion_tokens >= 1
            assert eng.cache_stats["chain_steps"] > 0
            outs.append(res.token_ids)
        finally:
            eng.stop()
    assert outs[0] == outs[1]
