"""ServingEngine(kv_cache_dtype="fp8") on the tiny models (CPU, fp32
weights, FP8 e4m3 paged KV cache through the torch references)."""

import pytest
import torch

from dts_amd.llm.types import SamplingParams
from dts_amd.serving import ServingEngine
from dts_amd.serving.kv_cache import KVCachePool

PROMPT = [3, 17, 29, 41, 5, 6, 7, 8, 90, 11, 12, 13]


def _engine(model_name="llama-tiny", **kw):
    kw.setdefault("num_blocks", 256)
    kw.setdefault("weight_seed", 1)
    kw.setdefault("block_size", 4)
    return ServingEngine(
        model_name=model_name,
        device="cpu",
        dtype=torch.float32,
        max_batch_tokens=256,
        **kw,
    )


def _greedy(engine, max_tokens=8):
    fut = engine.submit_tokens(
        list(PROMPT), SamplingParams(max_tokens=max_tokens, seed=0, temperature=0.0)
    )
    engine.run_until_idle()
    return fut.result(timeout=5).token_ids


def _finite(pool):
    for cache in (pool.k, pool.v):
        assert cache.dtype == torch.float8_e4m3fn
        assert not ((cache.view(torch.uint8) & 0x7F) == 0x7F).any()


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("DTS_KV_CACHE_DTYPE", raising=False)
    monkeypatch.delenv("DTS_WEIGHT_QUANT", raising=False)


def test_generates_and_is_deterministic():
    runs = []
    for _ in range(2):
        eng = _engine(kv_cache_dtype="fp8")
        try:
            assert eng.cache_stats["kv_cache_dtype"] == "fp8"
            toks = _greedy(eng)
            assert len(toks) >= 1
            _finite(eng.kv_pool)
            # something was written
            assert eng.kv_pool.k.view(torch.uint8).any()
            runs.append(toks)
        finally:
            eng.stop()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("value", [None, "auto"])
def test_default_and_auto_keep_model_dtype(value):
    eng = _engine(kv_cache_dtype=value)
    try:
        assert eng.cache_stats["kv_cache_dtype"] is None
        assert eng.kv_pool.k.dtype == torch.float32
    finally:
        eng.stop()


def test_env_var_selects_fp8(monkeypatch):
    monkeypatch.setenv("DTS_KV_CACHE_DTYPE", "fp8")
    eng = _engine()
    try:
        assert eng.cache_stats["kv_cache_dtype"] == "fp8"
        assert eng.kv_pool.k.dtype == torch.float8_e4m3fn
    finally:
        eng.stop()


def test_keyword_wins_over_env(monkeypatch):
    monkeypatch.setenv("DTS_KV_CACHE_DTYPE", "fp8")
    eng = _engine(kv_cache_dtype="auto")
    try:
        assert eng.cache_stats["kv_cache_dtype"] is None
        assert eng.kv_pool.k.dtype == torch.float32
    finally:
        eng.stop()
    monkeypatch.setenv("DTS_KV_CACHE_DTYPE", "int3")
    eng = _engine(kv_cache_dtype="fp8")
    try:
        assert eng.cache_stats["kv_cache_dtype"] == "fp8"
    finally:
        eng.stop()


def test_bad_value_raises(monkeypatch):
    with pytest.raises(ValueError):
        _engine(kv_cache_dtype="int3")
    monkeypatch.setenv("DTS_KV_CACHE_DTYPE", "int3")
    with pytest.raises(ValueError):
        _engine()


def test_pool_has_dtype_bytes_times_the_blocks():
    budget = 1 << 20
    base = _engine(num_blocks=None, kv_memory_bytes=budget)
    fp8 = _engine(num_blocks=None, kv_memory_bytes=budget, kv_cache_dtype="fp8")
    try:
        dtype_bytes = base.kv_pool.k.element_size()
        assert dtype_bytes == 4
        assert abs(fp8.kv_pool.num_blocks - dtype_bytes * base.kv_pool.num_blocks) <= 1
        spec = fp8.spec
        assert fp8.kv_pool.num_blocks == KVCachePool.blocks_for_memory(
            budget, spec.num_layers, spec.num_kv_heads, spec.head_dim, 4, dtype_bytes=1
        )
        assert 2 * fp8.kv_pool.k.numel() * fp8.kv_pool.k.element_size() <= budget
    finally:
        base.stop()
        fp8.stop()


@pytest.mark.parametrize("model_name", ["gpt2-tiny", "mixtral-tiny"])
def test_other_architectures_run(model_name):
    eng = _engine(model_name, kv_cache_dtype="fp8")
    try:
        assert len(_greedy(eng, max_tokens=4)) >= 1
        _finite(eng.kv_pool)
    finally:
        eng.stop()


def test_combines_with_fp8_weights():
    eng = _engine(kv_cache_dtype="fp8", weight_quant="fp8")
    try:
        assert eng.cache_stats["kv_cache_dtype"] == "fp8"
        assert eng.cache_stats["weight_quant"] == "fp8"
        assert len(_greedy(eng)) >= 1
        _finite(eng.kv_pool)
    finally:
        eng.stop()


def test_speculative_rows_are_output_invisible():
    """Draft rows go through the prefill-attention path over FP8 pages; the
    stream must equal the spec-off stream, as with the fp32 cache."""
    # repetitive prompt; this tiny random model then loops, so drafts fire
    prompt = [310, 311, 312, 310, 311, 312, 310, 311]
    outs = {}
    for spec_k in (0, 4):
        eng = _engine(
            kv_cache_dtype="fp8", spec_k=spec_k, weight_seed=11,
            num_blocks=512, block_size=8,
        )
        try:
            fut = eng.submit_tokens(
                list(prompt), SamplingParams(max_tokens=48, temperature=0.0)
            )
            eng.run_until_idle()
            outs[spec_k] = fut.result(timeout=60).token_ids
            if spec_k:
                assert eng.spec_draft_tokens > 0
                assert eng.spec_accepted_tokens > 0
        finally:
            eng.stop()
    assert outs[0] == outs[4]
