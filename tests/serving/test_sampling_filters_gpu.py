"""top_k / min_p through the GPU engine: the chained decode loop and the
per-step sampler launch the same filtered kernels on the same statics, and a
filtered row leaves its unfiltered batch neighbours alone.

Only identical batch compositions are compared (a bf16 GEMM at M=2 reduces
differently than at M=1; see test_gpu_chain.py).
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.llm.types import SamplingParams
from dts_amd.serving import ServingEngine

PROMPT = [300 + (i * 37) % 900 for i in range(48)]
FILTERS = dict(top_k=8, min_p=0.05)


def _mk_engine(**env):
    old = {}
    for k, v in env.items():
        old[k] = os.environ.get(k)
        os.environ[k] = v
    try:
        return ServingEngine(
            model_name="llama-3-8b-2l",  # 2 layers, real D=128 kernels
            device="cuda:0",
            dtype=torch.bfloat16,
            kv_memory_bytes=1 << 30,
            weight_seed=7,
        )
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(env, param_list, max_tokens=32):
    eng = _mk_engine(**env)
    futs = [
        eng.submit_tokens(
            list(PROMPT), SamplingParams(max_tokens=max_tokens, temperature=0.8, **p)
        )
        for p in param_list
    ]
    eng.run_until_idle()
    return eng, [f.result(timeout=120).token_ids for f in futs]


def test_filtered_chain_matches_stepped():
    reqs = [dict(seed=31, **FILTERS), dict(seed=32, **FILTERS), dict(seed=33, top_k=2)]
    eng_off, ref = _run({"DTS_NO_CHAIN": "1", "DTS_SPEC_K": "0"}, reqs)
    assert eng_off.chain_steps == 0
    eng_on, out = _run({"DTS_SPEC_K": "0"}, reqs)
    assert eng_on.chain_steps > 0, "chain never engaged"
    assert out == ref
    assert all(len(t) == 32 for t in out)


def test_filtered_row_leaves_its_neighbour_alone():
    """Pair (unfiltered, filtered) against pair (unfiltered, unfiltered): the
    first request's stream is the same; its row runs through the filtered
    kernels as a disabled row in the first run."""
    env = {"DTS_SPEC_K": "0"}
    eng_a, a = _run(env, [dict(seed=41), dict(seed=42, **FILTERS)])
    eng_b, b = _run(env, [dict(seed=41), dict(seed=42)])
    assert eng_a.chain_steps > 0 and eng_b.chain_steps > 0
    assert len(a[0]) == len(a[1]) == len(b[1]) == 32  # both rows decode throughout
    assert a[0] == b[0]
    assert a[1] != b[1]  # and the filters did act on the second request
