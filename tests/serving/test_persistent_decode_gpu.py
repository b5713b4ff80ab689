"""Greedy decode of llama-3-8b-2l (the real K=4096 shapes: the small test
models have hidden sizes below 512 and never reach the skinny GEMM) with the
persistent skinny GEMM pinned off and pinned on, eager and through a
captured decode graph, at batch 1 and batch 8.

The persistent kernel is bit-identical to gemm_skinny_kernel by
construction, so the logits of every step are ``torch.equal`` between the
two pins, and a graph replay equals the eager forward under either pin.
Pinned on, every skinny GEMM whose K fits takes the new kernel (qkv, o,
gate_up with its SwiGLU epilogue at batch 8, lm_head at batch 8); down_proj
(K=14336) and the GEMV shapes of batch 1 keep theirs. So batch 8 is the leg
that covers the new kernel at the shapes the rule selects; at batch 1
gate_up and lm_head are GEMV calls under either pin and only qkv and o
change kernel. A graph keeps the kernels it was captured with, so each run
captures its own.
"""

import pytest
import torch

from dts_amd.serving.batch import ForwardBatch
from dts_amd.serving.graph_runner import DecodeGraphRunner
from dts_amd.serving.kv_cache import KVCachePool

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS = 16
PROMPT = 5
STEPS = 6
BLOCKS_PER_SEQ = 2  # PROMPT + STEPS positions fit in 32 slots
NUM_BLOCKS = 24
SCRATCH = 20


@pytest.fixture(scope="module")
def model():
    from dts_amd.models.config import get_model_spec
    from dts_amd.models.llama import LlamaModel

    m = LlamaModel(get_model_spec("llama-3-8b-2l"), dtype=torch.bfloat16, device=DEV)
    m.random_init(seed=3)
    yield m
    del m
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ext():
    from dts_amd.ops import _hip_ext_loader

    return _hip_ext_loader.load()


def _decode(model, ext, pin, batch, graph):
    """Logits [STEPS, batch, vocab] (fp32, CPU) of a greedy decode."""
    spec = model.spec
    g = torch.Generator().manual_seed(17 + batch)
    prompts = torch.randint(0, spec.vocab_size, (batch, PROMPT), generator=g).tolist()
    tables = [[1 + BLOCKS_PER_SEQ * i + j for j in range(BLOCKS_PER_SEQ)]
              for i in range(batch)]
    assert max(max(t) for t in tables) < SCRATCH
    pool = KVCachePool(spec.num_layers, spec.num_kv_heads, spec.head_dim,
                       NUM_BLOCKS, BS, dtype=torch.bfloat16, device=DEV)
    runner = DecodeGraphRunner(model, pool, DEV, SCRATCH,
                               max_blocks_per_seq=BLOCKS_PER_SEQ, max_bucket=16)
    previous = ext.skinny_persistent_pin(pin)
    try:
        out = []
        with torch.inference_mode():
            first = []
            for toks, table in zip(prompts, tables):
                b = ForwardBatch.single_prefill(toks, table, BS)
                first.append(model.forward(b.to(DEV), pool)[-1].float().cpu())
            tokens = [int(l.argmax()) for l in first]
            for k in range(STEPS):
                pos = PROMPT + k
                b = ForwardBatch(
                    token_ids=torch.tensor(tokens, dtype=torch.long),
                    positions=torch.full((batch,), pos, dtype=torch.long),
                    slot_mapping=torch.tensor(
                        [t[pos // BS] * BS + pos % BS for t in tables], dtype=torch.long
                    ),
                    num_decode_seqs=batch,
                    decode_block_tables=torch.tensor(tables, dtype=torch.int32),
                    decode_kv_lens=torch.full((batch,), pos + 1, dtype=torch.int32),
                    sample_indices=torch.arange(batch, dtype=torch.long),
                )
                if graph:
                    assert runner.can_run(b)
                    logits = runner.run(b)
                else:
                    logits = model.forward(b.to(DEV), pool)
                logits = logits.float().cpu().clone()
                assert logits.shape == (batch, spec.vocab_size)
                out.append(logits)
                tokens = logits.argmax(dim=-1).tolist()
            torch.cuda.synchronize()
        if graph:
            assert sorted(runner._graphs) == [batch]
    finally:
        ext.skinny_persistent_pin(previous)
    return torch.stack(out)


@pytest.mark.parametrize("batch", [1, 8])
def test_pinned_off_and_on_decode_the_same_logits(model, ext, batch):
    runs = {
        (pin, graph): _decode(model, ext, pin, batch, graph)
        for pin in (0, 1)
        for graph in (False, True)
    }
    base = runs[(0, False)]
    assert bool(torch.isfinite(base).all())
    # the decode moves: not one row of logits repeated
    assert not torch.equal(base[0], base[-1])
    for key, got in runs.items():
        for k in range(STEPS):
            assert torch.equal(got[k], base[k]), (key, k)


def test_pin_returns_the_previous_value_and_rejects_others(ext):
    start = ext.skinny_persistent_pin(1)
    try:
        assert ext.skinny_persistent_pin(0) == 1
        assert ext.skinny_persistent_pin(-1) == 0
        with pytest.raises(RuntimeError, match="pin must be"):
            ext.skinny_persistent_pin(2)
        assert ext.skinny_persistent_pin(-1) == -1
    finally:
        ext.skinny_persistent_pin(start)
