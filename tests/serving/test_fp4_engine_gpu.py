"""ServingEngine(weight_quant="mxfp4") on the GPU at Llama-3-8B layer shapes
(two layers): a decode step through the W4A16 kernels against the bf16
kernels on the same dequantised matrices, and graph replay against eager."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.models.quant import dequantize_mxfp4, quantized_linears
from dts_amd.serving import ServingEngine
from dts_amd.serving.batch import ForwardBatch
from dts_amd.serving.graph_runner import DecodeGraphRunner
from tests.serving import _graph_inputs as G

DEV = "cuda:0"


@pytest.fixture(scope="module")
def engine():
    eng = ServingEngine(model_name="llama-3-8b-2l", device=DEV, dtype=torch.bfloat16,
                        kv_memory_bytes=2 << 30, weight_seed=0, weight_quant="mxfp4")
    yield eng
    eng.stop()


def _decode_batch(engine, M):
    """M rows that each decode their first token: position 0 of block i, so
    the step reads no cache contents but its own."""
    bs = engine.kv_pool.block_size
    rows = torch.arange(M)
    return ForwardBatch(
        token_ids=(rows * 7919 + 300) % 100000,
        positions=torch.zeros(M, dtype=torch.long),
        slot_mapping=rows * bs,
        num_decode_seqs=M,
        decode_block_tables=rows.to(torch.int32).view(M, 1),
        decode_kv_lens=torch.ones(M, dtype=torch.int32),
        sample_indices=rows.clone(),
    )


@pytest.mark.parametrize("M", [1, 6, 16])
def test_decode_step_matches_bf16_kernels_on_the_same_matrix(engine, M):
    assert engine.cache_stats["weight_quant"] == "mxfp4"
    lins = list(quantized_linears(engine.model))
    assert len(lins) == 8
    for lin in lins:
        assert lin.weight_q.dtype == torch.uint8 and lin.weight_q.is_cuda
        deq = dequantize_mxfp4(lin.weight_q, lin.weight_scale, torch.bfloat16)
        assert torch.equal(lin.weight, deq)
    batch = _decode_batch(engine, M).to(DEV)
    saved = [lin.weight_q for lin in lins]
    with torch.inference_mode():
        got = engine.model.forward(batch, engine.kv_pool).float()
        try:
            for lin in lins:
                lin.weight_q = None
            ref = engine.model.forward(batch, engine.kv_pool).float()
        finally:
            for lin, w_q in zip(lins, saved):
                lin.weight_q = w_q
    assert got.shape == (M, engine.spec.vocab_size)
    torch.testing.assert_close(got, ref, atol=3e-2, rtol=3e-2)


def test_graph_replay_equals_eager(engine):
    """Bucket 4 for three rows (one pad row); several replays, each equal to
    the eager forward of the padded batch."""
    runner = DecodeGraphRunner(engine.model, engine.kv_pool, DEV, engine._scratch_block,
                               max_blocks_per_seq=G.MAX_BLOCKS, max_bucket=G.MAX_BUCKET)
    batch = _decode_batch(engine, 3)
    padded = G.padded_decode_batch(
        batch, 4, engine._scratch_block, G.MAX_BLOCKS, engine.kv_pool.block_size)
    with torch.inference_mode():
        eager = engine.model.forward(padded.to(DEV), engine.kv_pool).clone()
        for _ in range(3):
            out = runner.run(batch)
            torch.cuda.synchronize()
            assert torch.equal(out, eager[:3])
    assert sorted(runner._graphs) == [4]
