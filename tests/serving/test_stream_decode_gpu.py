"""Greedy decode of llama-3-8b-2l (the real Llama-3-8B layer shapes: o, qkv
and down are the projections the stream skinny GEMM is for) with
DTS_SKINNY_UNROLL=4 (gemm_skinny_kernel everywhere the persistent rule does
not apply) and with DTS_SKINNY_UNROLL=32 (the stream kernel wherever it
fits): eight steps at batch 1 and at batch 8, per-step logits torch.equal.

The pin is read once per process, so each setting runs in a fresh child,
one after the other, each under its own timeout; the second child is not
started if the first failed.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

CHILD = r"""
import sys
import torch
from dts_amd.serving import ServingEngine
from dts_amd.serving.batch import ForwardBatch

DEV = "cuda:0"
STEPS = 8
eng = ServingEngine(model_name="llama-3-8b-2l", device=DEV, dtype=torch.bfloat16,
                    kv_memory_bytes=1 << 30, weight_seed=0)
bs = eng.kv_pool.block_size
assert bs >= STEPS
saved = {}
for M in (1, 8):
    rows = torch.arange(M)
    tokens = (rows * 7919 + 300) % 100000
    per_step = []
    for s in range(STEPS):
        # row i decodes position s of its own block i
        batch = ForwardBatch(
            token_ids=tokens,
            positions=torch.full((M,), s, dtype=torch.long),
            slot_mapping=rows * bs + s,
            num_decode_seqs=M,
            decode_block_tables=rows.to(torch.int32).view(M, 1),
            decode_kv_lens=torch.full((M,), s + 1, dtype=torch.int32),
            sample_indices=rows.clone(),
        )
        with torch.inference_mode():
            logits = eng.model.forward(batch.to(DEV), eng.kv_pool)
        assert logits.shape == (M, eng.spec.vocab_size)
        assert bool(torch.isfinite(logits.float()).all())
        per_step.append(logits.cpu())
        tokens = logits.float().argmax(dim=-1).cpu()
    saved[M] = torch.stack(per_step)
eng.stop()
torch.save(saved, sys.argv[1])
"""


def test_stream_pin_gives_the_same_logits(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    outs = {}
    for pin in ("4", "32"):
        path = tmp_path / f"logits_unroll{pin}.pt"
        env = dict(os.environ, DTS_SKINNY_UNROLL=pin)
        env.pop("DTS_SKINNY_PERSISTENT", None)
        r = subprocess.run([sys.executable, "-c", CHILD, str(path)], env=env, cwd=root,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, f"unroll={pin}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
        outs[pin] = torch.load(path)
    for M in (1, 8):
        a, b = outs["4"][M], outs["32"][M]
        assert a.shape == b.shape and a.shape[0] == 8 and a.shape[1] == M
        # the decode moved: later steps differ from the first
        assert not torch.equal(a[0], a[-1])
        assert torch.equal(a, b), M
