"""Last-token logits with an FP8 (e4m3) KV cache against the bf16 cache.

llama-3-8b-2l with RANDOM weights and a random 512-token prompt: the
numbers say how far the quantised cache moves the logits of this synthetic
model, not what it does to a trained one. Prints one JSON line with the
cosine and the max absolute difference, after the prompt's prefill and
after one decode step on the token the bf16 engine sampled.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from dts_amd.llm.types import SamplingParams  # noqa: E402
from dts_amd.serving import ServingEngine  # noqa: E402


def _step_logits(engine, force_token=None):
    with engine._lock:
        batch = engine.scheduler.schedule()
    with torch.inference_mode():
        logits = engine.model.forward(batch.to(engine.device), engine.kv_pool)
    if engine.device.startswith("cuda"):
        torch.cuda.synchronize()
    seqs = batch._sampled_seqs
    toks = engine.sampler.sample(logits, seqs)
    if force_token is not None:
        toks = [force_token]
    with engine._lock:
        engine.scheduler.advance_computed(batch)
        for seq, tok in zip(seqs, toks):
            engine._handle_sampled(seq, tok)
    return logits[-1].float().cpu(), int(toks[0])


def main():
    prompt = [int(x) for x in torch.randint(300, 100000, (512,),
                                            generator=torch.Generator().manual_seed(0))]
    # --cpu-tiny: dry run of the script itself on the tiny model
    if "--cpu-tiny" in sys.argv:
        model, device, dtype = "llama-tiny", "cpu", torch.float32
        prompt = [t % 200 for t in prompt]
    else:
        model, device, dtype = "llama-3-8b-2l", "cuda:0", torch.bfloat16
    out = {}
    first = None
    for name, kv in (("bf16", None), ("fp8", "fp8")):
        engine = ServingEngine(
            model_name=model, device=device, dtype=dtype,
            kv_memory_bytes=1 << 30, weight_seed=0, kv_cache_dtype=kv, spec_k=0,
        )
        engine.submit_tokens(
            list(prompt), SamplingParams(max_tokens=4, seed=0, temperature=0.0)
        )
        prefill, tok = _step_logits(engine, force_token=first)
        if first is None:
            first = tok
        decode, _ = _step_logits(engine)
        out[name] = (prefill, decode)
        engine.stop()
        del engine
    rec = {"probe": f"kv_fp8_logits_{model}_random_weights_prompt512"}
    for i, phase in enumerate(("prefill", "decode")):
        a, b = out["bf16"][i], out["fp8"][i]
        rec[f"{phase}_cosine"] = round(float(torch.nn.functional.cosine_similarity(a, b, dim=0)), 6)
        rec[f"{phase}_max_abs_diff"] = round(float((a - b).abs().max()), 4)
        rec[f"{phase}_logit_absmax"] = round(float(a.abs().max()), 3)
        rec[f"{phase}_argmax_equal"] = bool(a.argmax() == b.argmax())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
