"""Last-token logits with an FP8 (e4m3) KV cache against the bf16 cache.

llama-3-8b-2l with RANDOM weights and a random 512-token prompt: the
numbers say how far the quantised cache moves the logits of this synthetic
model, not what it does to a trained one. Prints one JSON line with the
cosine and the max absolute difference, after the prompt's prefill and
after one decode step on the token the bf16 engine sampled.

--kv-scales VALUE (calibrate, or a JSON file of save_kv_scales) adds the
FP8 cache with those per-head scales and prints a second line, so unit and
calibrated scales stand side by side. --v-shift E multiplies the v rows of
qkv_proj by 2^E and o_proj by 2^-E first (the same function, exactly, with
V moved by 2^E): the unmodified random model's K/V sit near 1.0, where the
unit scale is already adequate.
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


def _arg(flag):
    if flag in sys.argv:
        return sys.argv[sys.argv.index(flag) + 1]
    return None


def _shift_v(model, e):
    spec = model.spec
    off = (spec.num_heads + spec.num_kv_heads) * spec.head_dim
    with torch.no_grad():
        for layer in model.layers:
            layer.attn.qkv_proj.weight[off:] *= 2.0**e
            layer.attn.o_proj.weight *= 2.0**-e


def main():
    kv_scales = _arg("--kv-scales")
    v_shift = int(_arg("--v-shift") or 0)
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
    configs = [("bf16", None, None), ("fp8", "fp8", None)]
    if kv_scales:
        configs.append(("fp8_scaled", "fp8", kv_scales))
    shared_model = None
    for name, kv, scales in configs:
        engine = ServingEngine(
            model_name=model, device=device, dtype=dtype,
            kv_memory_bytes=1 << 30, weight_seed=0, kv_cache_dtype=kv, spec_k=0,
            model=shared_model,
        )
        if shared_model is None:
            shared_model = engine.model
            if v_shift:
                _shift_v(shared_model, v_shift)
        if scales == "calibrate":
            engine.calibrate_kv_scales([prompt])
        elif scales:
            engine.load_kv_scales(scales)
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
    for name, _, scales in configs[1:]:
        rec = {"probe": f"kv_fp8_logits_{model}_random_weights_prompt512",
               "kv_scales": "unit" if scales is None else scales,
               "v_shift_log2": v_shift}
        for i, phase in enumerate(("prefill", "decode")):
            a, b = out["bf16"][i], out[name][i]
            rec[f"{phase}_cosine"] = round(float(torch.nn.functional.cosine_similarity(a, b, dim=0)), 6)
            rec[f"{phase}_rel_l2"] = round(float((a - b).norm() / a.norm()), 5)
            rec[f"{phase}_max_abs_diff"] = round(float((a - b).abs().max()), 4)
            rec[f"{phase}_logit_absmax"] = round(float(a.abs().max()), 3)
            rec[f"{phase}_argmax_equal"] = bool(a.argmax() == b.argmax())
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
