"""CPU checks of the dense fp64 reference and, against it, of the project's
models run in fp32 on the torch_ref path through the whole batch script.

* the reference is THE published forward: its fp64 logits equal Hugging
  Face's implementation (built from a config, loaded from the file
  ``save_*_safetensors`` writes, run in fp64) to 1e-9 relative;
* ``rounded(fp32)`` stays within 1e-5 of ``exact`` (fp32 epsilon 6e-8 x
  sqrt of ~2000-term sums x ~60 ops);
* the project's models stay within 4x the ``rounded(fp32)`` noise of
  ``exact`` at every checkpoint and every row. The noise comes from the
  reference alone, never from the model under test;
* the inputs are not degenerate, and Mixtral's routing-gap cap holds.
"""

from __future__ import annotations

import functools

import pytest
import torch
from torch.overrides import TorchFunctionMode

from tests.models import _scenarios as S
from tests.models._dense_ref import dense_forward, read_params

MARGIN = 4.0
SPEC_NAMES = list(S.SPECS)
# (spec, fp8 kv cache): the FP8 pool on CPU is what shows a wrong
# kv_scale row without a GPU
CPU_CASES = [(n, False) for n in SPEC_NAMES] + [("llama-g4-d128", True)]


@functools.lru_cache(maxsize=None)
def _model(spec_name: str, dtype=torch.float32):
    return S.build_model(spec_name, "cpu", dtype)


@functools.lru_cache(maxsize=None)
def _exact(spec_name: str):
    model = _model(spec_name)
    return S.reference_for(model, S.sequences_for(model.spec), S.script_steps())


@functools.lru_cache(maxsize=None)
def _rounded(spec_name: str, fp8_kv: bool):
    model = _model(spec_name)
    return S.reference_for(
        model, S.sequences_for(model.spec), S.script_steps(), mode=torch.float32,
        kv_scales=S.kv_scales_for(model.spec) if fp8_kv else None,
    )


def _checkpoints(spec_name: str, fp8_kv: bool):
    """(step index, key, exact rows, rounded rows) of every checkpoint."""
    L = S.SPECS[spec_name].num_layers
    for i, st in enumerate(S.script_steps()):
        e = S.reference_step(_exact(spec_name), st, L)
        r = S.reference_step(_rounded(spec_name, fp8_kv), st, L)
        for key in e:
            yield i, key, e[key], r[key]


@pytest.mark.parametrize("spec_name", SPEC_NAMES)
def test_rounded_fp32_is_a_small_noise(spec_name):
    worst = 0.0
    for i, key, e, r in _checkpoints(spec_name, False):
        noise = S.noise_of(r, e)
        assert 0.0 < noise < 1e-5, (i, key, noise)
        worst = max(worst, noise)
    print(f"{spec_name}: largest rounded(fp32) noise {worst:.2e}")


@pytest.mark.parametrize("spec_name,fp8_kv", CPU_CASES)
def test_project_model_matches_exact_reference(spec_name, fp8_kv):
    model = _model(spec_name)
    spec = model.spec
    steps = S.script_steps()
    tables, spare = S.block_tables(11)
    pool = S.make_pool(spec, "cpu", torch.float32, fp8_kv)
    S.fill_pool_nan_(pool)
    caps = S.run_script(
        model, pool, S.sequences_for(spec), steps, tables, spare[0], "cpu"
    )
    got = [S.capture_step(c, spec.num_layers) for c in caps]
    worst: dict = {}
    failures = []
    for i, key, e, r in _checkpoints(spec_name, fp8_kv):
        noise = S.noise_of(r, e)
        assert got[i][key].shape == e.shape, (i, key)
        assert bool(torch.isfinite(got[i][key]).all()), (i, key)
        ratio = float(S.row_rel_err(got[i][key], e).max()) / noise
        kind = S.kind_of(key)
        worst[kind] = max(worst.get(kind, 0.0), ratio)
        if not ratio <= MARGIN:
            failures.append((i, key, round(ratio, 2), noise))
    print(f"{spec_name} fp8_kv={fp8_kv}: max error/noise "
          + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not failures, failures[:10]


# ---------------------------------------------------------------------------
# Hugging Face cross-check
# ---------------------------------------------------------------------------

class _UpcastToFp64(TorchFunctionMode):
    """Hugging Face's modules upcast to fp32 by name (RMSNorm, the softmax
    of attention and of the router, the RoPE angles) whatever dtype the
    model runs in. The cross-check wants fp64 on both sides, so while HF's
    own, unpatched forward runs, every such upcast goes to fp64 instead."""

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func is torch.Tensor.float:
            func = torch.Tensor.double
        args = tuple(torch.float64 if a is torch.float32 else a for a in args)
        kwargs = {
            k: torch.float64 if v is torch.float32 else v
            for k, v in (kwargs or {}).items()
        }
        return func(*args, **kwargs)


def _hf_model(spec_name: str, path: str):
    transformers = pytest.importorskip("transformers")
    spec = S.SPECS[spec_name]
    model = _model(spec_name)
    from dts_amd.models import weights

    common = dict(vocab_size=spec.vocab_size, attn_implementation="eager")
    if spec.arch == "gpt2":
        weights.save_gpt2_safetensors(model, path)
        cfg = transformers.GPT2Config(
            n_positions=spec.max_position, n_embd=spec.hidden_size,
            n_layer=spec.num_layers, n_head=spec.num_heads,
            n_inner=spec.intermediate_size, activation_function="gelu_new",
            layer_norm_epsilon=spec.layernorm_eps, resid_pdrop=0.0,
            embd_pdrop=0.0, attn_pdrop=0.0, tie_word_embeddings=True, **common,
        )
        cls = transformers.GPT2LMHeadModel
    else:
        llama_like = dict(
            hidden_size=spec.hidden_size, intermediate_size=spec.intermediate_size,
            num_hidden_layers=spec.num_layers, num_attention_heads=spec.num_heads,
            num_key_value_heads=spec.num_kv_heads, head_dim=spec.head_dim,
            max_position_embeddings=spec.max_position, rms_norm_eps=spec.rms_eps,
            rope_theta=spec.rope_theta, tie_word_embeddings=False,
            attention_dropout=0.0, **common,
        )
        if spec.arch == "llama":
            weights.save_llama_safetensors(model, path)
            cfg = transformers.LlamaConfig(
                hidden_act="silu", attention_bias=False, mlp_bias=False, **llama_like
            )
            cls = transformers.LlamaForCausalLM
        else:
            weights.save_mixtral_safetensors(model, path)
            cfg = transformers.MixtralConfig(
                num_local_experts=spec.num_experts,
                num_experts_per_tok=spec.experts_per_token,
                sliding_window=None, router_jitter_noise=0.0, **llama_like,
            )
            cls = transformers.MixtralForCausalLM
    cfg.save_pretrained(path)
    try:
        extra = {"experts_implementation": "eager"} if spec.arch == "mixtral" else {}
        hf, info = cls.from_pretrained(
            path, local_files_only=True, output_loading_info=True, **extra
        )
    except Exception as e:  # noqa: BLE001
        if spec.arch == "mixtral":
            pytest.skip(f"installed MixtralForCausalLM cannot load the saved key layout: {e}")
        raise
    bad = [k for k in list(info["missing_keys"]) + list(info["unexpected_keys"])
           if "lm_head" not in k or not spec.tie_embeddings]
    if bad and spec.arch == "mixtral":
        pytest.skip(f"installed MixtralForCausalLM does not accept the saved key layout: {bad[:4]}")
    assert not bad, bad
    hf = hf.double().eval()
    if spec.arch != "gpt2":
        # the one buffer HF computes (in fp32) when the model is built
        i = torch.arange(0, spec.head_dim, 2, dtype=torch.float64)
        rot = hf.model.rotary_emb
        assert rot.inv_freq.shape == i.shape and float(rot.attention_scaling) == 1.0
        rot.inv_freq = 1.0 / (spec.rope_theta ** (i / spec.head_dim))
    return hf


@pytest.mark.parametrize("spec_name", SPEC_NAMES)
def test_exact_reference_is_the_hugging_face_forward(spec_name, tmp_path):
    hf = _hf_model(spec_name, str(tmp_path))
    seqs = S.sequences_for(S.SPECS[spec_name])
    exact = _exact(spec_name)
    worst = 0.0
    for name in ("A", "B", "S7", "X2"):
        with torch.no_grad(), _UpcastToFp64():
            logits = hf(input_ids=torch.tensor([seqs[name]])).logits[0]
        assert logits.dtype == torch.float64
        ref = exact[name]["logits"]
        rel = float((logits - ref).norm() / ref.norm())
        worst = max(worst, rel, float(S.row_rel_err(logits, ref).max()))
    print(f"{spec_name}: max relative difference to Hugging Face {worst:.2e}")
    assert worst <= 1e-9, worst


# ---------------------------------------------------------------------------
# the scenario itself
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mixtral_routing_gap_cap_is_zero_exclusions(dtype):
    """The committed token lists leave >= ROUTING_GAP between the 2nd and
    the 3rd expert at EVERY token of every layer, for the weights the GPU
    tests use (bf16) and the ones the CPU tests use (fp32)."""
    model = _model("mixtral-g4-d128", dtype)
    seqs = S.sequences_for(model.spec)
    assert set(seqs) == set(S.SEQ_NAMES)
    refs = dense_forward(model, [seqs[n] for n in S.SEQ_NAMES])
    n_tok = sum(p.shape[0] for r in refs for p in r["router_probs"])
    assert n_tok == model.spec.num_layers * sum(t for _, t in S.SEQ_LENGTHS.values())
    assert S.min_routing_gap(refs) >= S.ROUTING_GAP
    # and more than one expert pair is in use
    pairs = {
        tuple(sorted(torch.topk(row, 2).indices.tolist()))
        for r in refs for p in r["router_probs"] for row in p
    }
    assert len(pairs) >= 4, pairs


@pytest.mark.parametrize("spec_name", SPEC_NAMES)
def test_inputs_are_not_degenerate(spec_name):
    model = _model(spec_name)
    spec = model.spec
    P = read_params(model)
    names = ("ln1", "ln2") if spec.arch != "gpt2" else (
        "ln1_w", "ln1_b", "ln2_w", "ln2_b", "bq", "bk", "bv", "bo", "b_fc", "b_proj")
    tensors = [(f"layer{i}.{n}", L[n]) for i, L in enumerate(P["layers"]) for n in names]
    tensors += [(n, P[n]) for n in (("norm",) if spec.arch != "gpt2" else ("lnf_w", "lnf_b"))]
    for name, t in tensors:
        assert bool((t > t.mean()).any()) and bool((t < t.mean()).any()), name
        if name.endswith(("ln1", "ln2", "norm", "_w")):
            assert 0.5 <= float(t.min()) and float(t.max()) <= 1.5, name
            assert float(t.std()) > 0.2, name
    # layer norms differ from each other (swapped ln1 / ln2 must show)
    L0 = P["layers"][0]
    a, b = ("ln1", "ln2") if spec.arch != "gpt2" else ("ln1_w", "ln2_w")
    assert not torch.equal(L0[a], L0[b])
    # a few embedding rows sit near the epsilon of the first norm
    eps = spec.rms_eps if spec.arch != "gpt2" else spec.layernorm_eps
    seqs = S.sequences_for(spec)
    emb = P["embed"] if spec.arch != "gpt2" else None
    near = 0
    for name, toks in seqs.items():
        for pos, t in enumerate(toks):
            if spec.arch == "gpt2":
                x = P["wte"][t] + P["wpe"][pos]
                ms = float(x.var(unbiased=False))
            else:
                ms = float(emb[t].pow(2).mean())
            near += int(0.3 * eps <= ms <= 3 * eps)
    assert near >= 3, near
    # no residual checkpoint of the reference is constant across rows
    for i, key, e, _ in _checkpoints(spec_name, False):
        if key.startswith("resid"):
            assert float((e - e.mean(dim=0)).norm(dim=-1).min()) > 1e-3 * float(
                e.norm(dim=-1).max()
            ), (i, key)


def test_script_shapes_paths_and_block_tables():
    steps = S.script_steps()
    assert [len(s.rows()) for s in steps] == [73, 48, 3, 3, 3, 63, 12, 12, 6, 18, 17]
    mixed = steps[S.STEP_MIXED]
    assert mixed.prefill and mixed.decode
    assert len(set(mixed.sample)) == len(mixed.sample) < len(mixed.rows())
    assert mixed.sample != sorted(mixed.sample)
    # MoE: T * top_k <= 64 takes the grouped GEMM, everything else the loop
    k = S.SPECS["mixtral-g4-d128"].experts_per_token
    assert tuple(i for i, s in enumerate(steps) if len(s.rows()) * k <= 64) == S.GROUPED_STEPS
    tables, spare = S.block_tables(11)
    owned = [b for t in tables.values() for b in t]
    assert len(set(owned)) == len(owned) and len(spare) == S.NUM_SPARE
    assert sorted(owned + spare) == list(range(S.NUM_BLOCKS))
    assert owned != sorted(owned)
