"""GPU forward of LlamaModel / MixtralModel / GPT2Model against the dense
fp64 reference (tests/models/_dense_ref.py), through the fixed batch script
of tests/models/_scenarios.py, eagerly (no graph capture, no engine loop).

Tolerance rule: at every step, for the residual stream after every layer,
the logits of every sampled row and the K/V read back from the pool, the
per-row relative L2 error against ``exact`` is at most MARGIN = 4 times the
``rounded(bf16)`` noise of that checkpoint (RMS over its rows, measured on
the reference alone; with an FP8 KV cache ``rounded`` includes the FP8
store). The margin covers what ``rounded`` cannot model: fp32 reduction
order, the split-KV combine, ``exp`` approximations and the per-row
fluctuation of the noise around its RMS.

Exact rules (``torch.equal``): a different shuffle of physical blocks and
identity block tables change nothing; NaN in every slot the script does not
write changes nothing and leaks nowhere; permuting the rows of the M=12
decode batch permutes its logits; the prefill chunk of step 1 leaves the
cached prefix of A and B's blocks byte-identical.

Observed maximum error/noise ratio per spec, mode and checkpoint kind on an
MI355X (margin 4):

  spec / weights / KV cache           resid  logits      k      v
  llama-g4-d128-wbf16-kvbf16           1.48    1.42   1.48   1.47
  llama-g8-d128-wbf16-kvbf16           1.58    1.45   1.42   1.57
  llama-g1-d64-wbf16-kvbf16            1.53    1.46   1.50   1.44
  mixtral-g4-d128-wbf16-kvbf16         1.55    1.37   1.52   1.60
  gpt2-d64-wbf16-kvbf16                1.33    1.12   1.24   1.27
  llama-g4-d128-wfp8-kvbf16            1.42    1.36   1.48   1.38
  llama-g8-d128-wfp8-kvbf16            1.73    1.47   1.51   1.60
  llama-g1-d64-wfp8-kvbf16             1.49    1.37   1.40   1.49
  llama-g4-d128-wbf16-kvfp8            1.43    1.41   1.36   1.37
  llama-g8-d128-wbf16-kvfp8            1.50    1.46   1.43   1.51
  llama-g1-d64-wbf16-kvfp8             1.85    1.35   1.72   1.50
  mixtral-g4-d128-wbf16-kvfp8          1.81    1.42   1.93   1.59
  gpt2-d64-wbf16-kvfp8                 1.47    1.27   1.27   1.28
  llama-g4-d128-wfp8-kvfp8             1.59    1.27   1.56   1.43

No rounding point had to be added to ``rounded`` beyond those listed in
_dense_ref.py for any ratio to stay under the margin.
"""

from __future__ import annotations

import pytest
import torch

from tests.models import _scenarios as S

pytestmark = pytest.mark.gpu

MARGIN = 4.0
DEV = "cuda"

# (spec, fp8 weights, fp8 kv cache)
CASES = (
    [(n, False, False) for n in S.SPECS]
    # weight_quant covers the Llama family only (models/quant.py)
    + [(n, True, False) for n in S.SPECS if S.SPECS[n].arch == "llama"]
    + [(n, False, True) for n in S.SPECS]
    + [("llama-g4-d128", True, True)]
)


def _case_id(c):
    return f"{c[0]}-w{'fp8' if c[1] else 'bf16'}-kv{'fp8' if c[2] else 'bf16'}"


class Case:
    """One model, its references and the base run, built once per module."""

    def __init__(self, spec_name, fp8_w, fp8_kv):
        self.spec = S.SPECS[spec_name]
        self.fp8_kv = fp8_kv
        self.model = S.build_model(spec_name, DEV, torch.bfloat16, weight_quant=fp8_w)
        assert (getattr(self.model, "weight_quant", None) == "fp8") == fp8_w
        self.seqs = S.sequences_for(self.spec)
        self.steps = S.script_steps()
        scales = S.kv_scales_for(self.spec) if fp8_kv else None
        self.exact = S.reference_for(self.model, self.seqs, self.steps)
        self.rounded = S.reference_for(
            self.model, self.seqs, self.steps, mode=torch.bfloat16, kv_scales=scales
        )
        self.base = self.run(shuffle=11)

    def run(self, shuffle, nan_fill=False, row_perm=None, after_step=None):
        tables, spare = S.block_tables(shuffle)
        pool = S.make_pool(self.spec, DEV, torch.bfloat16, self.fp8_kv)
        if nan_fill:
            S.fill_pool_nan_(pool)
        return S.run_script(
            self.model, pool, self.seqs, self.steps, tables, spare[0], DEV,
            row_perm=row_perm, after_step=after_step,
        )


@pytest.fixture(scope="module", params=CASES, ids=_case_id)
def case(request):
    assert torch.cuda.is_available()
    c = Case(*request.param)
    yield c
    del c
    torch.cuda.empty_cache()


def _assert_same(run, base, what):
    assert len(run) == len(base)
    for i, (a, b) in enumerate(zip(run, base)):
        assert torch.equal(a.logits, b.logits), (what, i, "logits")
        assert bool(torch.isfinite(a.logits).all()), (what, i, "logits")
        for l, (x, y) in enumerate(zip(a.resid, b.resid)):
            assert torch.equal(x, y), (what, i, f"resid{l}")
            assert bool(torch.isfinite(x).all()), (what, i, f"resid{l}")
        assert torch.equal(a.k, b.k) and torch.equal(a.v, b.v), (what, i, "kv")
        assert bool(torch.isfinite(a.k).all() and torch.isfinite(a.v).all()), (what, i)


def test_forward_matches_dense_fp64_reference(case):
    L = case.spec.num_layers
    if case.spec.arch == "mixtral":
        assert S.min_routing_gap(list(case.exact.values())) >= S.ROUTING_GAP
    worst: dict = {}
    failures = []
    for i, st in enumerate(case.steps):
        e = S.reference_step(case.exact, st, L)
        r = S.reference_step(case.rounded, st, L)
        got = S.capture_step(case.base[i], L)
        for key in e:
            assert got[key].shape == e[key].shape, (i, key)
            assert bool(torch.isfinite(got[key]).all()), (i, key)
            noise = S.noise_of(r[key], e[key])
            assert noise > 0, (i, key)
            err = S.row_rel_err(got[key], e[key])
            ratio = float(err.max()) / noise
            kind = S.kind_of(key)
            worst[kind] = max(worst.get(kind, 0.0), ratio)
            if not ratio <= MARGIN:
                failures.append(
                    (i, key, int(err.argmax()), f"{ratio:.2f}", f"{noise:.2e}")
                )
    print("RATIOS " + _case_id((case.spec.name, hasattr(case.model, "weight_quant"),
                                case.fp8_kv))
          + " " + " ".join(f"{k}={v:.2f}" for k, v in sorted(worst.items())))
    assert not failures, failures[:12]


def test_moe_paths_taken(case, monkeypatch):
    """Steps with T * top_k <= 64 run MoEMLP._forward_grouped (two grouped
    GEMMs per layer), every other step the per-expert loop; the dense
    models never reach the grouped GEMM."""
    from dts_amd import ops

    calls = []
    real = ops.moe_grouped_linear

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "moe_grouped_linear", counting)
    per_step = []
    case.run(shuffle=11, after_step=lambda i, pool: per_step.append(len(calls)))
    counts = [b - a for a, b in zip([0] + per_step, per_step)]
    moe = case.spec.arch == "mixtral"
    want = [2 * case.spec.num_layers if moe and i in S.GROUPED_STEPS else 0
            for i in range(len(case.steps))]
    assert counts == want


def test_paging_changes_no_arithmetic(case):
    _assert_same(case.run(shuffle=5), case.base, "other shuffle")
    _assert_same(case.run(shuffle=None), case.base, "identity tables")


def test_nan_in_unwritten_slots_changes_nothing(case):
    _assert_same(case.run(shuffle=11, nan_fill=True), case.base, "NaN fill")


def test_row_permutation_of_m12_decode_permutes_logits(case):
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(12, generator=g).tolist()
    assert perm != sorted(perm)
    run = case.run(shuffle=11, row_perm={S.STEP_M12: perm})
    i = S.STEP_M12
    assert case.steps[i].sample == list(range(12))
    assert torch.equal(run[i].logits, case.base[i].logits[perm])
    for l in range(case.spec.num_layers):
        assert torch.equal(run[i].resid[l], case.base[i].resid[l][perm])
    assert torch.equal(run[i].k, case.base[i].k[:, perm])
    # the step wrote the same cache, so everything after it is unchanged
    _assert_same(run[i + 1 :], case.base[i + 1 :], "after the permuted step")


def test_prefill_chunk_leaves_cached_prefix_bytes(case):
    tables, _ = S.block_tables(11)
    bs = S.BLOCK_SIZE
    a_prefix = torch.tensor([tables["A"][p // bs] * bs + p % bs for p in range(40)])
    b_blocks = torch.tensor(
        [b * bs + o for b in tables["B"] for o in range(bs)
         if (b, o) != (tables["B"][33 // bs], 33 % bs)]  # step 1 appends B[33]
    )
    snaps = {}

    def snap(i, pool):
        if i in (S.STEP_PREFILL_1, S.STEP_MIXED):
            snaps[i] = [S.read_slots(pool, s, raw=True) for s in (a_prefix, b_blocks)]

    case.run(shuffle=11, after_step=snap)
    for before, after in zip(snaps[S.STEP_PREFILL_1], snaps[S.STEP_MIXED]):
        for x, y in zip(before, after):
            assert torch.equal(x, y)
    assert bool((snaps[S.STEP_PREFILL_1][0][0] != 0).any())
