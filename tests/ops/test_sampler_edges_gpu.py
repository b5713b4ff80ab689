"""top_p_sample (one workgroup per row) and top_p_sample_v2 (vocab sliced over
16 workgroups per row) at the edges of their index arithmetic and with an
exact nucleus.

- one dominant token at index 0, V - 1 and at lo / hi - 1 of each of v2's
  slices `slice * V / 16`, on odd vocabularies (GPT-2's 50257 among them);
- greedy and sampled rows in one call, top_p varying per row;
- a nucleus whose members sit in histogram bins of their own (logits 0.25 T
  apart = 8.5 bins) and a top_p in the middle of one token's mass, so the
  kernel's bin-granular cut and the reference's sorted cut are the same set:
  membership with no slack, and a 6-sigma count check on every member;
- -inf logits.

Inputs: tests/ops/_edge_inputs.py, proven on torch_ref in
test_edge_inputs_cpu.py.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd import ops
from dts_amd.ops import _hip_ext_loader
from tests.ops import _edge_inputs as E

ext = _hip_ext_loader.load()
DEV = "cuda:0"
SAMPLERS = [("v1", V) for V in E.V1_VOCABS] + [("v2", V) for V in E.V2_VOCABS]


def _sample(which, logits, temps, top_ps, seeds):
    S = logits.shape[0]
    out = torch.full((S,), -7, dtype=torch.long, device=DEV)
    args = (
        out, logits.to(DEV).contiguous(), temps.float().to(DEV),
        top_ps.float().to(DEV), seeds.to(DEV),
    )
    if which == "v2":
        ext.top_p_sample_v2(*args, *ops._sampler_workspace(S, torch.device(DEV)))
    else:
        ext.top_p_sample(*args)
    return out.cpu()


def _seeds(call, S=E.SAMPLER_ROWS):
    return torch.arange(S, dtype=torch.long) + call * S + 1


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_dominant_token_at_every_boundary(which, V):
    logits, idx = E.boundary_logits(V)
    S = logits.shape[0]
    greedy = _sample(which, logits, torch.zeros(S), torch.ones(S), _seeds(0))
    assert torch.equal(greedy, idx)
    for call in range(4):
        got = _sample(which, logits, torch.ones(S), torch.full((S,), 0.5), _seeds(call))
        assert torch.equal(got, idx), call


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_mixed_greedy_and_sampled_rows(which, V):
    logits, temps, top_ps, allowed = E.mixed_rows(V)
    for call in range(8):
        got = _sample(which, logits, temps, top_ps, _seeds(call)).tolist()
        for r, tok in enumerate(got):
            assert tok in allowed[r], (call, r, tok, allowed[r])


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_exact_nucleus(which, V):
    """2048 draws (32 rows of the same logits, distinct seeds, 64 calls):
    every draw is in the reference nucleus, no slack; -inf, -40 and -25
    tokens are never drawn; every nucleus token's count is within
    max(6 sqrt(N p), 25) of N p, p its renormalised reference probability."""
    logits, top_p, ids, pn = E.nucleus_case(V)
    S, calls = E.SAMPLER_ROWS, 64
    rows = logits.repeat(S, 1)
    temps, top_ps = torch.ones(S), torch.full((S,), top_p)
    draws = torch.cat([_sample(which, rows, temps, top_ps, _seeds(c)) for c in range(calls)])
    N = draws.numel()
    assert N == 2048
    outside = set(draws.tolist()) - set(ids.tolist())
    assert not outside, sorted(outside)[:8]
    counts = torch.bincount(draws, minlength=V)[ids]
    for tok, c, p in zip(ids.tolist(), counts.tolist(), pn.tolist()):
        bound = max(6.0 * math.sqrt(N * p), 25.0)
        print(f"token {tok}: {c} draws, expected {N * p:.1f} +- {bound:.1f}")
        assert abs(c - N * p) <= bound


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_single_finite_entry(which, V):
    logits, idx = E.single_entry_rows(V)
    S = logits.shape[0]
    assert torch.equal(_sample(which, logits, torch.zeros(S), torch.ones(S), _seeds(0)), idx)
    for call, p in enumerate((0.3, 1.0)):
        got = _sample(which, logits, torch.ones(S), torch.full((S,), p), _seeds(call))
        assert torch.equal(got, idx), p
