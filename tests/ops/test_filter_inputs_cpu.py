"""The top-k / min-p reference (torch_ref.filtered_probs, top_p_sample with
top_ks / min_ps) and the inputs of test_sampler_filters_gpu.py, proven on the
reference alone: every kept set the GPU file asserts is first shown here to be
the reference's own set for that input."""

import math

import pytest
import torch

from dts_amd.ops import torch_ref
from tests.ops import _filter_inputs as F

VOCABS = sorted(set(F.V1_VOCABS + F.V2_VOCABS))


@pytest.mark.parametrize("V", VOCABS)
def test_ladder_sets_are_exact(V):
    x, where = F.ladder(V)
    n = len(where)
    assert n == min(F.LADDER_RUNGS, V) and len(set(x[where].tolist())) == n
    assert {0, V - 1} <= set(where.tolist())
    assert set(F.boundary_indices(V)) <= set(where.tolist())
    others = torch.ones(V, dtype=torch.bool)
    others[where] = False
    assert (x[others] <= -25.0).all()
    for k in F.TOP_KS + (n,):
        if k < V:
            assert F.support(F.ref_probs(x, top_k=k)) == sorted(where[:k].tolist())
    for j in (0, F.MIN_P_RUNG, n - 2):
        got = F.support(F.ref_probs(x, min_p=F.min_p_between(j)))
        assert got == sorted(where[: j + 1].tolist())
    # the rungs are 8.5 bins apart and min_p sits 4.25 bins from both
    # neighbours: a cut at y >= log(min_p) gives the same set
    y = x.double()
    assert F.support(y >= math.log(F.min_p_between(F.MIN_P_RUNG))) == sorted(
        where[: F.MIN_P_RUNG + 1].tolist()
    )


@pytest.mark.parametrize("V", VOCABS)
def test_exact_cases_match_reference(V):
    for name, (x, params, kept) in F.exact_cases(V).items():
        p = F.ref_probs(x, **params)
        assert F.support(p) == kept, name
        assert abs(float(p.sum()) - 1.0) < 1e-12
        # fp32 evaluation of the reference keeps the same set
        p32 = torch_ref.filtered_probs(x, F.T, params["top_p"], params["top_k"], params["min_p"])
        assert F.support(p32) == kept, name
        # top_p sits well inside one token's mass: +-1e-3 changes nothing
        for d in (-1e-3, 1e-3):
            q = dict(params, top_p=params["top_p"] + d) if params["top_p"] < 1 else params
            assert F.support(F.ref_probs(x, **q)) == kept, name


@pytest.mark.parametrize("V", VOCABS)
def test_tie_at_kth_keeps_all_three(V):
    x, k, kept, tied = F.tie_case(V)
    assert len(set(x[torch.tensor(tied)].tolist())) == 1
    assert float(x[tied[0]]) == float(torch.topk(x, k).values[-1])
    assert F.support(F.ref_probs(x, top_k=k)) == kept and len(kept) == k + 2
    assert set(tied) <= set(kept)
    assert F.slice_of(tied[0], V) != F.slice_of(tied[2], V)
    if V > 10 + F.V1_STRIDE + 1:
        assert tied[0] % F.V1_STRIDE == tied[1] % F.V1_STRIDE


@pytest.mark.parametrize("V", VOCABS)
def test_order_cases_tell_the_orders_apart(V):
    x, head = F.head_tail(V)
    spec = F.support(F.ref_probs(x, **F.ORDER_KP))
    other = F.other_order_kp(x, **F.ORDER_KP)
    assert spec == sorted(head[:2]) and other == sorted(head) and spec != other
    spec = F.support(F.ref_probs(x, **F.ORDER_PM))
    other = F.other_order_pm(x, **F.ORDER_PM)
    assert spec == sorted(head[:3]) and other == [head[0]] and spec != other


@pytest.mark.parametrize("V", VOCABS)
def test_degenerate_cases(V):
    x, where = F.ladder(V)
    plain = torch.softmax(x.double() / F.T, dim=-1)
    for k in (0, V, V + 7):
        got = F.ref_probs(x, top_k=k)  # renormalised once more: a few ulp
        assert F.support(got) == F.support(plain), k
        torch.testing.assert_close(got, plain, rtol=1e-14, atol=0)
    kth = torch.topk(x, V - 1).values[-1]
    assert F.support(F.ref_probs(x, top_k=V - 1)) == F.support((x >= kth) & (plain > 0))
    top = int(torch.argmax(x))
    assert top == int(where[0])
    assert F.support(F.ref_probs(x, top_k=1)) == [top]
    assert F.support(F.ref_probs(x, min_p=1.0)) == [top]
    # more than the finite entries: the k-th logit is -inf, nothing is cut,
    # and only the finite entries carry mass
    rows, ids = F.few_finite_rows(V)
    for r in (0, 7, F.SAMPLER_ROWS - 1):
        assert F.support(F.ref_probs(rows[r], top_k=F.FEW_FINITE + 4)) == sorted(ids[r])


def test_top_p_sample_without_filters_is_unchanged():
    """top_ks=None, and disabled rows of a filtered call, reproduce the
    three-argument call for the same generators."""
    g = F.gen(5)
    V = 1000
    logits = torch.randn(6, V, generator=g) * 3
    temps = torch.tensor([0.0, 0.7, 1.0, 1.3, 0.7, 1.0])
    top_ps = torch.tensor([0.9, 0.9, 1.0, 0.5, 0.3, 0.95])

    def gens():
        return [torch.Generator().manual_seed(100 + i) for i in range(6)]

    want = torch_ref.top_p_sample(logits, temps, top_ps, gens())
    assert torch.equal(torch_ref.top_p_sample(logits, temps, top_ps, gens(), None, None), want)
    off_k = torch.tensor([0, 0, V, V + 7, 0, 0], dtype=torch.int32)
    off_p = torch.zeros(6)
    assert torch.equal(torch_ref.top_p_sample(logits, temps, top_ps, gens(), off_k, off_p), want)
    # greedy ignores the filters
    on_k = torch.full((6,), 3, dtype=torch.int32)
    got = torch_ref.top_p_sample(logits, temps, top_ps, gens(), on_k, torch.full((6,), 0.5))
    assert int(got[0]) == int(want[0]) == int(torch.argmax(logits[0]))


def test_top_p_sample_draws_inside_the_filtered_set():
    V = 1000
    x, where = F.ladder(V)
    rows = x.repeat(8, 1)
    ks = torch.tensor([1, 2, 5, 17, 0, 0, 3, 3], dtype=torch.int32)
    mps = torch.tensor([0, 0, 0, 0, F.min_p_between(2), 1.0, F.min_p_between(1), 0.0])
    tps = torch.tensor([1.0] * 7 + [0.5])
    sizes = [1, 2, 5, 17, 3, 1, 2, 2]
    for call in range(20):
        gens = [torch.Generator().manual_seed(call * 8 + i) for i in range(8)]
        got = torch_ref.top_p_sample(rows, torch.ones(8), tps, gens, ks, mps)
        for r, tok in enumerate(got.tolist()):
            assert tok in where[: sizes[r]].tolist(), (call, r, tok)
