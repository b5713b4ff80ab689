"""Input builders for the top-k / min-p sampler tests.

Deterministic CPU tensors, like _edge_inputs.py. test_filter_inputs_cpu.py
proves every construction on torch_ref alone (filtered_probs in fp64); the
GPU file test_sampler_filters_gpu.py moves them to the device.

All rows are built for T = 1 with their maximum at logit 0, so the kernels'
y = (x - max) / T is the logit itself, exactly.
"""

import functools
import math

import torch

from dts_amd.ops import torch_ref
from tests.ops._edge_inputs import (  # noqa: F401  (re-exported)
    S2_SLICES, SAMPLER_ROWS, V1_VOCABS, V2_VOCABS, boundary_indices, gen,
)

T = 1.0
STEP = 0.25  # 8.5 histogram bins of 30/1024, the spacing nucleus_case uses
LADDER_RUNGS = 40
FILLERS = (-25.0, -40.0, float("-inf"))  # in the histogram, below it, -inf
TOP_KS = (1, 2, 5, 17)
MIN_P_RUNG = 6  # min_p between rungs 6 and 7: seven tokens survive
V1_STRIDE = 256  # v1's thread t owns indices t, t + 256, ...


def filler(V):
    return torch.tensor(FILLERS).repeat(V // 3 + 1)[:V].clone()


def support(probs):
    return sorted(probs.nonzero().flatten().tolist())


def ref_probs(logits, top_p=1.0, top_k=0, min_p=0.0):
    """fp64 reference: [V] renormalised probabilities, 0 where dropped."""
    return torch_ref.filtered_probs(logits.double(), T, top_p, top_k, min_p)


def min_p_between(j):
    """Halfway (in y) between rungs j and j + 1: keeps rungs 0..j."""
    return math.exp(-STEP * (j + 0.5))


def slice_of(i, V):
    for s in range(S2_SLICES):
        if s * V // S2_SLICES <= i < (s + 1) * V // S2_SLICES:
            return s
    raise AssertionError(i)


@functools.lru_cache(maxsize=None)
def ladder(V, seed=61):
    """(logits [V], where [n]): rung j = -0.25 j sits at index where[j];
    n = min(40, V) distinct logits. The places are index 0, V - 1 and lo /
    hi - 1 of v2's slices, then random ones, in a shuffled order; all other
    tokens are at -25, -40 or -inf in turn. The top-k set is where[:k] and
    the min-p set at min_p_between(j) is where[:j + 1], by construction."""
    g = gen(seed + V)
    n = min(LADDER_RUNGS, V)
    places = list(dict.fromkeys(boundary_indices(V)))  # unique, ordered
    rest = [i for i in torch.randperm(V, generator=g).tolist() if i not in set(places)]
    places = (places + rest)[:n]
    assert 0 in places and V - 1 in places and len(set(places)) == n
    where = torch.tensor(places)[torch.randperm(n, generator=g)]
    x = filler(V)
    x[where] = -STEP * torch.arange(n, dtype=torch.float32)
    return x, where


TIE_K = 5
TIE_RUNGS = 12


@functools.lru_cache(maxsize=None)
def tie_case(V, seed=67):
    """(logits, k, kept ids, tied ids): twelve rungs; the k-th value (rung
    k - 1) is shared by three tokens. The rung itself is at V - 1 (v2's last
    slice) and the two copies at indices 10 and 10 + 256: the same v1 stride
    class, and another v2 slice than V - 1 (where V is too small for + 256
    the second copy is at 11). The kept set has k + 2 members."""
    g = gen(seed + V)
    k = TIE_K
    a, b = 10, (10 + V1_STRIDE if V > 10 + V1_STRIDE + 1 else 11)
    taken = {a, b, V - 1}
    free = [i for i in torch.randperm(V, generator=g).tolist() if i not in taken]
    where = free[: TIE_RUNGS]
    where[k - 1] = V - 1
    x = filler(V)
    x[torch.tensor(where)] = -STEP * torch.arange(TIE_RUNGS, dtype=torch.float32)
    x[a] = x[b] = -STEP * (k - 1)
    tied = [a, b, V - 1]
    if b == a + V1_STRIDE:
        assert a % V1_STRIDE == b % V1_STRIDE
    assert slice_of(V - 1, V) != slice_of(a, V)
    kept = sorted(where[:k] + [a, b])
    assert len(kept) == k + 2
    return x, k, kept, tied


HEAD = 4
HEAD_MASS = 0.4


@functools.lru_cache(maxsize=None)
def head_tail(V):
    """(logits, head ids): four head tokens at 0, -0.25, -0.5, -0.75 (index
    0, V - 1 and two slice boundaries) hold about 0.4 of the mass; every
    other token shares one logit below the head and together they hold the
    rest."""
    b = boundary_indices(V)
    head = [0, V - 1, b[len(b) // 2], b[len(b) // 2 + 1]]
    assert len(set(head)) == HEAD
    e = torch.exp(-STEP * torch.arange(HEAD, dtype=torch.float64))
    tail_y = math.log(float(e.sum()) * (1 - HEAD_MASS) / HEAD_MASS / (V - HEAD))
    assert tail_y < -STEP * (HEAD - 1) - 1.0  # clearly below the last head token
    x = torch.full((V,), tail_y, dtype=torch.float32)
    x[torch.tensor(head)] = -STEP * torch.arange(HEAD, dtype=torch.float32)
    p = torch.softmax(x.double(), dim=-1)[torch.tensor(head)].sum()
    assert abs(float(p) - HEAD_MASS) < 1e-3
    return x, head


# top-k then top-p: top-k keeps the head, whose renormalised masses are
# 0.350, 0.273, 0.212, 0.165; top_p = 0.5 lies inside the second one, so two
# tokens survive. top-p on the full distribution would keep the whole head
# (0.4 < 0.5) and the intersection with the top 4 would be all four.
ORDER_KP = dict(top_k=HEAD, top_p=0.5, min_p=0.0)
# top-p then min-p: on the full distribution the head's exclusive cumulative
# masses are 0, 0.140, 0.249, 0.334; top_p = 0.3 lies inside the third token,
# so three survive, and min-p (between the head and the tail) removes none of
# them. min-p first would renormalise the head to 0.350, ... and top_p = 0.3
# would then keep the first token only.
ORDER_PM = dict(top_k=0, top_p=0.3, min_p=min_p_between(HEAD - 1))


def other_order_kp(logits, top_k, top_p, min_p):
    """top-p on the full distribution, intersected with the top-k set."""
    nucleus = ref_probs(logits, top_p=top_p) > 0
    topk = ref_probs(logits, top_k=top_k) > 0
    return sorted((nucleus & topk).nonzero().flatten().tolist())


def other_order_pm(logits, top_k, top_p, min_p):
    """min-p first, then top-p on the renormalised survivors."""
    first = ref_probs(logits, min_p=min_p)
    sp, si = torch.sort(first, descending=True)
    keep = (torch.cumsum(sp, 0) - sp) < top_p
    keep[0] = True
    return sorted(si[keep & (sp > 0)].tolist())


FEW_FINITE = 3


@functools.lru_cache(maxsize=None)
def few_finite_rows(V):
    """[32, V] of -inf with three finite entries per row (0, -0.25, -0.5)
    at consecutive slice-boundary indices; returns (logits, ids [32, 3])."""
    idx = list(dict.fromkeys(boundary_indices(V)))
    x = torch.full((SAMPLER_ROWS, V), float("-inf"))
    ids = []
    for r in range(SAMPLER_ROWS):
        row = [idx[(r + j) % len(idx)] for j in range(FEW_FINITE)]
        x[r, torch.tensor(row)] = -STEP * torch.arange(FEW_FINITE, dtype=torch.float32)
        ids.append(row)
    return x, ids


def exact_cases(V):
    """name -> (logits, params, expected kept ids) of the cases whose kept
    set is known by construction: top-k alone, min-p alone, both orders."""
    lad, where = ladder(V)
    ht, head = head_tail(V)
    cases = {}
    for k in TOP_KS:
        cases[f"top_k={k}"] = (
            lad, dict(top_k=k, top_p=1.0, min_p=0.0), sorted(where[:k].tolist())
        )
    cases["min_p"] = (
        lad, dict(top_k=0, top_p=1.0, min_p=min_p_between(MIN_P_RUNG)),
        sorted(where[: MIN_P_RUNG + 1].tolist()),
    )
    cases["top_k->top_p"] = (ht, ORDER_KP, sorted(head[:2]))
    cases["top_p->min_p"] = (ht, ORDER_PM, sorted(head[:3]))
    return cases


CASE_NAMES = [f"top_k={k}" for k in TOP_KS] + ["min_p", "top_k->top_p", "top_p->min_p"]
