"""sample_filtered (one workgroup per row) and sample_filtered_v2 (gridded):
top-k -> top-p -> min-p on the device, against torch_ref.filtered_probs.

- exact kept sets and 6-sigma counts for top-k alone, min-p alone and the two
  order cases (top-k before top-p, top-p before min-p);
- a tie at the k-th logit across v2 slices and inside one v1 stride class;
- top_k=1 / min_p=1.0 equal the greedy answer; k >= V, k = V - 1 and k above
  the number of finite entries;
- disabled and greedy rows of a filtered call equal the unfiltered binding
  bit for bit; the same call twice; workspace reuse across k=5 / k=0 / k=5;
- every argument check of the two wrappers.

Inputs: tests/ops/_filter_inputs.py, proven on torch_ref in
test_filter_inputs_cpu.py.
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
from tests.ops import _filter_inputs as F

ext = _hip_ext_loader.load()
DEV = "cuda:0"
S = F.SAMPLER_ROWS
SAMPLERS = [("v1", V) for V in F.V1_VOCABS] + [("v2", V) for V in F.V2_VOCABS]


def _vec(v, dtype):
    if not torch.is_tensor(v):
        v = torch.full((S,), v)
    return v.to(dtype).to(DEV)


def _workspaces(n=S):
    dev = torch.device(DEV)
    return (*ops._sampler_workspace(n, dev), *ops._sampler_filter_workspace(n, dev))


def _filtered(which, logits, seeds, temps=1.0, top_p=1.0, top_k=0, min_p=0.0):
    """logits: [S, V] on the device. Scalars are broadcast over the rows."""
    out = torch.full((S,), -7, dtype=torch.long, device=DEV)
    args = (
        out, logits, _vec(temps, torch.float32), _vec(top_p, torch.float32),
        _vec(top_k, torch.int32), _vec(min_p, torch.float32), seeds.to(DEV),
    )
    if which == "v2":
        ext.sample_filtered_v2(*args, *_workspaces())
    else:
        ext.sample_filtered(*args)
    return out.cpu()


def _unfiltered(which, logits, seeds, temps, top_p):
    out = torch.full((S,), -7, dtype=torch.long, device=DEV)
    args = (out, logits, _vec(temps, torch.float32), _vec(top_p, torch.float32), seeds.to(DEV))
    if which == "v2":
        ext.top_p_sample_v2(*args, *ops._sampler_workspace(S, torch.device(DEV)))
    else:
        ext.top_p_sample(*args)
    return out.cpu()


def _seeds(call):
    return torch.arange(S, dtype=torch.long) + call * S + 1


def _rows(x):
    return x.repeat(S, 1).to(DEV).contiguous()


def _draws(which, x, calls=64, **params):
    rows = _rows(x)
    return torch.cat([_filtered(which, rows, _seeds(c), **params) for c in range(calls)])


@pytest.mark.parametrize("case", F.CASE_NAMES)
@pytest.mark.parametrize("which,V", SAMPLERS)
def test_exact_set_and_counts(which, V, case):
    """2048 draws: all inside the exact set; each member's count within
    max(6 sqrt(N p), 25) of N p, p the reference's renormalised probability."""
    x, params, kept = F.exact_cases(V)[case]
    p = F.ref_probs(x, **params)
    assert F.support(p) == kept
    draws = _draws(which, x, **params)
    N = draws.numel()
    assert N == 2048
    outside = set(draws.tolist()) - set(kept)
    assert not outside, sorted(outside)[:8]
    counts = torch.bincount(draws, minlength=V)
    for tok in kept:
        c, want = int(counts[tok]), N * float(p[tok])
        bound = max(6.0 * math.sqrt(want), 25.0)
        print(f"token {tok}: {c} draws, expected {want:.1f} +- {bound:.1f}")
        assert abs(c - want) <= bound


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_tie_at_kth(which, V):
    x, k, kept, tied = F.tie_case(V)
    draws = _draws(which, x, top_k=k)
    outside = set(draws.tolist()) - set(kept)
    assert not outside, sorted(outside)[:8]
    counts = torch.bincount(draws, minlength=V)
    for tok in tied:
        print(f"tied token {tok}: {int(counts[tok])} draws")
        assert int(counts[tok]) >= 1


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_single_survivor_is_greedy(which, V):
    """top_k=1 and min_p=1.0 at T=1 leave the maximum alone."""
    lad, where = F.ladder(V)
    bnd, idx = E.boundary_logits(V)
    for logits, want in ((_rows(lad), torch.full((S,), int(where[0]))), (bnd.to(DEV), idx)):
        greedy = _filtered(which, logits, _seeds(0), temps=0.0)
        assert torch.equal(greedy, want)
        for call in range(4):
            for params in (dict(top_k=1), dict(min_p=1.0), dict(top_k=1, min_p=1.0, top_p=0.3)):
                got = _filtered(which, logits, _seeds(call), **params)
                assert torch.equal(got, greedy), (call, params)


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_degenerate_k(which, V):
    lad, where = F.ladder(V)
    rows = _rows(lad)
    for k in (V, V + 7):  # disabled: the unfiltered sampler, bit for bit
        for call in range(2):
            got = _filtered(which, rows, _seeds(call), top_p=0.9, top_k=k)
            assert torch.equal(got, _unfiltered(which, rows, _seeds(call), 1.0, 0.9)), k
    allowed = set(F.support(F.ref_probs(lad, top_k=V - 1)))
    for call in range(4):
        got = _filtered(which, rows, _seeds(call), top_k=V - 1)
        assert set(got.tolist()) <= allowed
    # k above the number of finite entries: the k-th logit is -inf
    few, ids = F.few_finite_rows(V)
    few = few.to(DEV)
    for call in range(4):
        got = _filtered(which, few, _seeds(call), top_k=F.FEW_FINITE + 4).tolist()
        for r, tok in enumerate(got):
            assert tok in ids[r], (call, r, tok)


def _mixed(V):
    """Per row: logits, temps, top_p, top_k, min_p, and the allowed set of a
    filtered row (None: the row must equal the unfiltered sampler's)."""
    lad, where = F.ladder(V)
    kinds = [
        dict(temps=1.0, top_p=0.9, top_k=0, min_p=0.0),  # disabled
        dict(temps=1.0, top_p=0.9, top_k=V + 3, min_p=0.0),  # disabled: k >= V
        dict(temps=1.0, top_p=1.0, top_k=5, min_p=0.0),
        dict(temps=1.0, top_p=1.0, top_k=0, min_p=F.min_p_between(F.MIN_P_RUNG)),
        dict(temps=1.0, top_p=0.5, top_k=3, min_p=F.min_p_between(0)),
        dict(temps=0.0, top_p=0.9, top_k=4, min_p=0.3),  # greedy
    ]
    cols = {k: [] for k in kinds[0]}
    allowed = []
    for r in range(S):
        kind = kinds[r % len(kinds)]
        for k, v in kind.items():
            cols[k].append(v)
        plain = kind["temps"] <= 0 or (not 1 <= kind["top_k"] < V and kind["min_p"] == 0)
        allowed.append(
            None if plain else set(F.support(F.ref_probs(
                lad, top_p=kind["top_p"], top_k=kind["top_k"], min_p=kind["min_p"])))
        )
    assert allowed[4] == {int(where[0])}  # all three filters: one survivor
    return _rows(lad), {k: torch.tensor(v) for k, v in cols.items()}, allowed


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_disabled_rows_are_the_unfiltered_sampler(which, V):
    rows, params, allowed = _mixed(V)
    for call in range(4):
        got = _filtered(which, rows, _seeds(call), **params)
        old = _unfiltered(which, rows, _seeds(call), params["temps"], params["top_p"])
        again = _filtered(which, rows, _seeds(call), **params)
        assert torch.equal(got, again)  # the same call twice
        plain = torch.tensor([a is None for a in allowed])
        assert torch.equal(got[plain], old[plain])
        for r, a in enumerate(allowed):
            if a is not None:
                assert int(got[r]) in a, (call, r, int(got[r]))


@pytest.mark.parametrize("which,V", SAMPLERS)
def test_workspace_reuse(which, V):
    lad, where = F.ladder(V)
    rows = _rows(lad)
    first = _filtered(which, rows, _seeds(3), top_k=5)
    off = _filtered(which, rows, _seeds(3), top_p=0.9, top_k=0)
    third = _filtered(which, rows, _seeds(3), top_k=5)
    assert torch.equal(third, first)
    assert torch.equal(off, _unfiltered(which, rows, _seeds(3), 1.0, 0.9))
    assert set(first.tolist()) <= set(where[:5].tolist())


def test_ops_dispatch():
    """ops.top_p_sample with top_ks / min_ps: v2 at V >= 4096 and S <= 32, v1
    otherwise; both None is the unfiltered call."""
    for V in (1000, 4099):
        lad, where = F.ladder(V)
        rows = _rows(lad)
        temps, tops = _vec(1.0, torch.float32), _vec(1.0, torch.float32)
        seeds = _seeds(0).to(DEV)
        got = ops.top_p_sample(rows, temps, tops, seeds=seeds, top_ks=_vec(2, torch.int32))
        assert set(got.tolist()) <= set(where[:2].tolist())
        got = ops.top_p_sample(rows, temps, tops, seeds=seeds, min_ps=_vec(1.0, torch.float32))
        assert set(got.tolist()) == {int(where[0])}
        which = "v2" if V >= 4096 else "v1"
        plain = ops.top_p_sample(rows, temps, _vec(0.9, torch.float32), seeds=seeds)
        assert torch.equal(plain.cpu(), _unfiltered(which, rows, _seeds(0), 1.0, 0.9))


# ---------------------------------------------------------------------------
# rejected calls: host-side checks, nothing is launched. Every bad argument
# is at least as large as the good one.
# ---------------------------------------------------------------------------

def _good(V=4099):
    lad, _ = F.ladder(V)
    ws = _workspaces()
    return dict(
        out=torch.zeros(S, dtype=torch.long, device=DEV), logits=_rows(lad),
        temps=_vec(1.0, torch.float32), top_ps=_vec(0.9, torch.float32),
        top_ks=_vec(5, torch.int32), min_ps=_vec(0.05, torch.float32),
        seeds=_seeds(0).to(DEV), ws_max=ws[0], ws_bins=ws[1], ws_slice=ws[2],
        ws_tau=ws[3], ws_cnt=ws[4], ws_xk=ws[5],
    )


# never narrower than the right one
WRONG_DTYPE = {
    torch.float32: torch.float64, torch.int32: torch.int64, torch.int64: torch.float64,
}


def _strided(t):
    return torch.stack([t, t], dim=1)[:, 0]


def _bad_vectors(good, names):
    bad = {}
    for name in names:
        t = good[name]
        bad[f"{name}: dtype"] = {name: t.to(WRONG_DTYPE[t.dtype])}
        bad[f"{name}: length"] = {name: torch.cat([t, t[:1]])}
        bad[f"{name}: strided"] = {name: _strided(t)}
        bad[f"{name}: host tensor"] = {name: t.cpu()}
        bad[f"{name}: 2-d"] = {name: t.view(S, 1)}
    return bad


def _bad_logits(good):
    x = good["logits"]
    return {
        "logits: fp64": dict(logits=x.double()),
        "logits: bf16": dict(logits=x.to(torch.bfloat16)),
        "logits: strided": dict(logits=torch.cat([x, x], dim=1)[:, : x.shape[1]]),
        "logits: 3-d": dict(logits=x.view(S, 1, -1)),
        "logits: host tensor": dict(logits=x.cpu()),
    }


def _expect_rejections(fn, good, bad_cases):
    fn(**good)
    torch.cuda.synchronize()
    for name, bad in bad_cases.items():
        with pytest.raises(RuntimeError):
            fn(**{**good, **bad})
        print(f"rejected: {name}")
    torch.cuda.synchronize()


VECTORS = ["out", "temps", "top_ps", "top_ks", "min_ps", "seeds"]


def test_sample_filtered_contract():
    good = {k: v for k, v in _good(1000).items() if not k.startswith("ws_")}

    def fn(out, logits, temps, top_ps, top_ks, min_ps, seeds):
        ext.sample_filtered(out, logits, temps, top_ps, top_ks, min_ps, seeds)

    _expect_rejections(fn, good, {**_bad_logits(good), **_bad_vectors(good, VECTORS)})


def test_sample_filtered_v2_contract():
    good = _good()

    def fn(out, logits, temps, top_ps, top_ks, min_ps, seeds, ws_max, ws_bins,
           ws_slice, ws_tau, ws_cnt, ws_xk):
        ext.sample_filtered_v2(out, logits, temps, top_ps, top_ks, min_ps, seeds,
                               ws_max, ws_bins, ws_slice, ws_tau, ws_cnt, ws_xk)

    bad = {**_bad_logits(good), **_bad_vectors(good, VECTORS)}
    for name in ("ws_max", "ws_bins", "ws_slice", "ws_tau", "ws_cnt", "ws_xk"):
        t = good[name]
        bad[f"{name}: dtype"] = {name: t.to(WRONG_DTYPE[t.dtype])}
        bad[f"{name}: host tensor"] = {name: t.cpu()}
        bad[f"{name}: strided"] = {name: torch.stack([t, t], dim=-1)[..., 0]}
    # the one check a larger tensor cannot trip: a workspace for fewer rows.
    # It is rejected before anything is enqueued.
    small = _workspaces(S - 1)
    bad["ws_cnt: too small"] = dict(ws_cnt=small[4])
    bad["ws_bins: too small"] = dict(ws_bins=small[1])
    _expect_rejections(fn, good, bad)
