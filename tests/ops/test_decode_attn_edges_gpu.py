"""Decode attention on a bf16 cache, every instantiation, with exact answers.

Selection: each query head has one key that leads every other by a score
margin of >= 45.25, so the output is that key's V row bit for bit; across the
batch every key position 0..519 -- every (split, wave, slot) of a 33-page
sequence -- is selected once. A dropped page, a wrong split boundary or an
off-by-one in `valid` returns 100.0 (the other keys' V) instead. The block
table is permuted with spare blocks and q is a row-strided view.

Guards, kv_len = 0, workspace reuse and other split counts build on the same
inputs (tests/ops/_edge_inputs.py, proven on torch_ref in
test_edge_inputs_cpu.py).
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader
from tests.ops import _edge_inputs as E

ext = _hip_ext_loader.load()
DEV = "cuda:0"
BF16 = torch.bfloat16


def _decode(q, kc, vc, bt, kv_lens, scale):
    out = torch.empty(q.shape, dtype=BF16, device=DEV)
    ext.attn_decode_paged(
        out, q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), kv_lens.to(DEV), scale
    )
    return out.cpu()


@pytest.mark.parametrize("Hq,Hkv,D", E.DECODE_CONFIGS)
def test_selection_exact(Hq, Hkv, D):
    q, kc, vc, bt, kvl, scale, want = E.decode_selection_inputs(Hq, Hkv, D)
    got = _decode(q, kc, vc, bt, kvl, scale)
    wrong = (E.bits(got) != E.bits(want)).any(dim=-1).nonzero()
    print(f"{wrong.shape[0]} of {Hq * q.shape[0]} selected rows differ")
    assert torch.equal(E.bits(got), E.bits(want)), wrong[:8].tolist()


@pytest.mark.parametrize("Hq,Hkv,D", E.DECODE_CONFIGS)
def test_guards(Hq, Hkv, D):
    """NaN in every slot >= kv_len, every unowned block and every block named
    by an unused table entry: the output is finite and bit-equal to the
    unpoisoned run, at kv_lens {1, 15, 16, 17, 63, 64, 65, 520}."""
    q, kc, vc, bt, kvl, scale, _ = E.decode_selection_inputs(Hq, Hkv, D)
    B = q.shape[0]
    rq, rkc, rvc, rbt, _ = E.decode_randn_inputs(Hq, Hkv, D, B)
    lens = E.guard_lens(B)
    assert set(lens.tolist()) == set(E.GUARD_LENS)
    for name, (q_, kc_, vc_, bt_) in (
        ("selection", (q, kc, vc, bt)), ("randn", (rq, rkc, rvc, rbt)),
    ):
        for kv_lens in (lens, kvl):
            clean = _decode(q_, kc_, vc_, bt_, kv_lens, scale)
            kp, vp = E.poison_dead(kc_, vc_, bt_, kv_lens)
            dirty = _decode(q_, kp, vp, bt_, kv_lens, scale)
            assert torch.isfinite(dirty.float()).all(), name
            assert torch.equal(E.bits(dirty), E.bits(clean)), name


@pytest.mark.parametrize("Hq,Hkv,D", [(8, 2, 128), (4, 4, 64)])
def test_guards_fp8_cache(Hq, Hkv, D):
    """The same with an FP8 cache of uniformly random finite codes and the
    NaN code 0x7F as the poison."""
    B = E.SEL_LEN // Hq
    q, rkc, _, bt, scale = E.decode_randn_inputs(Hq, Hkv, D, B)
    g = E.gen(77 + D)
    kc = E.uniform_code_cache(tuple(rkc.shape), g)
    vc = E.uniform_code_cache(tuple(rkc.shape), g)
    for kv_lens in (E.guard_lens(B), torch.full((B,), E.SEL_LEN, dtype=torch.int32)):
        clean = _decode(q, kc, vc, bt, kv_lens, scale)
        kp, vp = E.poison_dead(kc, vc, bt, kv_lens)
        dirty = _decode(q, kp, vp, bt, kv_lens, scale)
        assert torch.isfinite(dirty.float()).all()
        assert torch.equal(E.bits(dirty), E.bits(clean))


@pytest.mark.parametrize("Hq,Hkv,D", E.DECODE_CONFIGS)
def test_kv_len_zero_row(Hq, Hkv, D):
    """A row with kv_len 0 between live rows is exactly 0 and its neighbours
    are bit-equal to a call (same B, so the same workspace) without it."""
    B = 5
    q, kc, vc, bt, scale = E.decode_randn_inputs(Hq, Hkv, D, B)
    live = torch.tensor([520, 17, 300, 64, 1], dtype=torch.int32)
    full = _decode(q, kc, vc, bt, live, scale)
    with_zero = live.clone()
    with_zero[2] = 0
    got = _decode(q, kc, vc, bt, with_zero, scale)
    assert torch.equal(E.bits(got[2]), torch.zeros_like(E.bits(got[2])))
    keep = [0, 1, 3, 4]
    assert torch.isfinite(full.float()).all() and full[2].float().abs().max() > 0
    assert torch.equal(E.bits(got[keep]), E.bits(full[keep]))


@pytest.mark.parametrize("Hq,Hkv,D", E.DECODE_CONFIGS)
def test_workspace_reuse_after_a_long_call(Hq, Hkv, D):
    """Two calls of one (B, Hkv, G, D): first 520 random keys per sequence
    under large queries (every split publishes partials with maxima far above
    45), then the selection inputs cut to kv_len = (b + 1) * Hq, where most
    splits are empty. The answer is still the selected V rows exactly: stale
    partials of empty splits are never combined."""
    q, kc, vc, bt, kvl, scale, want = E.decode_selection_inputs(Hq, Hkv, D)
    B = q.shape[0]
    rq, rkc, rvc, rbt, _ = E.decode_randn_inputs(Hq, Hkv, D, B, q_scale=64.0)
    first = _decode(rq, rkc, rvc, rbt, kvl, scale)
    assert torch.isfinite(first.float()).all()
    short = E.selection_short_lens(Hq, B)
    assert int(short.min()) == Hq and int(short.max()) == E.SEL_LEN
    got = _decode(q, kc, vc, bt, short, scale)
    assert torch.equal(E.bits(got), E.bits(want))


def test_other_split_counts():
    """The split count is read once per process: one fresh child at a time
    runs the selection tests under DTS_DECODE_SPLITS = 1, 3 and 64 (one wave
    chain over all 33 pages; 11 pages per split; 31 empty splits). A child
    that does not exit 0 fails the test and no further child starts."""
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for splits in (1, 3, 64):
        env = dict(os.environ, DTS_DECODE_SPLITS=str(splits))
        r = subprocess.run(
            [sys.executable, "-m", "pytest", __file__, "-q", "-x", "-k", "selection",
             "-p", "no:cacheprovider"],
            env=env, cwd=root, capture_output=True, text=True, timeout=120,
        )
        assert r.returncode == 0, f"splits={splits}:\n{r.stdout[-3000:]}\n{r.stderr[-1000:]}"
        assert "4 passed" in r.stdout, r.stdout[-2000:]
