"""The causal boundary of prefill attention, exactly.

A probe query (position p, one q head) scores 45.25 (D = 128) on the key at
its own position and twice that on the key at p + 1, which is in the future
and must be masked: the output is V[p] bit for bit, or V[p + 1] = 100.0 if
the mask is one key late. For the last position of a sequence the tempting
key sits in slot kv_len of the last page. Probes stand at the first and last
query of each chunk and on both sides of every 16-, 32- and 64-key boundary;
the variants are v6 (default), v5 and v1, at every (G, D) instantiation.

Inputs: tests/ops/_edge_inputs.py; test_edge_inputs_cpu.py shows that
torch_ref returns the probes exactly, and does not once the mask is shifted
by one.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader, torch_ref
from tests.ops import _edge_inputs as E

ext = _hip_ext_loader.load()
DEV = "cuda:0"
BF16 = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _reference(G, D):
    q, cu_q, q_pos, kc, vc, bt, kvl, scale, _ = E.prefill_probe_inputs(G, D)
    return torch_ref.attn_prefill_paged(
        q.float(), cu_q, q_pos, kc.float(), vc.float(), bt, kvl, scale
    )


@pytest.mark.parametrize("variant", E.PREFILL_VARIANTS)
@pytest.mark.parametrize("G,D", E.PREFILL_GD)
def test_causal_probes_exact(G, D, variant):
    q, cu_q, q_pos, kc, vc, bt, kvl, scale, probes = E.prefill_probe_inputs(G, D)
    out = torch.empty(q.shape, dtype=BF16, device=DEV)
    ext.attn_prefill_paged(
        out, q.to(DEV), cu_q.to(DEV), q_pos.to(DEV), kc.to(DEV), vc.to(DEV),
        bt.to(DEV), kvl.to(DEV), scale, swz=variant,
    )
    got = out.cpu()
    assert torch.isfinite(got.float()).all()
    wrong = [
        (s, p, head) for row, head, v, s, p in probes
        if not torch.equal(E.bits(got[row, head]), E.bits(v))
    ]
    print(f"{len(wrong)} of {len(probes)} probes differ: {wrong[:8]}")
    assert not wrong
    # every row, the zero queries (plain causal averages of V) included
    ref = _reference(G, D)
    print(f"max abs diff {(got.float() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got.float(), ref, atol=2.5e-2, rtol=2.5e-2)
