"""rope_kv_append and kv_append on a bf16 cache: the copies are bit copies
and are tested as such; the rotation is tested against fp64.

q, k and v are column ranges of one fused qkv buffer (row-strided views),
T = 37 tokens go to a random permutation of slots over 6 blocks, and the
caches start out full of a sentinel. D = 64 makes `half` (32) smaller than a
wave; (Hq, Hk) = (5, 1) makes the unit count no multiple of the 4 waves of a
workgroup. Inputs: tests/ops/_edge_inputs.py, proven on torch_ref in
test_edge_inputs_cpu.py.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.ops import _hip_ext_loader
from tests.ops import _edge_inputs as E

ext = _hip_ext_loader.load()
DEV = "cuda:0"


def _assert_append(kc, vc, slots, k, v):
    assert torch.equal(E.bits(E.cache_rows(vc, slots)), E.bits(v))
    assert torch.equal(E.bits(E.cache_rows(kc, slots)), E.bits(k))
    for c in (kc, vc):
        assert (E.untouched_rows(c, slots) == E.SENTINEL).all()


@pytest.mark.parametrize("Hq,Hk", E.ROPE_HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_rope_kv_append(D, Hq, Hk):
    fused, pos, cos, sin, slots = E.rope_inputs(D, Hq, Hk)
    dev = fused.to(DEV)
    q, k, v = E.split_qkv(dev, Hq, Hk, D)
    assert not k.is_contiguous()
    kc, vc = E.sentinel_cache(Hk, D).to(DEV), E.sentinel_cache(Hk, D).to(DEV)
    ext.rope_kv_append(
        q, k, v, pos.to(DEV), cos.to(DEV), sin.to(DEV), kc, vc, slots.to(DEV)
    )
    after = dev.cpu()
    q0, k0, v0 = E.split_qkv(fused, Hq, Hk, D)
    q1, k1, v1 = E.split_qkv(after, Hq, Hk, D)
    # the v columns of the fused buffer are unchanged
    assert torch.equal(E.bits(v1), E.bits(v0))
    # k cache = k after the call, v cache = v, everything else untouched
    _assert_append(kc.cpu(), vc.cpu(), slots, k1, v0)
    for name, got, x in (("q", q1, q0), ("k", k1, k0)):
        ref, slack = E.rope64(x, pos, cos, sin)
        assert torch.isfinite(got.float()).all()
        err = E.ulp_err(got, ref, slack)
        print(f"rope {name} D={D} Hq={Hq} Hk={Hk}: {err:.5f} ulp over the slack")
        assert err <= 1.0
    # and the rotation did something
    assert not torch.equal(q1, q0)


@pytest.mark.parametrize("Hk", [2, 12, 1])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_bf16(D, Hk):
    fused, _, _, _, slots = E.rope_inputs(D, 3, Hk)
    dev = fused.to(DEV)
    _, k, v = E.split_qkv(dev, 3, Hk, D)
    assert not k.is_contiguous() and not v.is_contiguous()
    kc, vc = E.sentinel_cache(Hk, D).to(DEV), E.sentinel_cache(Hk, D).to(DEV)
    ext.kv_append(k, v, kc, vc, slots.to(DEV))
    assert torch.equal(E.bits(dev.cpu()), E.bits(fused))
    _, k0, v0 = E.split_qkv(fused, 3, Hk, D)
    _assert_append(kc.cpu(), vc.cpu(), slots, k0, v0)
