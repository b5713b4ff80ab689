"""MoEMLP.fused_route on the tiled probe, both grouped GEMM paths: against the
fp32 reference and the unfused module, under graph capture, off by default."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd import ops
from dts_amd.ops import torch_ref
from tests.models.test_moe_tiled_gpu import probe  # noqa: F401  (fixture)

FUSED_OPS = ("moe_route", "moe_sort_gather", "moe_combine")
ROWS = pytest.mark.parametrize("rows", [5, 40])  # grouped skinny path, tiled path


@ROWS
def test_fused_matches_reference_and_unfused(probe, monkeypatch, rows):
    moe, x, ref = probe[0], probe[1][:rows], probe[3][:rows]
    with torch.inference_mode():
        base = moe(x)
        monkeypatch.setattr(moe, "fused_route", True)
        out = moe(x)
        w32, e32 = torch_ref.moe_route(x, moe.router_w, moe.top_k)
        w, e = ops.moe_route(x, moe.router_w, moe.top_k)
    torch.testing.assert_close(out.float(), ref, atol=5e-2, rtol=5e-2)
    same = (e.long() == e32).all(-1) & (w == w32).all(-1)
    assert torch.equal(out[same], base[same])
    torch.testing.assert_close(out.float(), base.float(), atol=5e-2, rtol=5e-2)


@ROWS
def test_fused_path_captures_and_replays_other_routing(probe, monkeypatch, rows):
    moe, x, x2 = probe[0], probe[1][:rows], probe[2][:rows]
    monkeypatch.setattr(moe, "fused_route", True)
    with torch.inference_mode():
        routed = [ops.moe_route(v, moe.router_w, moe.top_k)[1] for v in (x, x2)]
    assert not torch.equal(routed[0].sort(-1).values, routed[1].sort(-1).values)
    static = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.inference_mode():
        for _ in range(2):
            moe(static)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.inference_mode():
        with torch.cuda.graph(g):
            out = moe(static)
        for v in (x, x2, x2):
            static.copy_(v)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, moe(v))


@pytest.mark.parametrize("fused,calls", [(False, 0), (True, 1)])
@ROWS
def test_fused_ops_run_only_with_the_flag(probe, monkeypatch, rows, fused, calls):
    moe = probe[0]
    assert moe.fused_route is False  # the default
    seen = dict.fromkeys(FUSED_OPS, 0)
    for name in FUSED_OPS:
        def counting(*a, _real=getattr(ops, name), _name=name, **kw):
            seen[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counting)
    monkeypatch.setattr(moe, "fused_route", fused)
    with torch.inference_mode():
        moe(probe[1][:rows])
    assert seen == dict.fromkeys(FUSED_OPS, calls)
