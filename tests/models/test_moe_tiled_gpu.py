"""MoEMLP's tiled grouped-GEMM path (T * top_k > 64, `tiled = True`) at module
level: against a per-token fp32 reference of the routed mixture, under graph
capture, and which grouped op each step size calls."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd import ops
from dts_amd.models.config import ModelSpec
from dts_amd.models.mixtral import MoEMLP
from dts_amd.parallel.tp import TPContext

T, H, TOP_K, ROUTING_GAP = 40, 512, 2, 1e-3


def _probs(moe, x):
    return torch.softmax(F.linear(x.float(), moe.router_w.float()), -1)


def _draw(moe, seed):
    """T rows whose 2nd and 3rd router probabilities lie >= 2 ROUTING_GAP apart"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(4 * T, H, generator=g).to(torch.bfloat16).cuda()
    top = _probs(moe, x).topk(3).values
    return x[top[:, 1] - top[:, 2] >= 2 * ROUTING_GAP][:T].contiguous()


@pytest.fixture(scope="module")
def probe():
    """(moe, x, x2, fp32 reference of moe(x), expert histograms of x and x2)"""
    spec = ModelSpec(
        name="moe-tiled-probe", arch="mixtral", vocab_size=512, hidden_size=H,
        intermediate_size=512, num_layers=1, num_heads=4, num_kv_heads=4, head_dim=128,
        rope_theta=1e4, max_position=2048, num_experts=4, experts_per_token=TOP_K,
    )
    torch.manual_seed(3)
    moe = MoEMLP(spec, TPContext.single(), torch.bfloat16).to("cuda")
    with torch.no_grad():
        moe.router_w.normal_(0, 0.02)
        moe.gate_up_w.normal_(0, 0.05)
        moe.down_w.normal_(0, 0.05)
    moe.tiled = True
    x, x2 = _draw(moe, 5), _draw(moe, 6)
    assert x.shape == x2.shape == (T, H)
    top, e = _probs(moe, x).topk(3)
    assert float((top[:, 1] - top[:, 2]).min()) >= ROUTING_GAP
    w = top[:, :TOP_K] / top[:, :TOP_K].sum(-1, keepdim=True)
    ref = torch.zeros(T, H, dtype=torch.float32, device="cuda")
    for t in range(T):
        for j in range(TOP_K):
            ei = int(e[t, j])
            gu = F.linear(x[t].float(), moe.gate_up_w[ei].float())
            act = F.silu(gu[:512]) * gu[512:]
            ref[t] += float(w[t, j]) * F.linear(act, moe.down_w[ei].float())
    hist = [torch.bincount(_probs(moe, v).topk(TOP_K).indices.flatten(),
                           minlength=4).tolist() for v in (x, x2)]
    return moe, x, x2, ref, hist


def test_tiled_matches_reference(probe):
    moe, x, _, ref, _ = probe
    with torch.inference_mode():
        out = moe(x)
    torch.testing.assert_close(out.float(), ref, atol=5e-2, rtol=5e-2)


def test_tiled_path_captures_and_replays_other_routing(probe):
    moe, x, x2, _, hist = probe
    assert hist[0] != hist[1]
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


@pytest.mark.parametrize("rows,grouped,tiled", [(T, 0, 2), (5, 2, 0)])
def test_which_grouped_op_runs(probe, monkeypatch, rows, grouped, tiled):
    calls = {"moe_grouped_linear": 0, "moe_grouped_gemm": 0}
    for name in calls:
        def counting(*a, _real=getattr(ops, name), _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counting)
    with torch.inference_mode():
        probe[0](probe[1][:rows])
    assert calls == {"moe_grouped_linear": grouped, "moe_grouped_gemm": tiled}
