"""MoEMLP's tiled path with `tiled_block = 128`: the bits of the 64-row blocks,
with and without the fused routing kernels, and close to an fp32 reference."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd.models.config import ModelSpec
from dts_amd.models.mixtral import MoEMLP
from dts_amd.parallel.tp import TPContext

T, H, INTER, E, TOP_K, ROUTING_GAP = 300, 512, 512, 4, 2, 1e-3


@pytest.fixture(scope="module")
def probe():
    """(moe, x, fp32 CPU reference of moe(x)); one expert owns > 128 rows"""
    spec = ModelSpec(
        name="moe-wide-probe", arch="mixtral", vocab_size=512, hidden_size=H,
        intermediate_size=INTER, num_layers=1, num_heads=4, num_kv_heads=4, head_dim=128,
        rope_theta=1e4, max_position=2048, num_experts=E, experts_per_token=TOP_K,
    )
    torch.manual_seed(3)
    moe = MoEMLP(spec, TPContext.single(), torch.bfloat16)
    with torch.no_grad():
        for p, std in ((moe.router_w, 0.02), (moe.gate_up_w, 0.05), (moe.down_w, 0.05)):
            p.normal_(0, std)
    moe.tiled = True
    router, gate_up, down = moe.router_w.float(), moe.gate_up_w.float(), moe.down_w.float()
    # rows whose 2nd and 3rd router probabilities lie >= 2 ROUTING_GAP apart
    x = torch.randn(4 * T, H, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    top = torch.softmax(F.linear(x.float(), router), -1).topk(3).values
    x = x[top[:, 1] - top[:, 2] >= 2 * ROUTING_GAP][:T].contiguous()
    top, e = torch.softmax(F.linear(x.float(), router), -1).topk(TOP_K)
    assert x.shape == (T, H) and int(torch.bincount(e.flatten()).max()) > 128
    w = top / top.sum(-1, keepdim=True)
    ref = torch.zeros(T, H)
    for ei in range(E):
        t, j = (e == ei).nonzero(as_tuple=True)
        gu = F.linear(x[t].float(), gate_up[ei])
        act = F.silu(gu[:, :INTER]) * gu[:, INTER:]
        ref.index_add_(0, t, w[t, j].unsqueeze(1) * F.linear(act, down[ei]))
    return moe.to("cuda"), x.cuda(), ref


def _forward(moe, x, block, fused):
    moe.tiled_block, moe.fused_route = block, fused
    with torch.inference_mode():
        return moe(x)


@pytest.mark.parametrize("fused", [False, True])
def test_wide_blocks_give_the_bits_of_64_row_blocks(probe, fused):
    moe, x, _ = probe
    assert torch.equal(_forward(moe, x, 128, fused), _forward(moe, x, 64, fused))


def test_wide_matches_reference(probe):
    moe, x, ref = probe
    out = _forward(moe, x, 128, False).float().cpu()
    torch.testing.assert_close(out, ref, atol=5e-2, rtol=5e-2)
