"""On CPU the MoE routing ops are the torch references that MoEMLP runs: the
flag changes nothing there."""

import torch

from dts_amd.models.config import get_model_spec
from dts_amd.models.mixtral import MoEMLP
from dts_amd.parallel.tp import TPContext


def test_fused_route_flag_is_inert_on_cpu():
    spec = get_model_spec("mixtral-tiny")
    moe = MoEMLP(spec, TPContext.single(), torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in moe.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    x = torch.randn(9, spec.hidden_size, generator=g).to(torch.bfloat16)
    assert moe.fused_route is False
    base = moe(x)
    moe.fused_route = True
    assert torch.equal(moe(x), base)

