"""The MoE glue kernels (moe_route.hip): route against fp64, sort/gather and
the top-2 combine exactly, and one rejected call per wrapper check."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd import ops
from dts_amd.ops import torch_ref
from tests.ops.test_binding_contracts_gpu import _bf16, _check, ext

DEV, BF16, ROUTING_GAP = "cuda:0", torch.bfloat16, 1e-3


@pytest.mark.parametrize("T,H,E,k", [
    (1, 8, 3, 1), (5, 512, 8, 2), (3, 4104, 64, 8), (7, 64, 4, 4), (33, 4096, 8, 2),
    (2, 8200, 4, 2),  # past 8192 columns the row is not held in registers
])
def test_route_matches_fp64(T, H, E, k):
    """Rows whose first k + 1 sorted fp64 probabilities lie pairwise >=
    ROUTING_GAP apart (so the k-th and (k+1)-th do): picks equal, in order.
    Weights: within 4x the fp32 torch routing's error on the same rows, floor
    1e-6. Measured on an MI355X, in case order: torch 0, 1.3e-7, 2.2e-7, 6.0e-8,
    3.4e-7 (bound 1.4e-6), 6.0e-8; the kernel 0, 1.0e-7, 9.7e-8, 7.9e-8, 1.7e-7,
    7.9e-9."""
    g = torch.Generator().manual_seed(H + E)
    x = torch.randn(64 * T, H, generator=g).to(BF16).to(DEV)
    w = (torch.randn(E, H, generator=g) * 2 / H**0.5).to(BF16).to(DEV)
    probs = torch.softmax(x.double() @ w.double().T, -1)
    p, e = probs.sort(dim=-1, descending=True, stable=True)
    m = min(k, E - 1)
    keep = (p[:, :m] - p[:, 1 : m + 1]).min(-1).values >= ROUTING_GAP
    x, p, e = x[keep][:T].contiguous(), p[keep][:T, :k], e[keep][:T, :k]
    assert x.shape[0] == T
    ref_w = p / p.sum(-1, keepdim=True)
    err32 = float((torch_ref.moe_route(x, w, k)[0].double() - ref_w).abs().max())
    got_w, got_e = ops.moe_route(x, w, k)
    err = float((got_w.double() - ref_w).abs().max())
    print(f"T={T} H={H} E={E} k={k}: torch fp32 err {err32:.2e}, kernel err {err:.2e}")
    assert got_e.dtype == torch.int32 and torch.equal(got_e.long(), e)
    assert err <= max(4 * err32, 1e-6)


@pytest.mark.parametrize("k", [1, 2])
def test_route_tie_takes_lowest_index(k):
    w = torch.zeros(4, 8, dtype=BF16, device=DEV)
    w[0], w[1], w[2] = -1.0, 1.0, 1.0  # experts 1 and 2: bit-equal logits
    got_w, got_e = ops.moe_route(torch.ones(2, 8, dtype=BF16, device=DEV), w, k)
    assert got_e.tolist() == [[1, 2][:k]] * 2
    assert got_w.tolist() == [[1.0 / k] * k] * 2


@pytest.mark.parametrize("name,T,k,E,H", [
    ("P < E", 1, 2, 8, 8), ("one expert", 9, 2, 4, 64), ("gap", 40, 2, 4, 4096),
    ("long scan", 700, 2, 8, 8), ("E = 64", 50, 4, 64, 4104),
])
def test_sort_gather_is_the_stable_sort(name, T, k, E, H):
    experts = torch.randint(0, E, (T, k), generator=torch.Generator().manual_seed(T))
    if name == "one expert":
        experts[:] = 2
    if name == "gap":  # expert 2 of 4 stays empty
        experts[experts == 2] = 3
    experts, x = experts.to(DEV), _bf16(T, H)
    flat = experts.reshape(-1)
    order = torch.argsort(flat, stable=True)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(T * k, device=DEV)
    counts = torch.bincount(flat, minlength=E)
    x_sorted, got_counts, got_offsets, dst = ops.moe_sort_gather(x, experts.int(), E)
    assert torch.equal(dst.long(), inv)
    assert torch.equal(got_counts.long(), counts)
    assert torch.equal(got_offsets.long(), counts.cumsum(0) - counts)
    assert torch.equal(x_sorted, x[order // k])


def test_combine_top2_is_bit_equal_to_torch():
    T, k, H = 37, 2, 4104
    y, w = _bf16(T * k, H), torch.rand(T, k, device=DEV)
    dst = torch.randperm(T * k, device=DEV)
    ref = (y[dst].view(T, k, H).float() * w[..., None]).sum(1).to(BF16)
    assert torch.equal(ops.moe_combine(y, dst.int(), w), ref)


def test_combine_top4_within_one_ulp_of_fp64():
    """Positive terms: no cancellation, so one bf16 ulp of the result holds."""
    T, k, H = 5, 4, 64
    y = (torch.rand(T * k, H, device=DEV) + 0.5).to(BF16)
    w, dst = torch.rand(T, k, device=DEV) + 0.1, torch.randperm(T * k, device=DEV)
    ref = (y[dst].view(T, k, H).double() * w.double()[..., None]).sum(1)
    ulp = 2.0 ** (torch.floor(torch.log2(ref)) - 7)
    assert ((ops.moe_combine(y, dst.int(), w).double() - ref).abs() <= ulp).all()


T_, H_, E_, K_, P_ = 6, 64, 4, 2, 12  # P = T * k
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def _h12(rows):  # contiguous [rows, 12] window of a larger buffer: H % 8 != 0
    return _bf16(rows * 12 + 64)[: rows * 12].view(rows, 12)


def test_moe_route_contract():
    good = dict(e=_z(I32, T_, K_), w=_z(F32, T_, K_), x=_bf16(T_, H_), r=_bf16(E_, H_))
    _check(lambda e, w, x, r: ext.moe_route(e, w, x, r), good, {
        "strided x": dict(x=_bf16(T_, 2 * H_)[:, :H_]),
        "H = 12": dict(x=_h12(T_), r=_h12(E_)),
        "router of 2H columns": dict(r=_bf16(E_, 2 * H_)),
        "E = 65": dict(r=_bf16(65, H_)),
        "int64 experts_out": dict(e=_z(I64, T_, K_)),
        "k = 5 > E": dict(e=_z(I32, T_, 5), w=_z(F32, T_, 5)),
        "weights_out of another k": dict(w=_z(F32, T_, K_ + 1)),
    })


def test_moe_sort_gather_contract():
    good = dict(xs=_bf16(P_, H_), dst=_z(I32, P_), c=_z(I32, E_), o=_z(I32, E_),
                x=_bf16(T_, H_), e=_z(I32, T_, K_))
    _check(lambda xs, dst, c, o, x, e: ext.moe_sort_gather(xs, dst, c, o, x, e), good, {
        "fp32 x": dict(x=_z(F32, T_, H_)),
        "H = 12": dict(x=_h12(T_), xs=_h12(P_)),
        "int64 experts": dict(e=_z(I64, T_, K_)),
        "x_sorted of T rows": dict(xs=_bf16(T_, H_)),
        "int64 dst": dict(dst=_z(I64, P_)),
        "int64 counts": dict(c=_z(I64, E_)),
        "offsets of another length": dict(o=_z(I32, E_ + 1)),
        "E = 65": dict(c=_z(I32, 65), o=_z(I32, 65)),
    })


def test_moe_combine_contract():
    good = dict(out=_bf16(T_, H_), y=_bf16(P_, H_), dst=_z(I32, P_), w=_z(F32, T_, K_))
    _check(lambda out, y, dst, w: ext.moe_combine(out, y, dst, w), good, {
        "fp32 y": dict(y=_z(F32, P_, H_)),
        "H = 12": dict(y=_h12(P_), out=_h12(T_)),
        "weights of another T": dict(w=_z(F32, T_ + 1, K_)),
        "int64 dst": dict(dst=_z(I64, P_)),
        "out of P rows": dict(out=_bf16(P_, H_)),
    })
