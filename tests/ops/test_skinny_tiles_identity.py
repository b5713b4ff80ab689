"""Bit-identity of the skinny GEMM across tiles-per-workgroup settings and
of its fused SwiGLU epilogue against the two-kernel path.

Every output element must see the same arithmetic whatever the N tiling
(same per-wave k-chunk order, same 4-way cross-wave sum), so the checks
are torch.equal — no tolerance. Shapes are the smallest at which the
tiling can go wrong: K=512 (minimum), a single tile, an odd tile count
(dead tiles in the last workgroup), N not a multiple of 16, several
workgroups; one long-K case for the k loop.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dts_amd.ops import _hip_ext_loader

    ext = _hip_ext_loader.load()
else:  # collected but skipped off-GPU
    ext = None

DEV = "cuda:0"


def _inputs(M, K, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(DEV)
    return x, w


def _run(x, w, nt, out=None):
    if out is None:
        # poison: elements the kernel fails to write must show up
        out = torch.full(
            (x.shape[0], w.shape[0]), float("nan"), dtype=torch.bfloat16, device=DEV
        )
    ext.gemm_skinny_bf16(out, x, w, tiles_per_wg=nt)
    return out


@pytest.mark.parametrize("nt", [2, 4])
@pytest.mark.parametrize("N", [16, 48, 100, 272])
@pytest.mark.parametrize("M", [1, 7, 16])
def test_tiles_per_wg_bit_identical(M, N, nt):
    x, w = _inputs(M, 512, N)
    ref = _run(x, w, 1)
    got = _run(x, w, nt)
    assert not torch.isnan(ref.float()).any()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("nt", [2, 4])
def test_tiles_per_wg_long_k(nt):
    x, w = _inputs(7, 14336, 64, seed=1)
    assert torch.equal(_run(x, w, nt), _run(x, w, 1))


# (M, N): auto picks 1 tile per workgroup below M=8; 2 at 384 tiles (the
# qkv width); 4 from 1024 tiles above M=8; 4 from 4096 tiles at M=8
@pytest.mark.parametrize(
    "M,N", [(7, 272), (8, 6144), (16, 6144), (16, 16 * 1024), (8, 16 * 4096)]
)
def test_auto_matches_pinned(M, N):
    x, w = _inputs(M, 512, N, seed=2)
    assert torch.equal(_run(x, w, 0), _run(x, w, 1))


def test_explicit_unroll8_rejects_ragged_k():
    x, w = _inputs(4, 512, 32, seed=9)
    out = torch.empty(4, 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="unroll=8"):
        ext.gemm_skinny_bf16(out, x, w, tiles_per_wg=1, unroll=8)


@pytest.mark.parametrize("nt", [2, 4])
def test_tiles_per_wg_strided_x_and_out(nt):
    M, K, N = 6, 512, 100
    g = torch.Generator().manual_seed(3)
    big = torch.randn(M, 2 * K, generator=g).to(torch.bfloat16).to(DEV)
    x = big[:, K:]  # strided rows (fused qkv views)
    _, w = _inputs(M, K, N, seed=4)
    outs = []
    for t in (1, nt):
        out_big = torch.full((M, 2 * N + 8), 7.0, dtype=torch.bfloat16, device=DEV)
        _run(x, w, t, out=out_big[:, 8 : 8 + N])
        outs.append(out_big)
    assert torch.equal(outs[0], outs[1])
    # nothing outside the view was touched
    assert (outs[1][:, :8] == 7.0).all() and (outs[1][:, 8 + N :] == 7.0).all()


@pytest.mark.parametrize("I", [16, 48, 272])
@pytest.mark.parametrize("M", [1, 6, 16])
def test_swiglu_epilogue_bit_identical(M, I):
    K = 512
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = torch.randn(2 * I, K, generator=g) / math.sqrt(K)
    w[:I] *= 10.0  # gate pre-activations ~N(0, 10)
    # and two planted gate rows that put row 0 at about +30 and -30, so
    # both tails of the exponential are exercised at every (M, I)
    x0 = x[0].float().cpu()
    w[0] = x0 * (30.0 / x0.square().sum())
    w[1] = -w[0]
    w = w.to(torch.bfloat16).to(DEV)

    gu = torch.empty(M, 2 * I, dtype=torch.bfloat16, device=DEV)
    ext.gemm_skinny_bf16(gu, x, w, tiles_per_wg=1)
    assert gu[0, 0].item() > 25.0 and gu[0, 1].item() < -25.0
    ref = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
    ext.silu_mul(ref, gu)

    got = torch.full((M, I), float("nan"), dtype=torch.bfloat16, device=DEV)
    ext.gemm_skinny_swiglu_bf16(got, x, w)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("M,I", [(8, 48), (16, 48), (6, 48), (8, 40)])
def test_linear_swiglu_dispatch_bit_identical(M, I):
    # fused at M >= 8 with I % 16 == 0; two kernels below M=8 and at I=40
    from dts_amd import ops

    x, w = _inputs(M, 512, 2 * I, seed=6)
    assert torch.equal(ops.linear_swiglu(x, w), ops.silu_mul(ops.linear_bf16(x, w)))


@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("M,K,N", [(7, 1024, 48), (8, 14336, 64), (16, 2048, 100)])
def test_unroll_bit_identical(M, K, N, nt):
    # 8 k-chunks in flight (auto for deep K) vs 4: same chunk order
    x, w = _inputs(M, K, N, seed=8)
    out4 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    out8 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ext.gemm_skinny_bf16(out4, x, w, tiles_per_wg=nt, unroll=4)
    ext.gemm_skinny_bf16(out8, x, w, tiles_per_wg=nt, unroll=8)
    assert torch.equal(out8, out4)
    assert torch.equal(_run(x, w, 0), out4)  # auto NT and auto unroll
