"""Bit-identity of the persistent skinny GEMM (one workgroup per CU, the
activation staged in LDS) against gemm_skinny_kernel at one tile per
workgroup, and of its SwiGLU form against gemm_skinny_swiglu_bf16.

A team of the persistent workgroup is the existing workgroup unchanged
(same per-wave k-chunk order, same 4-way cross-wave sum, one rounding), so
every check is torch.equal. Shapes are the smallest at which the new parts
can go wrong: K=512 (one chunk group per wave, nothing to pipeline), 1024
(two groups: both weight buffers), 4096 (the largest image); N=16 (one
tile, every other team and workgroup dead), 40 (ragged last tile), 48
(fewer tiles than teams), and one tile more than a full pass of all teams
of all workgroups, so the loop wraps and teams differ in live trips.
Outputs are NaN-poisoned so an element the kernel fails to write shows.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dts_amd.ops import _hip_ext_loader

    ext = _hip_ext_loader.load()
    CUS = torch.cuda.get_device_properties(0).multi_processor_count
else:  # collected but skipped off-GPU
    ext = None
    CUS = 256

DEV = "cuda:0"
TEAMS = 4  # teams per persistent workgroup


def _inputs(M, K, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(DEV)
    return x, w


def _poison(M, N):
    return torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)


def _ref(x, w):
    out = _poison(x.shape[0], w.shape[0])
    ext.gemm_skinny_bf16(out, x, w, tiles_per_wg=1)
    return out


def _pers(x, w, out=None):
    if out is None:
        out = _poison(x.shape[0], w.shape[0])
    ext.gemm_skinny_bf16(out, x, w, persistent=1)
    return out


def _swiglu(x, w, persistent):
    out = _poison(x.shape[0], w.shape[0] // 2)
    ext.gemm_skinny_swiglu_bf16(out, x, w, persistent=persistent)
    return out


@pytest.mark.parametrize("M", [1, 7, 8, 9, 16])
@pytest.mark.parametrize("N", [16, 40, 48])
@pytest.mark.parametrize("K", [512, 1024, 4096])
def test_plain_bit_identical(K, N, M):
    x, w = _inputs(M, K, N, seed=K + N + M)
    ref = _ref(x, w)
    got = _pers(x, w)
    assert not torch.isnan(ref.float()).any()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("M", [1, 7, 8, 9, 16])
def test_plain_loop_wraps(M):
    # one tile more than one pass of all teams: workgroup 0's team 0 runs a
    # second live trip, every other team a dead one
    N = 16 * (TEAMS * CUS) + 16
    x, w = _inputs(M, 512, N, seed=M)
    assert torch.equal(_pers(x, w), _ref(x, w))


# the two large I (one pair more than one per workgroup; one pair more than
# a full pass of all teams, so the loop wraps) are K=512 cases, like the
# plain wrap case
SWIGLU_KI = [(K, I) for K in (512, 1024, 4096) for I in (16, 48)] + [
    (512, 16 * CUS + 16),
    (512, 16 * (TEAMS * CUS) + 16),
]


@pytest.mark.parametrize("M", [1, 7, 8, 9, 16])
@pytest.mark.parametrize("K,I", SWIGLU_KI)
def test_swiglu_bit_identical(K, I, M):
    x, w = _inputs(M, K, 2 * I, seed=K + I + M)
    ref = _swiglu(x, w, 0)
    got = _swiglu(x, w, 1)
    assert not torch.isnan(ref.float()).any()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("M", [1, 8, 15])
def test_strided_operands(M):
    K, N = 1024, 40
    g = torch.Generator().manual_seed(3)
    # x is every second row of a larger tensor whose other rows, and the
    # rows just past M, are NaN: a read of a row >= M or of a wrong row
    # poisons the output
    big = torch.full((2 * M + 4, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    xs = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    big[0 : 2 * M : 2] = xs
    x = big[0 : 2 * M : 2]
    assert x.stride(0) == 2 * K
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(DEV)
    ref = _ref(xs, w)
    wide = _poison(M, 2 * N + 8)
    out = wide[:, 8 : 8 + N]
    _pers(x, w, out)
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, ref)
    # nothing outside the view was written
    assert torch.isnan(wide[:, :8].float()).all()
    assert torch.isnan(wide[:, 8 + N :].float()).all()


def test_back_to_back_inputs():
    # a stale LDS image or reduction buffer would leak the first input's
    # values into the second call
    K, N, M = 1024, 48, 8
    x1, w = _inputs(M, K, N, seed=1)
    x2, _ = _inputs(M, K, N, seed=2)
    a1 = _pers(x1, w)
    a2 = _pers(x2, w)
    a1_again = _pers(x1, w)
    assert torch.equal(a1, _ref(x1, w))
    assert torch.equal(a2, _ref(x2, w))
    assert torch.equal(a1, a1_again)
    assert not torch.equal(a1, a2)


def test_pinned_on_off_and_auto_agree():
    # the Llama-3-8B gate_up (1792 tiles, 896 pairs) at M=8: a shape the
    # measured rule selects, so the unpinned call runs the new kernel too
    M, K, N = 8, 4096, 28672
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    plain, fused = [], []
    for p in (0, 1, -1):
        out = _poison(M, N)
        ext.gemm_skinny_bf16(out, x, w, persistent=p)
        plain.append(out)
        fused.append(_swiglu(x, w, p))
    assert torch.equal(plain[0], _ref(x, w))
    for outs in (plain, fused):
        assert bool(torch.isfinite(outs[0].float()).all())
        assert torch.equal(outs[0], outs[1])
        assert torch.equal(outs[0], outs[2])


def test_rejections():
    x, w = _inputs(8, 512, 32)
    out = _poison(8, 32)
    # a K whose image does not fit, pinned on
    xk, wk = _inputs(8, 4608, 32)
    with pytest.raises(RuntimeError, match="persistent=1 needs K"):
        ext.gemm_skinny_bf16(out, xk, wk, persistent=1)
    with pytest.raises(RuntimeError, match="persistent=1 needs K"):
        ext.gemm_skinny_swiglu_bf16(_poison(8, 16), xk, wk, persistent=1)
    # the same K unpinned keeps the existing kernel
    ext.gemm_skinny_bf16(out, xk, wk)
    assert torch.equal(out, _ref(xk, wk))
    with pytest.raises(RuntimeError, match="persistent must be"):
        ext.gemm_skinny_bf16(out, x, w, persistent=2)
    with pytest.raises(RuntimeError, match="no tiles_per_wg or unroll"):
        ext.gemm_skinny_bf16(out, x, w, tiles_per_wg=2, persistent=1)
    # wrong dtypes
    with pytest.raises(RuntimeError):
        ext.gemm_skinny_bf16(out, x.float(), w, persistent=1)
    with pytest.raises(RuntimeError, match="weight must be bfloat16"):
        ext.gemm_skinny_bf16(out, x, w.half(), persistent=1)
    with pytest.raises(RuntimeError):
        ext.gemm_skinny_bf16(_poison(9, 32), x, w, persistent=1)
