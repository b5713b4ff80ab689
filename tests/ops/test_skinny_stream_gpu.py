"""Bit-identity of the stream skinny GEMM (unroll=16|32: a ring of load
groups in flight per wave, x and W through range-checked buffer loads)
against the EXISTING gemm_skinny_kernel pinned with tiles_per_wg=1, unroll=4.

The stream kernel keeps the per-wave chunk order, the single accumulator per
tile and the 4-way cross-wave sum, so every check is torch.equal. Shapes are
the smallest at which the ring can go wrong (a group is 8 chunks, the ring 2
groups at unroll=16 and 4 at 32): K=1024 (one group per wave: fewer than the
ring is deep), 2048 (two: exactly the ring at 16, short of it at 32), 4096
(four: the ring at 32, two steady rounds at 16), 14336 (14 groups: steady
rounds, then a tail that still refills at 32). N=16 (one tile), 40 (ragged:
half the last tile's lanes have no row), 48; 64 adds an even tile count for
two tiles per workgroup. The weight ends exactly at the end of its tensor,
behind a NaN pad; x is a column slice of a wider NaN tensor with NaN rows
past M, so a read of a row >= M, of a wrong column or in front of W shows;
outputs are slices of NaN-poisoned tensors.
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
MS = (1, 5, 8, 16)
NAN = float("nan")


def _inputs(M, K, N, seed):
    """x: [M, K] view with row stride 2K + 64 inside a [16, 2K + 64] NaN
    tensor; w: [N, K] at the very end of a NaN-padded flat tensor."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    big = torch.full((16, 2 * K + 64), NAN, dtype=torch.bfloat16, device=DEV)
    big[:M, 64 : 64 + K] = xs
    x = big[:M, 64 : 64 + K]
    assert x.stride(0) == 2 * K + 64 or M == 1
    ws = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    flat = torch.full((1024 + N * K,), NAN, dtype=torch.bfloat16, device=DEV)
    flat[1024:] = ws.to(DEV).view(-1)
    w = flat[1024:].view(N, K)
    assert w.is_contiguous()
    return xs, x, w


def _ref(xs, w):
    """The existing kernel on a dense copy of x."""
    out = torch.full((xs.shape[0], w.shape[0]), NAN, dtype=torch.bfloat16, device=DEV)
    ext.gemm_skinny_bf16(out, xs, w, tiles_per_wg=1, unroll=4)
    assert torch.isfinite(out.float()).all()
    return out


def _stream(x, w, unroll, nt=1):
    """The stream kernel into a column slice of a wider NaN tensor; checks
    that nothing outside the slice was written."""
    M, N = x.shape[0], w.shape[0]
    wide = torch.full((M, 2 * N + 8), NAN, dtype=torch.bfloat16, device=DEV)
    out = wide[:, 8 : 8 + N]
    ext.gemm_skinny_bf16(out, x, w, tiles_per_wg=nt, unroll=unroll)
    assert torch.isnan(wide[:, :8].float()).all()
    assert torch.isnan(wide[:, 8 + N :].float()).all()
    return out


@pytest.mark.parametrize("unroll", [16, 32])
@pytest.mark.parametrize("N", [16, 40, 48])
@pytest.mark.parametrize("K", [1024, 2048, 4096])
def test_bit_identical(K, N, unroll):
    for M in MS:
        xs, x, w = _inputs(M, K, N, seed=K + N + M)
        assert torch.equal(_stream(x, w, unroll), _ref(xs, w)), M


@pytest.mark.parametrize("unroll", [16, 32])
def test_bit_identical_deep_k(unroll):
    for M in MS:
        xs, x, w = _inputs(M, 14336, 48, seed=M)
        assert torch.equal(_stream(x, w, unroll), _ref(xs, w)), M


@pytest.mark.parametrize("N", [40, 48, 64])  # 3, 3 and 4 tiles
@pytest.mark.parametrize("K", [1024, 4096, 14336])
def test_two_tiles_per_workgroup(K, N):
    for M in MS:
        xs, x, w = _inputs(M, K, N, seed=K + N + M + 1)
        assert torch.equal(_stream(x, w, 16, nt=2), _ref(xs, w)), M


def test_dense_operands_and_auto_tiles():
    # plain contiguous x and out, tiles_per_wg left to the dispatcher: at
    # M=8 and 384 tiles it takes two tiles per workgroup at unroll=16
    M, K, N = 8, 1024, 6144
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    ref = _ref(x, w)
    for unroll in (16, 32):
        out = torch.full((M, N), NAN, dtype=torch.bfloat16, device=DEV)
        ext.gemm_skinny_bf16(out, x, w, unroll=unroll)
        assert torch.equal(out, ref), unroll


@pytest.mark.parametrize("unroll", [16, 32])
def test_same_call_twice_same_bits(unroll):
    xs, x, w = _inputs(8, 2048, 40, seed=7)
    a = _stream(x, w, unroll)
    b = _stream(x, w, unroll)
    assert torch.equal(a, b)
    assert torch.equal(a, _ref(xs, w))


def test_graph_replay_equals_eager():
    # three calls (both ring depths and the two-tile variant) in one graph
    xs, x, w = _inputs(8, 2048, 40, seed=9)
    outs = [torch.full((8, 40), NAN, dtype=torch.bfloat16, device=DEV) for _ in range(3)]
    pins = [dict(unroll=16), dict(unroll=32), dict(unroll=16, tiles_per_wg=2)]

    def calls():
        for out, pin in zip(outs, pins):
            ext.gemm_skinny_bf16(out, x, w, **pin)

    calls()
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    ref = _ref(xs, w)
    for e in eager:
        assert torch.equal(e, ref)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    for _ in range(2):
        for o in outs:
            o.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)


def test_rejections():
    _, _, w = _inputs(8, 1024, 32, seed=1)
    x = torch.randn(8, 1024, device=DEV).to(torch.bfloat16)
    out = torch.full((8, 32), NAN, dtype=torch.bfloat16, device=DEV)
    # a K that is no whole number of 8-chunk groups per wave
    xk = torch.randn(8, 1536, device=DEV).to(torch.bfloat16)
    wk = torch.randn(32, 1536, device=DEV).to(torch.bfloat16)
    for unroll in (16, 32):
        with pytest.raises(RuntimeError, match=f"unroll={unroll} needs K % 1024"):
            ext.gemm_skinny_bf16(out, xk, wk, unroll=unroll)
    with pytest.raises(RuntimeError, match="unroll must be"):
        ext.gemm_skinny_bf16(out, x, w, unroll=3)
    with pytest.raises(RuntimeError, match="unroll=32 has no tiles_per_wg=2"):
        ext.gemm_skinny_bf16(out, x, w, tiles_per_wg=2, unroll=32)
    with pytest.raises(RuntimeError, match="unroll=16 has no tiles_per_wg=4"):
        ext.gemm_skinny_bf16(out, x, w, tiles_per_wg=4, unroll=16)
    with pytest.raises(RuntimeError, match="weight must be bfloat16"):
        ext.gemm_skinny_bf16(out, x, w.half(), unroll=16)
    assert torch.isnan(out.float()).all()  # no rejected call launched
    # a weight over 2 GiB cannot be addressed by 32-bit buffer offsets
    n_big = (1 << 20) + 16
    w_big = torch.empty(n_big, 1024, dtype=torch.bfloat16, device=DEV)
    out_big = torch.empty(1, n_big, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="at most 2 GiB"):
        ext.gemm_skinny_bf16(out_big, x[:1], w_big, unroll=16)
