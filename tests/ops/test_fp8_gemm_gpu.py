"""W8A16 skinny GEMM (FP8 e4m3fn weights, bf16 activations) on the GPU.

Two exact cases pin the kernel's mechanics — one-hot activations over every
finite e4m3 code and every k position (dequantisation, A/B fragment
agreement), integer data (split-K, reduction, scale indexing, ragged
tiles) — and random data is held to TestGemmSkinny's tolerances against
torch_ref.linear_w8a16. Shapes are the smallest at which the kernel can go
wrong: K = 512 (one k-group per wave) and 2048, N = 16 / 40 (ragged last
tile) / 112 (7 tiles: NT = 2 and 4 leave dead tiles), K = 1024 at
unroll=8. Every case loops M in {1, 3, 8, 16} and tiles_per_wg in {1, 2, 4}.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd import ops
from dts_amd.models.quant import quantize_fp8_rowwise
from dts_amd.ops import _hip_ext_loader, torch_ref

ext = _hip_ext_loader.load()

DEV = "cuda:0"
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
MS = (1, 3, 8, 16)
NTS = (1, 2, 4)
SENTINEL = 12345.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _scales(n, seed):
    """Arbitrary positive fp32 scales (not powers of two)."""
    return torch.rand(n, generator=_gen(seed)) * 3.0 + 0.01


def _run(x, w_q, scale, nt=0, unroll=0):
    """Launch into a sentinel-filled buffer one tile wider than N and check
    nothing outside [M, N] was written."""
    M, N = x.shape[0], w_q.shape[0]
    buf = torch.full((M + 1, N + 16), SENTINEL, dtype=BF16, device=DEV)
    out = buf[:M, :N]
    ext.gemm_skinny_w8_bf16(out, x, w_q, scale, tiles_per_wg=nt, unroll=unroll)
    assert torch.all(buf[:, N:] == SENTINEL) and torch.all(buf[M:] == SENTINEL)
    return out


# ---------------------------------------------------------------------------
# every code, every k position — exact
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def all_codes():
    N, K = 48, 512
    codes = torch.tensor(
        [c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8
    )
    assert codes.numel() == 254
    n = torch.arange(N)[:, None]
    k = torch.arange(K)[None, :]
    w_q = codes[(7 * n + k) % 254].view(FP8).contiguous()
    assert not torch.any(torch.isnan(w_q.float()))
    scale = _scales(N, 11)
    # out[k, n] for the one-hot row selecting k: one product with 1.0, one
    # fp32 multiply, one round-to-nearest-even — on both sides
    expected = (w_q.float().T * scale).to(BF16)  # [K, N]
    return w_q.to(DEV), scale.to(DEV), expected


@pytest.mark.parametrize("M", MS)
def test_every_code_every_k_exact(all_codes, M):
    w_q, scale, expected = all_codes
    K, N = w_q.shape[1], w_q.shape[0]
    eye = torch.eye(K, dtype=BF16, device=DEV)
    for nt in NTS:
        out_all = torch.full((K, N), SENTINEL, dtype=BF16, device=DEV)
        for s in range(0, K, M):  # one-hot rows, M per launch, every k hit
            ext.gemm_skinny_w8_bf16(
                out_all[s : s + M], eye[s : s + M], w_q, scale, tiles_per_wg=nt
            )
        got = out_all.cpu()
        # torch.equal semantics (value equality: the sum of +0 and the -0
        # code is +0), with the first mismatch named on failure
        bad = (got != expected).nonzero()
        assert torch.equal(got, expected), (
            f"nt={nt}: {bad.shape[0]} mismatches, first (k, n)={bad[0].tolist()} "
            f"got {got[tuple(bad[0])].item()} want {expected[tuple(bad[0])].item()}"
        )


# ---------------------------------------------------------------------------
# integer data — exact
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def integer_case():
    K, N = 2048, 40
    w = torch.randint(-16, 17, (N, K), generator=_gen(21)).float()
    w_q = w.to(FP8)
    assert torch.equal(w_q.float(), w)  # integers up to 16 are e4m3 values
    x = torch.randint(-4, 5, (16, K), generator=_gen(22)).to(BF16)
    scale = _scales(N, 23)
    # |sum| <= 16*4*2048 < 2^24: the fp32 sum is exact in any order
    ref = torch_ref.linear_w8a16(x, w_q, scale)
    return x.to(DEV), w_q.to(DEV), scale.to(DEV), ref


@pytest.mark.parametrize("unroll", [4, 8])
@pytest.mark.parametrize("M", MS)
def test_integer_data_exact(integer_case, M, unroll):
    x, w_q, scale, ref = integer_case
    for nt in NTS:
        out = _run(x[:M], w_q, scale, nt, unroll)
        assert torch.equal(out.cpu(), ref[:M]), f"nt={nt}"


# ---------------------------------------------------------------------------
# random data
# ---------------------------------------------------------------------------

_random_cache = {}


def _random_case(K, N):
    if (K, N) not in _random_cache:
        w = torch.randn(N, K, generator=_gen(K + N)) / math.sqrt(K)
        w_q, _ = quantize_fp8_rowwise(w * 100.0)  # codes spread over the range
        scale = _scales(N, K + N + 1) / 100.0
        x = torch.randn(16, K, generator=_gen(K + N + 2)).to(BF16)
        ref = torch_ref.linear_w8a16(x, w_q, scale).float()
        _random_cache[(K, N)] = (x.to(DEV), w_q.to(DEV), scale.to(DEV), ref)
    return _random_cache[(K, N)]


@pytest.mark.parametrize(
    "K,N,unroll",
    [(K, N, 0) for K in (512, 2048) for N in (16, 40, 112)] + [(1024, 40, 8)],
)
@pytest.mark.parametrize("M", MS)
def test_random_matches_reference(M, K, N, unroll):
    x, w_q, scale, ref = _random_case(K, N)
    for nt in NTS:
        out = _run(x[:M], w_q, scale, nt, unroll)
        torch.testing.assert_close(
            out.cpu().float(), ref[:M], atol=3e-2, rtol=3e-2, msg=lambda m: f"nt={nt}: {m}"
        )
    # auto dispatch
    out = _run(x[:M], w_q, scale)
    torch.testing.assert_close(out.cpu().float(), ref[:M], atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("M", MS)
def test_strided_x_and_out(M):
    """Row stride larger than the row, for x (fused qkv views) and out."""
    K, N = 2048, 112
    x, w_q, scale, ref = _random_case(K, N)
    big = torch.full((M, 2 * K), float("nan"), dtype=BF16, device=DEV)
    big[:, K:] = x[:M]
    xs = big[:, K:]
    assert xs.stride(0) == 2 * K
    for nt in NTS:
        out_big = torch.full((M, 3 * N), SENTINEL, dtype=BF16, device=DEV)
        out = out_big[:, N : 2 * N]
        ext.gemm_skinny_w8_bf16(out, xs, w_q, scale, tiles_per_wg=nt)
        torch.testing.assert_close(out.cpu().float(), ref[:M], atol=3e-2, rtol=3e-2)
        assert torch.all(out_big[:, :N] == SENTINEL)
        assert torch.all(out_big[:, 2 * N :] == SENTINEL)


def test_nt_and_unroll_are_bit_identical():
    """Same per-wave chunk order and reduction for every NT and unroll."""
    x, w_q, scale, _ = _random_case(2048, 112)
    base = _run(x, w_q, scale, 1, 4)
    for nt in NTS:
        for unroll in (4, 8):
            assert torch.equal(_run(x, w_q, scale, nt, unroll), base)


# ---------------------------------------------------------------------------
# fused SwiGLU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("data", ["random", "integer"])
@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("I", [16, 48])
def test_fused_swiglu_equals_gemm_then_silu_mul(I, K, data):
    N = 2 * I
    if data == "integer":
        # small integers so silu_mul sees distinct, exactly-known operands
        # and a swapped gate/up scale changes the result
        w_q = torch.randint(-16, 17, (N, K), generator=_gen(I + K)).float().to(FP8)
        x16 = torch.randint(-4, 5, (16, K), generator=_gen(I + K + 1)).to(BF16)
        scale = _scales(N, I + K + 2) / 256.0
    else:
        w = torch.randn(N, K, generator=_gen(I + K + 3)) / math.sqrt(K)
        w_q, scale = quantize_fp8_rowwise(w)
        x16 = torch.randn(16, K, generator=_gen(I + K + 4)).to(BF16)
    w_q, scale, x16 = w_q.to(DEV), scale.to(DEV), x16.to(DEV)
    unroll = 8 if K % 1024 == 0 and K >= 8192 else 4  # the fused kernel's auto
    for M in MS:
        x = x16[:M]
        buf = torch.full((M + 1, I + 16), SENTINEL, dtype=BF16, device=DEV)
        out = buf[:M, :I]
        ext.gemm_skinny_swiglu_w8_bf16(out, x, w_q, scale)
        assert torch.all(buf[:, I:] == SENTINEL) and torch.all(buf[M:] == SENTINEL)
        for nt in NTS:
            two = ops.silu_mul(_run(x, w_q, scale, nt, unroll).contiguous())
            assert torch.equal(out, two), f"M={M} nt={nt}"
        if data == "integer":
            # and the pair is the right one: exact operands on the host
            gu = torch_ref.linear_w8a16(x.cpu(), w_q.cpu(), scale.cpu())
            ref = torch_ref.silu_mul(gu).float()
            torch.testing.assert_close(out.cpu().float(), ref, atol=3e-2, rtol=3e-2)


def test_ops_dispatch_runs_the_fp8_kernel():
    """ops.linear_w8a16 at M <= 16 streams w_q (a w_deq of NaNs proves the
    dequantised copy is not what was read); above 16 it is linear_bf16 on
    w_deq."""
    x, w_q, scale, ref = _random_case(2048, 112)
    poison = torch.full(w_q.shape, float("nan"), dtype=BF16, device=DEV)
    out = ops.linear_w8a16(x[:4], w_q, scale, poison)
    torch.testing.assert_close(out.cpu().float(), ref[:4], atol=3e-2, rtol=3e-2)
    w_deq = (w_q.float() * scale[:, None]).to(BF16)
    x32 = torch.cat([x, x])
    assert torch.equal(
        ops.linear_w8a16(x32, w_q, scale, w_deq), ops.linear_bf16(x32, w_deq)
    )
    act = ops.linear_swiglu_w8a16(x[:8], w_q[:96], scale[:96], poison[:96])
    two = ops.silu_mul(ops.linear_w8a16(x[:8], w_q[:96], scale[:96], poison[:96]))
    assert torch.equal(act, two)


# ---------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------

class TestHostChecks:
    def _args(self, M=4, K=512, N=32):
        x = torch.zeros(M, K, dtype=BF16, device=DEV)
        w_q = torch.zeros(N, K, dtype=torch.uint8, device=DEV).view(FP8)
        scale = torch.ones(N, device=DEV)
        out = torch.empty(M, N, dtype=BF16, device=DEV)
        return out, x, w_q, scale

    def test_valid_call_passes(self):
        ext.gemm_skinny_w8_bf16(*self._args())

    def test_m_17_raises(self):
        with pytest.raises(RuntimeError):
            ext.gemm_skinny_w8_bf16(*self._args(M=17))

    def test_k_256_raises(self):
        with pytest.raises(RuntimeError):
            ext.gemm_skinny_w8_bf16(*self._args(K=256))

    def test_non_contiguous_w_q_raises(self):
        out, x, w_q, scale = self._args()
        wide = torch.zeros(32, 1024, dtype=torch.uint8, device=DEV).view(FP8)
        with pytest.raises(RuntimeError):
            ext.gemm_skinny_w8_bf16(out, x, wide[:, :512], scale)

    def test_wrong_scale_length_raises(self):
        out, x, w_q, scale = self._args()
        with pytest.raises(RuntimeError):
            ext.gemm_skinny_w8_bf16(out, x, w_q, scale[:31])
        with pytest.raises(RuntimeError):
            ext.gemm_skinny_swiglu_w8_bf16(
                torch.empty(4, 16, dtype=BF16, device=DEV), x, w_q, scale[:16]
            )

    def test_bf16_weight_raises(self):
        out, x, w_q, scale = self._args()
        with pytest.raises(RuntimeError):
            ext.gemm_skinny_w8_bf16(out, x, w_q.to(BF16), scale)

    def test_unroll_8_needs_k_1024(self):
        with pytest.raises(RuntimeError):
            ext.gemm_skinny_w8_bf16(*self._args(), unroll=8)
