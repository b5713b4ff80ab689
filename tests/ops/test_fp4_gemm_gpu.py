"""W4A16 skinny GEMM (MXFP4 weights) on the GPU, mirroring test_fp8_gemm_gpu.py:
exact one-hot and integer cases, random data at TestGemmSkinny's tolerances,
every launch into a sentinel-filled buffer one tile wider than N."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from dts_amd import ops
from dts_amd.models.quant import dequantize_mxfp4, quantize_mxfp4_rowwise
from dts_amd.ops import _hip_ext_loader, torch_ref

ext = _hip_ext_loader.load()
DEV, BF16, U8 = "cuda:0", torch.bfloat16, torch.uint8
MS, NTS, SENTINEL = (1, 3, 8, 16), (1, 2, 4), 12345.0
TOL = dict(atol=3e-2, rtol=3e-2)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unrolls(K):
    return [u for u in (4, 8, 16) if K % (128 * u) == 0]


def _pack(code):  # [N, K] codes -> [N, K/2], element 2i in the low nibble
    c = code.to(U8).view(code.shape[0], -1, 2)
    return (c[:, :, 0] | (c[:, :, 1] << 4)).contiguous()


def _run(fn, x, w_q, scale, n_out, **kw):
    M = x.shape[0]
    buf = torch.full((M + 1, n_out + 16), SENTINEL, dtype=BF16, device=DEV)
    fn(buf[:M, :n_out], x, w_q, scale, **kw)
    assert torch.all(buf[:, n_out:] == SENTINEL) and torch.all(buf[M:] == SENTINEL)
    return buf[:M, :n_out]


def _gemm(x, w_q, scale, nt=0, unroll=0):
    return _run(ext.gemm_skinny_w4_bf16, x, w_q, scale, w_q.shape[0],
                tiles_per_wg=nt, unroll=unroll)


@pytest.fixture(scope="module")
def all_codes():
    # consecutive blocks step 3 through 11 exponents: a quad's four all differ
    N, K = 48, 512
    n, k, blk = torch.arange(N)[:, None], torch.arange(K)[None], torch.arange(K // 32)[None]
    exps = torch.tensor([-125] + list(range(-20, 21, 5)) + [125])
    w_q = _pack((7 * n + k) % 16)
    scale = (exps[(5 * n + 3 * blk) % len(exps)] + 127).to(U8).contiguous()
    return w_q.to(DEV), scale.to(DEV), dequantize_mxfp4(w_q, scale, BF16).T.contiguous()


@pytest.mark.parametrize("M", MS)
def test_every_code_every_k_exact(all_codes, M):
    w_q, scale, expected = all_codes
    K, N = expected.shape
    eye = torch.eye(K, dtype=BF16, device=DEV)
    for nt in NTS:
        out = torch.full((K, N), SENTINEL, dtype=BF16, device=DEV)
        for s in range(0, K, M):  # one-hot rows, M per launch, every k hit
            ext.gemm_skinny_w4_bf16(out[s : s + M], eye[s : s + M], w_q, scale, tiles_per_wg=nt)
        bad = (out.cpu() != expected).nonzero()
        assert torch.equal(out.cpu(), expected), f"nt={nt}: first (k, n) {bad[:1].tolist()}"


@pytest.fixture(scope="module")
def integer_case():
    K, N = 2048, 40
    codes = torch.tensor([0, 2, 4, 5, 6, 7, 10, 12, 13, 14, 15])  # the integer values
    w_q = _pack(codes[torch.randint(0, len(codes), (N, K), generator=_gen(21))])
    scale = (torch.randint(0, 3, (N, K // 32), generator=_gen(23)) + 127).to(U8)
    x = torch.randint(-4, 5, (16, K), generator=_gen(22)).to(BF16)
    # |sum| <= 6*4*4*2048 < 2^24: the fp32 sum is exact in any order
    return x.to(DEV), w_q.to(DEV), scale.to(DEV), torch_ref.linear_w4a16(x, w_q, scale)


@pytest.mark.parametrize("unroll", _unrolls(2048))
@pytest.mark.parametrize("M", MS)
def test_integer_data_exact(integer_case, M, unroll):
    x, w_q, scale, ref = integer_case
    for nt in NTS:
        assert torch.equal(_gemm(x[:M], w_q, scale, nt, unroll).cpu(), ref[:M]), f"nt={nt}"


@pytest.fixture(scope="module")
def random_case():
    cache = {}

    def get(K, N):
        if (K, N) not in cache:
            w_q, scale = quantize_mxfp4_rowwise(torch.randn(N, K, generator=_gen(K + N)) / K**0.5)
            x = torch.randn(16, K, generator=_gen(K + N + 2)).to(BF16)
            ref = torch_ref.linear_w4a16(x, w_q, scale).float()
            cache[(K, N)] = (x.to(DEV), w_q.to(DEV), scale.to(DEV), ref)
        return cache[(K, N)]

    return get


@pytest.mark.parametrize("K,N", [(512, 16), (1536, 40), (2048, 112)])
@pytest.mark.parametrize("M", MS)
def test_random_matches_reference(random_case, M, K, N):
    x, w_q, scale, ref = random_case(K, N)
    for nt in (0,) + NTS:
        for unroll in [0] + _unrolls(K):  # K = 1536: auto falls back to 4
            out = _gemm(x[:M], w_q, scale, nt, unroll)
            torch.testing.assert_close(out.cpu().float(), ref[:M], **TOL)


def test_nt_and_unroll_are_bit_identical(random_case):
    x, w_q, scale, _ = random_case(2048, 112)
    base = _gemm(x, w_q, scale, 1, 4)
    for nt in NTS:
        for unroll in _unrolls(2048):
            assert torch.equal(_gemm(x, w_q, scale, nt, unroll), base)


@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("I", [16, 56])
def test_fused_swiglu_equals_gemm_then_silu_mul(I, K):
    w_q, scale = (t.to(DEV) for t in quantize_mxfp4_rowwise(
        torch.randn(2 * I, K, generator=_gen(I + K)) / K**0.5))
    x = torch.randn(16, K, generator=_gen(I + K + 1)).to(BF16).to(DEV)
    poison = torch.full((2 * I, K), float("nan"), dtype=BF16, device=DEV)
    for M in MS:
        out = _run(ext.gemm_skinny_swiglu_w4_bf16, x[:M], w_q, scale, I)
        assert torch.equal(out, ops.silu_mul(_gemm(x[:M], w_q, scale).contiguous())), f"M={M}"
        # ops reads the MXFP4 copy at M <= 16, never w_deq
        assert torch.equal(out, ops.linear_swiglu_w4a16(x[:M], w_q, scale, poison))
    # and the pair is the right one (gate rows n, up rows I + n)
    ref = torch_ref.silu_mul(torch_ref.linear_w4a16(x.cpu(), w_q.cpu(), scale.cpu()))
    torch.testing.assert_close(out.cpu().float(), ref.float(), **TOL)


def _args(M=4, K=1024, N=32):
    return dict(
        out=torch.empty(M, N, dtype=BF16, device=DEV),
        x=torch.zeros(M, K, dtype=BF16, device=DEV),
        w_q=torch.zeros(N, K // 2, dtype=U8, device=DEV),
        scale=torch.full((N, K // 32), 127, dtype=U8, device=DEV),
    )


BAD_CALLS = {  # one per binding check: what to change in a valid call
    "cpu_operand": lambda a: dict(scale=a["scale"].cpu()),
    "x_not_bf16": lambda a: dict(x=a["x"].half()),
    "w_q_not_uint8": lambda a: dict(w_q=a["w_q"].view(torch.int8)),
    "w_q_not_contiguous": lambda a: dict(w_q=torch.zeros(32, 1024, dtype=U8, device=DEV)[:, :512]),
    "w_q_wrong_width": lambda a: dict(w_q=torch.zeros(32, 1024, dtype=U8, device=DEV)),
    "scale_not_uint8": lambda a: dict(scale=a["scale"].float()),
    "scale_wrong_width": lambda a: dict(scale=a["scale"][:, :16].contiguous()),
    "scale_wrong_rows": lambda a: dict(scale=a["scale"][:31]),
    "x_rows_misaligned": lambda a: dict(x=torch.zeros(4, 1028, dtype=BF16, device=DEV)[:, :1024]),
    "m_17": lambda a: _args(M=17),
    "k_256": lambda a: _args(K=256),
    "out_wrong_width": lambda a: dict(out=a["out"][:, :16]),
    "out_wrong_rows": lambda a: dict(out=a["out"][:3]),
    "tiles_per_wg_3": lambda a: dict(tiles_per_wg=3),
    "unroll_12": lambda a: dict(unroll=12),
    "unroll_16_on_k_1024": lambda a: dict(unroll=16),
    "unroll_8_on_k_512": lambda a: dict(_args(K=512), unroll=8),
}


@pytest.mark.parametrize("name", BAD_CALLS)
def test_rejected_calls(name):
    args = _args()
    ext.gemm_skinny_w4_bf16(**args)  # the base call is valid
    args.update(BAD_CALLS[name](args))
    with pytest.raises(RuntimeError):
        ext.gemm_skinny_w4_bf16(**args)
    if name in ("scale_wrong_rows", "w_q_not_uint8", "k_256", "x_rows_misaligned"):
        out = torch.empty(args["x"].shape[0], 16, dtype=BF16, device=DEV)
        with pytest.raises(RuntimeError):
            ext.gemm_skinny_swiglu_w4_bf16(out, args["x"], args["w_q"], args["scale"])
