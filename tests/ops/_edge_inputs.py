"""Input builders and fp64 references for the edge-case kernel tests.

Every builder is deterministic (seeded CPU generators) and returns CPU
tensors. The GPU files (test_*_edges_gpu.py, test_gemm_exact_gpu.py,
test_prefill_causal_exact_gpu.py) move them to the device;
test_edge_inputs_cpu.py runs every builder through torch_ref or fp64 and
asserts the properties the GPU assertions rely on, so each construction is
proven on the reference alone.
"""

import functools
import math

import torch

from dts_amd.ops import torch_ref

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
BS = 16
EPS = 1e-5
SENTINEL = -12352.0  # a bf16 value no builder produces


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------
# bf16 ulp measure
# ---------------------------------------------------------------------------

def bf16_ulp(r):
    """ulp(r) = 2^(floor(log2|r|) - 7) of an fp64 reference value; below the
    smallest normal bf16 (2^-126) the spacing of the format stays 2^-133."""
    a = r.abs().double().clamp_min(2.0**-126)
    _, e = torch.frexp(a)  # a = m * 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    return torch.ldexp(torch.ones_like(a), e - 8)


def ulp_err(got, ref64, slack=None):
    """max over elements of (|got - ref| - slack) / ulp(ref)."""
    d = (got.double() - ref64).abs()
    if slack is not None:
        d = d - slack
    return float((d / bf16_ulp(ref64)).max())


# ---------------------------------------------------------------------------
# Norms
# ---------------------------------------------------------------------------

NORM_SHAPES = [(4100, 2056), (2049, 8), (3, 8192), (1, 768)]
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # what the kernel gets
LN_OFFSET_SHAPE = (67, 2056)
LN_OFFSET_MEAN = 100.0


@functools.lru_cache(maxsize=None)
def norm_inputs(T, H, seed=7):
    g = gen(seed * 1000003 + T * 131 + H)
    x = torch.randn(T, H, generator=g).to(BF16)
    r = torch.randn(T, H, generator=g).to(BF16)
    w = (1.0 + 0.1 * torch.randn(H, generator=g)).to(BF16)
    return x, r, w


@functools.lru_cache(maxsize=None)
def layernorm_inputs(T, H, mean=0.0, seed=11):
    """x, w, b for which one fp32 evaluation is inside one bf16 ulp of fp64.

    Two things would otherwise break the measure, in any fp32 layernorm and
    in torch_ref's as well (2.8 ulp at (4100, 2056) with free signs):
    - The rounding of the row mean shows wherever x is close to the mean.
      Rows are pairs |a|, -|a| around `mean` on a 2^-8 grid (coarser where
      bf16 is), so every partial sum is a multiple of 2^-8 below 2^16, the
      fp32 row sum is exact in any order and the mean is exactly `mean`.
    - (x - mean) * inv * w and b cancel to any depth among millions of
      elements. Each column holds one sign of x - mean and b carries that
      sign (w > 0), so the last addition never cancels.
    The column signs are shuffled; the kernel has no path that depends on
    them."""
    assert H % 2 == 0
    g = gen(seed * 1000003 + T * 131 + H)
    a = (torch.randn(T, H // 2, generator=g).abs() * 256).round() / 256
    a = a.to(BF16).float()
    perm = torch.randperm(H, generator=g)
    sign = torch.cat([torch.ones(H // 2), -torch.ones(H // 2)])[perm]
    x = (torch.cat([a, -a], dim=1)[:, perm] + mean).to(BF16)
    assert torch.equal(x.double().sum(dim=1), torch.full((T,), mean * H).double())
    assert ((x.float() - mean) * sign >= 0).all()
    w = (1.0 + 0.1 * torch.randn(H, generator=g)).to(BF16)
    b = (0.1 * torch.randn(H, generator=g).abs() * sign).to(BF16)
    assert (w > 0).all()
    return x, w, b


def rmsnorm64(x, w):
    xd = x.double()
    return xd * torch.rsqrt(xd.pow(2).mean(dim=-1, keepdim=True) + EPS32) * w.double()


def add_residual(x, r):
    return (x.float() + r.float()).to(BF16)


def layernorm64(x, w, b):
    """Two-pass: the variance is of the centred values."""
    xd = x.double()
    mu = xd.mean(dim=-1, keepdim=True)
    d = xd - mu
    inv = torch.rsqrt(d.pow(2).mean(dim=-1, keepdim=True) + EPS32)
    return d * inv * w.double() + b.double()


# ---------------------------------------------------------------------------
# SiLU * up
# ---------------------------------------------------------------------------

SILU_SWEEP = (1025, 4104)
SILU_UPS = (1.0, -3.0, 2.0**-20, 240.0)
# fp32 exp(-g) overflows from g = -89 down (88.5 is the last bf16 gate
# below ln(FLT_MAX) = 88.72): there g / (1 + inf) is exactly -0.
SILU_ZERO_GATE = -89.0


@functools.lru_cache(maxsize=None)
def silu_sweep_inputs(seed=3):
    T, inter = SILU_SWEEP
    assert T * inter > 2048 * 256 * 8 and inter % 8 == 0
    return (3.0 * torch.randn(T, 2 * inter, generator=gen(seed))).to(BF16)


@functools.lru_cache(maxsize=None)
def silu_exhaustive_inputs():
    """All 65536 bf16 gate patterns x SILU_UPS as [512, 2*512]."""
    gates = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)
    gate = gates.repeat(len(SILU_UPS)).view(512, 512)
    up = torch.tensor(SILU_UPS).to(BF16).repeat_interleave(65536).view(512, 512)
    assert torch.equal(up.float().unique(), torch.tensor(sorted(SILU_UPS)))
    return torch.cat([gate, up], dim=1).contiguous()


def silu_mul64(gate_up):
    g, u = gate_up.double().chunk(2, dim=-1)
    return g / (1.0 + torch.exp(-g)) * u


def silu_expectation(gate_up):
    """(ref64, finite mask, nan mask, inf mask, zero mask, zero bits).

    finite: compare at 1 ulp. nan / inf: where fp64, rounded to bf16's
    range, gives them. zero: finite gates <= SILU_ZERO_GATE, where the fp32
    formula gives exactly -0 * up (fp64 gives about -g * e^g there, down to
    2e-37, which no fp32 evaluation of g / (1 + exp(-g)) produces; torch's
    own fp32 silu returns the same zero)."""
    g, u = gate_up.float().chunk(2, dim=-1)
    ref = silu_mul64(gate_up)
    as_bf16 = ref.float().to(BF16)
    nan = torch.isnan(as_bf16)
    inf = torch.isinf(as_bf16)
    zero = torch.isfinite(g) & (g <= SILU_ZERO_GATE)
    # -0 * u: the sign is the opposite of u's, for u = +-0 as well
    zero_bits = torch.where(torch.signbit(u), 0, -32768).to(torch.int16)
    finite = ~nan & ~inf & ~zero
    return ref, finite, nan, inf, zero, zero_bits


# ---------------------------------------------------------------------------
# RoPE + append
# ---------------------------------------------------------------------------

ROPE_T = 37
ROPE_BLOCKS = 6
ROPE_HEADS = [(8, 2), (12, 12), (5, 1)]
ROPE_MAXPOS = 64


@functools.lru_cache(maxsize=None)
def rope_inputs(D, Hq, Hk, seed=5):
    """fused [T, (Hq + 2 Hk) D] bf16 (q | k | v column ranges), positions,
    fp32 cos / sin, slots (a random permutation over ROPE_BLOCKS blocks)."""
    g = gen(seed * 7919 + D * 31 + Hq * 5 + Hk)
    T = ROPE_T
    fused = torch.randn(T, (Hq + 2 * Hk) * D, generator=g).to(BF16)
    pos = torch.randint(0, ROPE_MAXPOS, (T,), generator=g)
    cos, sin = torch_ref.build_rope_cache(D, ROPE_MAXPOS, 10000.0)
    slots = torch.randperm(ROPE_BLOCKS * BS, generator=g)[:T]
    return fused, pos, cos, sin, slots


def split_qkv(fused, Hq, Hk, D):
    T = fused.shape[0]
    q = fused[:, : Hq * D].view(T, Hq, D)
    k = fused[:, Hq * D : (Hq + Hk) * D].view(T, Hk, D)
    v = fused[:, (Hq + Hk) * D :].view(T, Hk, D)
    return q, k, v


def rope64(x, pos, cos, sin):
    """(rotated fp64, slack): slack = 2^-21 (|x1| + |x2|) covers the fp32
    rounding of the two products before they cancel."""
    xd = x.double()
    h = x.shape[-1] // 2
    c = cos[pos].double().unsqueeze(1)
    s = sin[pos].double().unsqueeze(1)
    x1, x2 = xd[..., :h], xd[..., h:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    slack = 2.0**-21 * (x1.abs() + x2.abs())
    return rot, torch.cat([slack, slack], dim=-1)


def sentinel_cache(Hk, D, blocks=ROPE_BLOCKS):
    return torch.full((blocks, Hk, BS, D), SENTINEL, dtype=BF16)


def cache_rows(cache, slots):
    """[T, Hk, D] rows of a [N, Hk, BS, D] cache at flat slots."""
    return cache[slots // BS, :, slots % BS]


def untouched_rows(cache, slots):
    m = torch.ones(cache.shape[0] * BS, dtype=torch.bool)
    m[slots] = False
    idx = m.nonzero().flatten()
    return cache_rows(cache, idx)


# ---------------------------------------------------------------------------
# Decode attention
# ---------------------------------------------------------------------------

DECODE_CONFIGS = [(8, 2, 128), (8, 1, 128), (4, 4, 128), (4, 4, 64)]
SEL_LEN = 520
SEL_PAGES = (SEL_LEN + BS - 1) // BS  # 33
SEL_SPARE = 2  # table entries past the last page
GUARD_LENS = (1, 15, 16, 17, 63, 64, 65, 520)


def selected_values(shape, g):
    """bf16 with |v| in [2^-6, 4], random sign."""
    mag = torch.exp2(torch.rand(shape, generator=g) * 8.0 - 6.0)
    sign = torch.randint(0, 2, shape, generator=g) * 2.0 - 1.0
    v = (mag * sign).to(BF16)
    a = v.float().abs()
    assert a.min() >= 2.0**-6 and a.max() <= 4.0
    return v


def strided_q(q):
    """The same values as a row-strided view (dense heads)."""
    T, Hq, D = q.shape
    buf = torch.zeros(T, Hq * D + 2 * D, dtype=q.dtype)
    view = buf[:, D : D + Hq * D].view(T, Hq, D)
    view.copy_(q)
    assert not view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def decode_selection_inputs(Hq, Hkv, D, seed=21):
    """q, kc, vc, bt, kv_lens, scale, expected [B, Hq, D].

    Query head h of sequence b is 16 e_h; the key at position b*Hq + h of
    its kv head is 32 e_h and every other key is zero, so that key leads by
    16*32/sqrt(D) >= 45.25 and the output is its V row exactly (the other
    <= 519 keys, V = 100, weigh <= 519 e^-45.25 * 100 ~ 1e-15 < half an ulp
    of 2^-6). Across the batch every position 0..519 is selected once."""
    g = gen(seed + Hq * 100 + Hkv * 10 + D)
    G = Hq // Hkv
    B = SEL_LEN // Hq
    assert B * Hq == SEL_LEN and Hq <= D
    W = SEL_PAGES + SEL_SPARE
    NB = B * W + 3
    bt = torch.randperm(NB, generator=g)[: B * W].view(B, W).to(torch.int32)
    kc = torch.zeros(NB, Hkv, BS, D, dtype=BF16)
    vc = torch.full((NB, Hkv, BS, D), 100.0, dtype=BF16)
    q = torch.zeros(B, Hq, D, dtype=BF16)
    want = selected_values((B, Hq, D), g)
    b_idx = torch.arange(B).view(B, 1).expand(B, Hq)
    h_idx = torch.arange(Hq).view(1, Hq).expand(B, Hq)
    j = b_idx * Hq + h_idx
    blk = bt.long()[b_idx, j // BS]
    q[b_idx, h_idx, h_idx] = 16.0
    kc[blk, h_idx // G, j % BS, h_idx] = 32.0
    vc[blk, h_idx // G, j % BS] = want
    assert torch.equal(j.flatten().sort().values, torch.arange(SEL_LEN))
    kv_lens = torch.full((B,), SEL_LEN, dtype=torch.int32)
    return strided_q(q), kc, vc, bt, kv_lens, 1.0 / math.sqrt(D), want


def selection_short_lens(Hq, B):
    """kv_len that just covers each sequence's own selected keys: short
    sequences leave most splits empty."""
    return ((torch.arange(B) + 1) * Hq).to(torch.int32)


@functools.lru_cache(maxsize=None)
def decode_randn_inputs(Hq, Hkv, D, B, q_scale=1.0, seed=23):
    g = gen(seed + Hq * 100 + Hkv * 10 + D + B * 1000)
    W = SEL_PAGES + SEL_SPARE
    NB = B * W + 3
    bt = torch.randperm(NB, generator=g)[: B * W].view(B, W).to(torch.int32)
    kc = torch.randn(NB, Hkv, BS, D, generator=g).to(BF16)
    vc = torch.randn(NB, Hkv, BS, D, generator=g).to(BF16)
    q = (q_scale * torch.randn(B, Hq, D, generator=g)).to(BF16)
    return strided_q(q), kc, vc, bt, 1.0 / math.sqrt(D)


def guard_lens(B):
    return torch.tensor([GUARD_LENS[i % len(GUARD_LENS)] for i in range(B)],
                        dtype=torch.int32)


def uniform_code_cache(shape, g):
    """Uniformly random finite e4m3fn codes (no 0x7F / 0xFF)."""
    c = torch.arange(256, dtype=torch.int32)
    c = c[(c & 0x7F) != 0x7F].to(torch.uint8)
    return c[torch.randint(0, 254, shape, generator=g)].view(FP8)


def live_slots(NB, bt, kv_lens):
    """[NB, BS] bool: slots at positions < kv_len of an owned page."""
    live = torch.zeros(NB, BS, dtype=torch.bool)
    n_seq, W = bt.shape
    pos = torch.arange(W * BS).view(1, -1).expand(n_seq, -1)
    ok = pos < kv_lens.view(-1, 1).long()
    blk = bt.long().gather(1, pos // BS)
    live[blk[ok], (pos % BS)[ok]] = True
    return live


def poison_dead(kc, vc, bt, kv_lens):
    """NaN (bf16) or code 0x7F (FP8) in every slot >= kv_len, every unowned
    block and every block that an unused table entry names. All of these are
    legal addresses: a kernel that read one would pick up a NaN, not fault."""
    live = live_slots(kc.shape[0], bt, kv_lens)
    assert not live.all(dim=1).all() and (~live.any(dim=1)).any()
    m = live.view(-1, 1, BS, 1)
    if kc.dtype == FP8:
        bad = torch.tensor(0x7F, dtype=torch.uint8)
        out = [torch.where(m, c.view(torch.uint8), bad).view(FP8) for c in (kc, vc)]
        assert torch.isnan(out[0].float()).any()
    else:
        bad = torch.tensor(float("nan"), dtype=BF16)
        out = [torch.where(m, c, bad) for c in (kc, vc)]
    used = (kv_lens.long() + BS - 1) // BS
    for i in range(bt.shape[0]):
        for blk in bt[i, int(used[i]):].tolist():
            assert torch.isnan(out[0][blk].float()).all()
    return out[0], out[1]


# ---------------------------------------------------------------------------
# Prefill causal boundary probes
# ---------------------------------------------------------------------------

PREFILL_VARIANTS = [6, 5, 0]
PREFILL_GD = [(4, 128), (2, 128), (8, 128), (1, 128), (1, 64)]
PREFILL_SEQS = ((0, 70), (40, 37), (130, 16), (63, 2))


def probe_positions(prefix, chunk):
    """First and last query of the chunk and both sides of every 16-key
    boundary inside it (every 32- and 64-key boundary is one of those)."""
    lo, hi = prefix, prefix + chunk - 1
    want = {lo, hi}
    for edge in range(BS, hi + 1, BS):
        for p in (edge - 1, edge):
            if lo <= p <= hi:
                want.add(p)
    return sorted(want)


@functools.lru_cache(maxsize=None)
def prefill_probe_inputs(G, D, seed=31):
    """q, cu_q, q_pos, kc, vc, bt, kv_lens, scale, probes.

    probes: list of (token row, q head, expected V row [D]). Probe i of a kv
    head owns dim i: its query is 16 e_i, the key at its own position p has
    +32 on dim i and the key at p + 1 -- the future, score 2x larger -- has
    +64. For the last position of a sequence p + 1 is slot kv_len of the
    last page. Every other query is zero."""
    g = gen(seed + G * 1000 + D)
    Hkv = 2
    Hq = Hkv * G
    kv_lens = [p + c for p, c in PREFILL_SEQS]
    assert all(n % BS for n in kv_lens)  # slot kv_len is in the last page
    P = len(PREFILL_SEQS)
    W = (max(kv_lens) + BS - 1) // BS
    NB = P * W + 2
    bt = torch.randperm(NB, generator=g)[: P * W].view(P, W).to(torch.int32)
    kc = torch.zeros(NB, Hkv, BS, D, dtype=BF16)
    vc = torch.full((NB, Hkv, BS, D), 100.0, dtype=BF16)
    cu = [0]
    for _, c in PREFILL_SEQS:
        cu.append(cu[-1] + c)
    q = torch.zeros(cu[-1], Hq, D, dtype=BF16)
    q_pos = torch.cat(
        [torch.arange(p, p + c, dtype=torch.long) for p, c in PREFILL_SEQS]
    )
    probes = []
    i = 0
    for s, (prefix, chunk) in enumerate(PREFILL_SEQS):
        for p in probe_positions(prefix, chunk):
            assert i < D
            row = cu[s] + p - prefix
            for kvh in range(Hkv):
                head = kvh * G + i % G
                q[row, head, i] = 16.0
                kc[int(bt[s, p // BS]), kvh, p % BS, i] += 32.0
                kc[int(bt[s, (p + 1) // BS]), kvh, (p + 1) % BS, i] += 64.0
                v = selected_values((D,), g)
                vc[int(bt[s, p // BS]), kvh, p % BS] = v
                probes.append((row, head, v, s, p))
            i += 1
    return (
        strided_q(q), torch.tensor(cu, dtype=torch.int32), q_pos, kc, vc, bt,
        torch.tensor(kv_lens, dtype=torch.int32), 1.0 / math.sqrt(D), probes,
    )


# ---------------------------------------------------------------------------
# Exact integer GEMMs
# ---------------------------------------------------------------------------

def ternary(shape, g):
    return torch.randint(-1, 2, shape, generator=g).to(BF16)


def exact_product(x, w):
    """x @ w^T of ternary operands: every product and partial sum is an
    integer below 2^24 (exact in fp32 in any order); |sum| <= 256 is exact
    in bf16 as well."""
    ref = x.double() @ w.double().transpose(-1, -2)
    assert ref.abs().max() <= 256
    out = ref.to(BF16)
    assert torch.equal(out.double(), ref)
    return out


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K, seed=41):
    g = gen(seed + M * 7 + N * 101 + K * 13)
    x, w = ternary((M, K), g), ternary((N, K), g)
    return x, w, exact_product(x, w)


def strided_rows(t, pad=8):
    """The same [M, K] values as a view with a larger row stride whose rows
    stay 16-byte aligned."""
    M, K = t.shape
    buf = torch.zeros(M, K + 2 * pad, dtype=t.dtype)
    v = buf[:, pad : pad + K]
    v.copy_(t)
    return v


MOE_COUNTS = [0, 1, 15, 16, 17, 33, 0, 5]
MOE_GAP_AFTER = 3  # rows [gap0, gap0 + 3) after expert 3 belong to no one
MOE_N, MOE_K = 40, 512


@functools.lru_cache(maxsize=None)
def moe_inputs(seed=43):
    """x [P, K], w [E, N, K], counts, offsets, expected [P, N] (sentinel in
    the gap rows), gap row indices."""
    g = gen(seed)
    offsets, o = [], 0
    for e, c in enumerate(MOE_COUNTS):
        offsets.append(o)
        o += c
        if e == MOE_GAP_AFTER:
            gap = list(range(o, o + 3))
            o += 3
    P = o
    x = ternary((P, MOE_K), g)
    w = ternary((len(MOE_COUNTS), MOE_N, MOE_K), g)
    want = torch.full((P, MOE_N), SENTINEL, dtype=BF16)
    owned = torch.zeros(P, dtype=torch.bool)
    for e, (c, off) in enumerate(zip(MOE_COUNTS, offsets)):
        if c:
            want[off : off + c] = exact_product(x[off : off + c], w[e])
            assert not owned[off : off + c].any()
            owned[off : off + c] = True
    assert (~owned).nonzero().flatten().tolist() == gap
    return (
        x, w, torch.tensor(MOE_COUNTS, dtype=torch.int32),
        torch.tensor(offsets, dtype=torch.int32), want, gap,
    )


# ---------------------------------------------------------------------------
# Samplers
# ---------------------------------------------------------------------------

V1_VOCABS = [33, 1000, 50257]
V2_VOCABS = [4099, 50257]
S2_SLICES = 16
SAMPLER_ROWS = 32


def boundary_indices(V):
    """lo and hi - 1 of each of the gridded sampler's 16 slices: 32 indices
    that include 0 and V - 1 (duplicates where V is small)."""
    idx = []
    for s in range(S2_SLICES):
        lo, hi = s * V // S2_SLICES, (s + 1) * V // S2_SLICES
        idx += [lo, max(lo, hi - 1)]
    assert idx[0] == 0 and idx[-1] == V - 1 and len(idx) == SAMPLER_ROWS
    return idx


def boundary_logits(V):
    """[32, V]: a floor of 0 and +20 at one boundary index per row. That
    token holds e^20 / (e^20 + V - 1) > 0.999 of the mass."""
    idx = boundary_indices(V)
    x = torch.zeros(len(idx), V)
    x[torch.arange(len(idx)), idx] = 20.0
    p = torch.softmax(x.double(), dim=-1)[torch.arange(len(idx)), idx]
    assert p.min() > 0.999
    return x, torch.tensor(idx)


def reference_nucleus(logits_row, T, top_p):
    """(token ids, renormalised fp64 probabilities) of torch_ref's rule:
    sorted descending, kept while the exclusive cumulative mass < top_p."""
    probs = torch.softmax(logits_row.double() / T, dim=-1)
    sp, si = torch.sort(probs, descending=True)
    keep = (torch.cumsum(sp, 0) - sp) < top_p
    keep[0] = True
    ids, p = si[keep], sp[keep]
    return ids, p / p.sum()


NUCLEUS_TOKENS = 12
NUCLEUS_STEP = 0.25  # in y = (logit - max) / T: 8.5 histogram bins of 30/1024


def nucleus_row(V, T, k, g):
    """(logits [V], top_p, nucleus ids, renormalised probabilities).

    Twelve tokens at y = 0, -0.25, ..., -2.75 (y = logit / T) at random
    places that include 0 and V - 1; everything else at y = -25 (inside the
    histogram), -40 (below it) or -inf, in turn. top_p is the middle of
    token k's mass, so the nucleus is the top k + 1 tokens."""
    y = torch.tensor([-25.0, -40.0, float("-inf")]).repeat(V // 3 + 1)[:V].clone()
    where = torch.randperm(V - 2, generator=g)[: NUCLEUS_TOKENS - 2] + 1
    where = torch.cat([torch.tensor([0, V - 1]), where])
    where = where[torch.randperm(NUCLEUS_TOKENS, generator=g)]
    y[where] = -NUCLEUS_STEP * torch.arange(NUCLEUS_TOKENS)
    logits = (y * T).float()
    p = torch.softmax(logits.double() / T, dim=-1)
    top_p = float(p[where[:k]].sum() + 0.5 * p[where[k]])
    ids, pn = reference_nucleus(logits, T, top_p)
    assert ids.tolist() == where[: k + 1].tolist()
    for d in (-1e-3, 1e-3):
        assert reference_nucleus(logits, T, top_p + d)[0].tolist() == ids.tolist()
    return logits, top_p, ids, pn


@functools.lru_cache(maxsize=None)
def nucleus_case(V, T=1.0, k=7, seed=51):
    return nucleus_row(V, T, k, gen(seed + V))


@functools.lru_cache(maxsize=None)
def mixed_rows(V, seed=53):
    """32 rows alternating T = 0 and T = 0.8, top_p varying per row (the
    nucleus is the top 2..12 tokens). Returns logits, temps, top_ps, and per
    row the reference nucleus ids (the argmax alone for greedy rows)."""
    g = gen(seed + V)
    rows, temps, top_ps, allowed = [], [], [], []
    for r in range(SAMPLER_ROWS):
        k = 1 + r % (NUCLEUS_TOKENS - 1)
        logits, top_p, ids, _ = nucleus_row(V, 0.8, k, g)
        greedy = r % 2 == 0
        rows.append(logits)
        temps.append(0.0 if greedy else 0.8)
        top_ps.append(top_p)
        assert int(torch.argmax(logits)) == int(ids[0])
        allowed.append(ids[:1].tolist() if greedy else ids.tolist())
    return torch.stack(rows), torch.tensor(temps), torch.tensor(top_ps), allowed


def single_entry_rows(V, seed=57):
    """[32, V] of -inf with one finite entry per row, at the slice-boundary
    indices; the entry's value varies in sign."""
    idx = boundary_indices(V)
    x = torch.full((len(idx), V), float("-inf"))
    val = torch.linspace(-9.0, 9.0, len(idx))
    x[torch.arange(len(idx)), idx] = val
    return x, torch.tensor(idx)
