"""Models, weights and the fixed batch script of the model-forward tests.

Specs are the smallest at which every custom kernel still runs:
hidden_size 512 gives K % 512 == 0, so linears at M <= 16 take the skinny
GEMM (a hidden size of 256 would send every linear to hipBLASLt).

The script is a fixed list of ``ForwardBatch``es over one ``KVCachePool``
(block_size 16). Tokens are teacher-forced from fixed lists, never sampled.
Sequences: A (70 prompt tokens, crosses the 64-key tile), B (33), C (17),
nine short ones S3..S11 (3..11 tokens), six one-token ones X0..X5 and D (17).

  step  0  prefill A[0:40] + B[0:33]                       T=73
  step  1  prefill A[40:70] over its prefix + C[0:17], decode B   T=48
           (sample_indices: a strict, unsorted subset of rows)
  step  2-4  decode {B, A, C}                               M=3
  step  5  prefill S3..S11                                  T=63
  step  6-7  decode the twelve                              M=12
  step  8  prefill X0..X5, one token each                   T=6
  step  9  decode all eighteen (kv_len 1 -> 2 for X*)       M=18
  step 10  prefill D alone                                  T=17

Step 10 exists for the MoE model: it is the only way a 17-token
prefill reaches ``MoEMLP._forward_grouped`` (T * top_k = 34 <= 64): C's 17
tokens share step 1 with 31 others, which takes the per-expert loop.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import torch

from dts_amd.models.config import ModelSpec
from dts_amd.serving.batch import ForwardBatch
from dts_amd.serving.kv_cache import KVCachePool

BLOCK_SIZE = 16
WEIGHT_SEED = 1234

# Embedding rows scaled down so that their mean square is near rms_eps
# (1e-5): only there does a wrong epsilon rise above the bf16 noise.
SMALL_TOKENS = (1, 2, 3)
# GPT-2: position rows scaled down likewise (LayerNorm sees wte + wpe).
SMALL_POSITIONS = (2, 35, 41)


def _llama(name, hq, hkv, d):
    return ModelSpec(
        name=name, arch="llama", vocab_size=1024, hidden_size=512,
        intermediate_size=1024, num_layers=2, num_heads=hq, num_kv_heads=hkv,
        head_dim=d, rope_theta=10000.0, rms_eps=1e-5, layernorm_eps=1e-3,
        max_position=256,
    )


SPECS = {
    "llama-g4-d128": _llama("llama-g4-d128", 8, 2, 128),  # q_size != hidden
    "llama-g8-d128": _llama("llama-g8-d128", 8, 1, 128),
    "llama-g1-d64": _llama("llama-g1-d64", 8, 8, 64),
    "mixtral-g4-d128": ModelSpec(
        name="mixtral-g4-d128", arch="mixtral", vocab_size=1024,
        hidden_size=512, intermediate_size=512, num_layers=2, num_heads=8,
        num_kv_heads=2, head_dim=128, rope_theta=1000000.0, rms_eps=1e-5,
        layernorm_eps=1e-3, max_position=256, num_experts=4,
        experts_per_token=2,
    ),
    "gpt2-d64": ModelSpec(
        name="gpt2-d64", arch="gpt2", vocab_size=1000, hidden_size=512,
        intermediate_size=2048, num_layers=2, num_heads=8, num_kv_heads=8,
        head_dim=64, rms_eps=1e-3, layernorm_eps=1e-5, max_position=256,
        tie_embeddings=True,
    ),
}


# ---------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------

# name -> (prompt length, total length incl. the teacher-forced decode steps)
SEQ_LENGTHS = {"A": (70, 76), "B": (33, 40), "C": (17, 23), "D": (17, 17)}
SEQ_LENGTHS.update({f"S{n}": (n, n + 3) for n in range(3, 12)})
SEQ_LENGTHS.update({f"X{i}": (1, 2) for i in range(6)})
SEQ_NAMES = list(SEQ_LENGTHS)

# positions that carry a SMALL_TOKENS id: in the first prefill, in the
# chunk over a cached prefix, in decode steps of every M
_SMALL_AT = {
    "A": (2, 35, 41, 71, 74), "B": (5, 34, 38), "C": (3, 18, 21),
    "S5": (1, 6), "S9": (0, 10), "X2": (0,), "X4": (1,), "D": (7,),
}


def _random_sequences(vocab: int) -> dict:
    g = torch.Generator().manual_seed(20240607)
    seqs = {}
    for name, (_, total) in SEQ_LENGTHS.items():
        toks = torch.randint(4, vocab, (total,), generator=g).tolist()
        for j, p in enumerate(_SMALL_AT.get(name, ())):
            toks[p] = SMALL_TOKENS[j % len(SMALL_TOKENS)]
        seqs[name] = toks
    return seqs


# Mixtral's token lists are fixed literals: found once by
# search_mixtral_sequences() below so that the router-probability gap
# between the 2nd and 3rd expert is >= ROUTING_GAP at every token of every
# layer, for the bf16 and for the fp32 build of the weights. No token of
# the scenario ever has to be excluded from a comparison (the cap is zero);
# tests/models/test_dense_ref_cpu.py asserts it.
ROUTING_GAP = 0.02
MIXTRAL_SEQUENCES: dict = {}  # filled in below the search function


def sequences_for(spec: ModelSpec) -> dict:
    if spec.arch == "mixtral":
        return {k: list(v) for k, v in MIXTRAL_SEQUENCES.items()}
    return _random_sequences(spec.vocab_size)


def search_mixtral_sequences(models: list, seed: int = 7) -> dict:
    """How MIXTRAL_SEQUENCES was found (not run by any test): a greedy
    left-to-right draw. Routing at position t depends on tokens 0..t only,
    so each position keeps the first candidate whose 2nd/3rd gap, in the
    exact reference of every model in `models`, is >= ROUTING_GAP + 0.005."""
    from tests.models._dense_ref import dense_forward, read_params

    params = [read_params(m) for m in models]
    g = torch.Generator().manual_seed(seed)
    vocab = models[0].spec.vocab_size
    found = {}
    for name, (_, total) in SEQ_LENGTHS.items():
        toks: list = []
        small = _SMALL_AT.get(name, ())
        for pos in range(total):
            for attempt in range(200):
                if pos in small and attempt < 3:
                    cand = SMALL_TOKENS[(small.index(pos) + attempt) % 3]
                else:
                    cand = int(torch.randint(4, vocab, (1,), generator=g))
                ok = True
                for m, P in zip(models, params):
                    ref = dense_forward(m, [toks + [cand]], params=P)[0]
                    if min_routing_gap([ref], last_only=True) < ROUTING_GAP + 0.005:
                        ok = False
                        break
                if ok:
                    toks.append(cand)
                    break
            else:
                raise RuntimeError(f"no token found for {name}[{pos}]")
        found[name] = toks
    return found


def min_routing_gap(refs: list, last_only: bool = False) -> float:
    """Smallest (2nd - 3rd) router probability over the reference results."""
    gap = 1.0
    for ref in refs:
        for probs in ref["router_probs"]:
            p = probs[-1:] if last_only else probs
            top = torch.topk(p, 3, dim=-1).values
            gap = min(gap, float((top[:, 1] - top[:, 2]).min()))
    return gap


MIXTRAL_SEQUENCES.update(
    {
        "A": [
            319, 536, 3, 845, 30, 271, 651, 755, 132, 121, 486, 494, 367,
            802, 704, 115, 752, 732, 371, 754, 880, 347, 989, 940, 864, 743,
            928, 396, 65, 336, 866, 243, 711, 4, 24, 2, 629, 16, 451, 684,
            124, 3, 723, 786, 933, 696, 399, 831, 836, 439, 932, 455, 279,
            295, 733, 800, 673, 282, 337, 821, 677, 85, 741, 1007, 471, 271,
            882, 473, 471, 543, 86, 3, 883, 244, 3, 804,
        ],
        "B": [
            29, 404, 783, 238, 416, 2, 45, 500, 783, 563, 127, 684, 279,
            784, 298, 850, 1006, 955, 943, 193, 338, 11, 369, 440, 96, 979,
            909, 120, 770, 809, 241, 428, 111, 573, 2, 420, 396, 813, 3, 589,
        ],
        "C": [
            953, 82, 980, 1, 516, 966, 428, 34, 44, 102, 703, 6, 982, 60,
            737, 978, 265, 233, 559, 565, 714, 3, 597,
        ],
        "D": [
            932, 472, 454, 1019, 141, 943, 989, 1, 612, 739, 312, 313, 959,
            966, 828, 865, 809,
        ],
        "S3": [
            870, 804, 619, 1023, 351, 781,
        ],
        "S4": [
            665, 412, 447, 677, 79, 150, 175,
        ],
        "S5": [
            520, 2, 863, 881, 476, 731, 2, 235,
        ],
        "S6": [
            129, 93, 632, 956, 626, 370, 744, 38, 760,
        ],
        "S7": [
            374, 733, 621, 737, 1015, 421, 715, 412, 296, 277,
        ],
        "S8": [
            371, 98, 16, 658, 554, 590, 464, 823, 200, 47, 661,
        ],
        "S9": [
            2, 1008, 164, 798, 1011, 610, 634, 720, 581, 107, 2, 652,
        ],
        "S10": [
            698, 635, 788, 372, 636, 241, 530, 880, 634, 468, 963, 309, 84,
        ],
        "S11": [
            141, 94, 276, 644, 560, 17, 387, 205, 645, 341, 534, 818, 668,
            611,
        ],
        "X0": [
            231, 564,
        ],
        "X1": [
            275, 926,
        ],
        "X2": [
            2, 74,
        ],
        "X3": [
            884, 378,
        ],
        "X4": [
            727, 1,
        ],
        "X5": [
            10, 210,
        ],
    }
)


# ---------------------------------------------------------------------------
# models and weights
# ---------------------------------------------------------------------------

def _uniform(shape, g, lo, hi):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def perturb_weights_(model) -> None:
    """Overwrite what random_init leaves at its neutral value: every norm
    weight gets values in [0.5, 1.5], every GPT-2 bias (LN biases too)
    N(0, 0.1); a few embedding rows shrink to a mean square near eps."""
    g = torch.Generator().manual_seed(WEIGHT_SEED + 1)
    spec = model.spec

    def put(p, value):
        p.copy_(value.to(p.dtype).to(p.device))

    with torch.no_grad():
        if model.arch == "gpt2":
            for layer in model.layers:
                put(layer.ln1_w, _uniform(layer.ln1_w.shape, g, 0.5, 1.5))
                put(layer.ln2_w, _uniform(layer.ln2_w.shape, g, 0.5, 1.5))
                for b in (layer.ln1_b, layer.ln2_b, layer.qkv_b, layer.o_b,
                          layer.fc_b, layer.proj_b):
                    put(b, torch.randn(b.shape, generator=g) * 0.1)
            put(model.lnf_w, _uniform(model.lnf_w.shape, g, 0.5, 1.5))
            put(model.lnf_b, torch.randn(model.lnf_b.shape, generator=g) * 0.1)
            # var(wte + wpe) ~ 4e-4 + 1e-4; shrink both to ~1e-5 in total
            for t in SMALL_TOKENS:
                model.wte[t].mul_(0.1)
            for p in SMALL_POSITIONS:
                model.wpe[p].mul_(0.25)
        else:
            for layer in model.layers:
                put(layer.input_norm_w, _uniform(layer.input_norm_w.shape, g, 0.5, 1.5))
                put(layer.post_norm_w, _uniform(layer.post_norm_w.shape, g, 0.5, 1.5))
            put(model.final_norm_w, _uniform(model.final_norm_w.shape, g, 0.5, 1.5))
            # mean square 4e-4 -> ~1e-5 = rms_eps
            for t in SMALL_TOKENS:
                model.embed[t].mul_(0.16)
    assert spec.rms_eps != spec.layernorm_eps  # a swapped epsilon must show


def build_model(spec_name: str, device: str, dtype, weight_quant: bool = False):
    spec = SPECS[spec_name]
    if spec.arch == "llama":
        from dts_amd.models.llama import LlamaModel

        model = LlamaModel(spec, dtype=dtype, device=device)
    elif spec.arch == "mixtral":
        from dts_amd.models.mixtral import MixtralModel

        model = MixtralModel(spec, dtype=dtype, device=device)
    else:
        from dts_amd.models.gpt2 import GPT2Model

        model = GPT2Model(spec, dtype=dtype, device=device)
    model.random_init(WEIGHT_SEED)
    perturb_weights_(model)
    if weight_quant:
        from dts_amd.models.quant import quantize_model_

        quantize_model_(model, "fp8")
    return model


def kv_scales_for(spec: ModelSpec) -> torch.Tensor:
    """[layers, 2, Hkv] powers of two in 2^-2..2^2 that differ per layer,
    per K/V and per head."""
    L, H = spec.num_layers, spec.num_kv_heads
    e = torch.empty(L, 2, H)
    for l in range(L):
        for kv in range(2):
            for h in range(H):
                e[l, kv, h] = (2 * l + 3 * kv + h) % 5 - 2
    e[0, 0, 0], e[L - 1, 1, 0] = -2, 2
    assert bool((e[0] != e[1]).any()) and bool((e[:, 0] != e[:, 1]).any())
    return torch.pow(2.0, e)


def make_pool(spec: ModelSpec, device: str, dtype, fp8: bool) -> KVCachePool:
    pool = KVCachePool(
        spec.num_layers, spec.num_kv_heads, spec.head_dim, NUM_BLOCKS,
        BLOCK_SIZE, dtype=torch.float8_e4m3fn if fp8 else dtype, device=device,
    )
    if fp8:
        pool.set_scales(kv_scales_for(spec))
    return pool


def fill_pool_nan_(pool: KVCachePool) -> None:
    """Every slot NaN (FP8: byte 0x7F). The script then overwrites exactly
    the slots it appends, so unused blocks and the slots past each kv_len
    stay NaN for the whole run."""
    for t in (pool.k, pool.v):
        if t.dtype == torch.float8_e4m3fn:
            t.view(torch.uint8).fill_(0x7F)
        else:
            t.fill_(float("nan"))


# ---------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------

def _blocks_needed(total: int) -> int:
    return (total + BLOCK_SIZE - 1) // BLOCK_SIZE


NUM_SPARE = 5
NUM_BLOCKS = sum(_blocks_needed(t) for _, t in SEQ_LENGTHS.values()) + NUM_SPARE


def block_tables(shuffle_seed: Optional[int]) -> tuple:
    """({name: [physical blocks]}, spare blocks). None = identity order."""
    ids = list(range(NUM_BLOCKS))
    if shuffle_seed is not None:
        g = torch.Generator().manual_seed(shuffle_seed)
        ids = [ids[i] for i in torch.randperm(NUM_BLOCKS, generator=g).tolist()]
    tables, at = {}, 0
    for name, (_, total) in SEQ_LENGTHS.items():
        n = _blocks_needed(total)
        tables[name] = ids[at : at + n]
        at += n
    return tables, ids[at:]


@dataclass
class Step:
    prefill: list = field(default_factory=list)  # (name, start, end)
    decode: list = field(default_factory=list)  # (name, position)
    sample: Optional[list] = None  # rows; None = every row (no indices)

    def rows(self) -> list:
        """(name, position) of every row of the flat batch."""
        out = [(n, p) for n, s, e in self.prefill for p in range(s, e)]
        return out + list(self.decode)

    def sampled_rows(self) -> list:
        rows = self.rows()
        return rows if self.sample is None else [rows[i] for i in self.sample]


def _last_rows(prefill: list) -> list:
    out, at = [], 0
    for _, s, e in prefill:
        at += e - s
        out.append(at - 1)
    return out


def script_steps() -> list:
    shorts = [f"S{n}" for n in range(3, 12)]
    singles = [f"X{i}" for i in range(6)]
    steps = [
        # last rows of B and A's chunk, B first: a strict, unsorted subset
        Step(prefill=[("A", 0, 40), ("B", 0, 33)], sample=[72, 39]),
        # rows 0..29 A[40:70], 30..46 C, 47 B's decode
        Step(prefill=[("A", 40, 70), ("C", 0, 17)], decode=[("B", 33)],
             sample=[47, 29, 46, 7]),
    ]
    pos = {n: SEQ_LENGTHS[n][0] for n in SEQ_NAMES}
    pos["B"] += 1

    def decode_step(names, sample):
        st = Step(decode=[(n, pos[n]) for n in names], sample=sample)
        for n in names:
            pos[n] += 1
        return st

    steps.append(decode_step(["B", "A", "C"], None))
    steps.append(decode_step(["B", "A", "C"], [0, 1, 2]))
    steps.append(decode_step(["B", "A", "C"], [2, 0]))
    pf = [(n, 0, SEQ_LENGTHS[n][0]) for n in shorts]
    steps.append(Step(prefill=pf, sample=_last_rows(pf)))
    twelve = ["B", "A", "C"] + shorts
    steps.append(decode_step(twelve, list(range(12))))
    steps.append(decode_step(twelve, list(range(12))))
    pf = [(n, 0, 1) for n in singles]
    steps.append(Step(prefill=pf, sample=_last_rows(pf)))
    steps.append(decode_step(twelve + singles, list(range(18))))
    steps.append(Step(prefill=[("D", 0, 17)], sample=[16, 0]))
    for n in SEQ_NAMES:  # every teacher-forced token is consumed
        assert max(p for s in steps for m, p in s.rows() if m == n) == SEQ_LENGTHS[n][1] - 1
    return steps


STEP_PREFILL_1, STEP_MIXED, STEP_M12, STEP_M18, STEP_D = 0, 1, 6, 9, 10
# which MoE path each step takes (T * top_k <= 64 -> grouped GEMM)
GROUPED_STEPS = (2, 3, 4, 6, 7, 8, 9, 10)


def prefill_masks(steps: list) -> dict:
    """{name: bool [total]}: positions whose attention ran in prefill."""
    masks = {n: torch.zeros(SEQ_LENGTHS[n][1], dtype=torch.bool) for n in SEQ_NAMES}
    for st in steps:
        for n, s, e in st.prefill:
            masks[n][s:e] = True
    return masks


def build_batch(step: Step, seqs: dict, tables: dict, pad_block: int,
                row_perm: Optional[list] = None) -> ForwardBatch:
    """The ForwardBatch of one step. Block tables are padded with
    `pad_block`, a spare block that no sequence owns. row_perm permutes the
    rows of a decode-only batch (new row j = old row row_perm[j])."""
    rows = step.rows()
    decode = list(step.decode)
    if row_perm is not None:
        assert not step.prefill
        rows = [rows[i] for i in row_perm]
        decode = [decode[i] for i in row_perm]
    tok = [seqs[n][p] for n, p in rows]
    posn = [p for _, p in rows]
    slots = [tables[n][p // BLOCK_SIZE] * BLOCK_SIZE + p % BLOCK_SIZE for n, p in rows]

    def table(names_lens):
        width = max(_blocks_needed(k) for _, k in names_lens)
        return torch.tensor(
            [
                (tables[n][: _blocks_needed(k)] + [pad_block] * width)[:width]
                for n, k in names_lens
            ],
            dtype=torch.int32,
        )

    kw = {}
    if step.prefill:
        pl = [(n, e) for n, _, e in step.prefill]
        cu = [0]
        for _, s, e in step.prefill:
            cu.append(cu[-1] + e - s)
        kw.update(
            num_prefill_seqs=len(pl), num_prefill_tokens=cu[-1],
            cu_q=torch.tensor(cu, dtype=torch.int32),
            prefill_block_tables=table(pl),
            prefill_kv_lens=torch.tensor([k for _, k in pl], dtype=torch.int32),
        )
    if decode:
        dl = [(n, p + 1) for n, p in decode]
        kw.update(
            num_decode_seqs=len(dl), decode_block_tables=table(dl),
            decode_kv_lens=torch.tensor([k for _, k in dl], dtype=torch.int32),
        )
    return ForwardBatch(
        token_ids=torch.tensor(tok, dtype=torch.long),
        positions=torch.tensor(posn, dtype=torch.long),
        slot_mapping=torch.tensor(slots, dtype=torch.long),
        sample_indices=(
            None if step.sample is None else torch.tensor(step.sample, dtype=torch.long)
        ),
        **kw,
    )


# ---------------------------------------------------------------------------
# running and capturing
# ---------------------------------------------------------------------------

def read_slots(pool: KVCachePool, slots: torch.Tensor, raw: bool = False):
    """K and V [layers, T, Hkv, D] at flat `slots`: fp32 values (FP8
    codes times their scale), or with raw=True the stored bytes."""
    blk = torch.div(slots, BLOCK_SIZE, rounding_mode="floor").to(pool.k.device)
    off = (slots % BLOCK_SIZE).to(pool.k.device)
    int_view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
    out = []
    for i, t in enumerate((pool.k, pool.v)):
        # two index tensors around a slice: the indexed dim comes first
        bits = t.view(int_view[t.element_size()])[:, blk, :, off].permute(1, 0, 2, 3)
        if raw:
            out.append(bits.cpu())
            continue
        x = bits.contiguous().view(t.dtype).float()
        if t.dtype == torch.float8_e4m3fn:
            x = x * pool.scales[:, i].float()[:, None, :, None]
        out.append(x.cpu())
    return out[0], out[1]


@dataclass
class StepCapture:
    resid: list  # per layer, fp32 [T, H]: the residual stream after it
    logits: torch.Tensor  # fp32 [sampled rows, V]
    k: torch.Tensor  # fp32 [layers, T, Hkv, D] read back from the pool
    v: torch.Tensor


def run_script(model, pool, seqs, steps, tables, pad_block, device,
               row_perm: Optional[dict] = None, after_step=None) -> list:
    """Runs every step through model.forward, eagerly. Residual streams
    come from forward hooks on model.layers[i], K/V from reading the pool
    at the slots the step wrote. after_step(i, pool) is called per step."""
    grabbed: list = []

    def hook(_mod, _args, output):
        if isinstance(output, tuple):  # (hidden, residual): their sum
            grabbed.append((output[0].float() + output[1].float()).cpu())
        else:
            grabbed.append(output.float().cpu())

    handles = [layer.register_forward_hook(hook) for layer in model.layers]
    caps = []
    try:
        with torch.no_grad():
            for i, st in enumerate(steps):
                perm = (row_perm or {}).get(i)
                batch = build_batch(st, seqs, tables, pad_block, perm)
                grabbed.clear()
                logits = model.forward(batch.to(device), pool)
                k, v = read_slots(pool, batch.slot_mapping)
                caps.append(StepCapture(list(grabbed), logits.float().cpu(), k, v))
                if after_step is not None:
                    after_step(i, pool)
    finally:
        for h in handles:
            h.remove()
    return caps


# ---------------------------------------------------------------------------
# reference rows and the error / noise rule
# ---------------------------------------------------------------------------

def reference_for(model, seqs: dict, steps: list, mode=None, kv_scales=None) -> dict:
    from tests.models._dense_ref import dense_forward

    masks = prefill_masks(steps)
    res = dense_forward(
        model, [seqs[n] for n in SEQ_NAMES], mode=mode, kv_scales=kv_scales,
        prefill_masks=[masks[n] for n in SEQ_NAMES],
    )
    return dict(zip(SEQ_NAMES, res))


def reference_step(ref: dict, step: Step, num_layers: int,
                   row_perm: Optional[list] = None) -> dict:
    """The reference's rows of one step, keyed like the checkpoints:
    'resid{l}', 'k{l}', 'v{l}' over all rows, 'logits' over sampled rows."""
    rows = step.rows()
    if row_perm is not None:
        rows = [rows[i] for i in row_perm]
    sampled = rows if step.sample is None else [rows[i] for i in step.sample]
    out = {"logits": torch.stack([ref[n]["logits"][p] for n, p in sampled])}
    for l in range(num_layers):
        out[f"resid{l}"] = torch.stack([ref[n]["resid"][l][p] for n, p in rows])
        out[f"k{l}"] = torch.stack([ref[n]["k"][l][p] for n, p in rows]).flatten(1)
        out[f"v{l}"] = torch.stack([ref[n]["v"][l][p] for n, p in rows]).flatten(1)
    return out


def capture_step(cap: StepCapture, num_layers: int) -> dict:
    out = {"logits": cap.logits.double()}
    for l in range(num_layers):
        out[f"resid{l}"] = cap.resid[l].double()
        out[f"k{l}"] = cap.k[l].double().flatten(1)
        out[f"v{l}"] = cap.v[l].double().flatten(1)
    return out


def row_rel_err(x: torch.Tensor, exact: torch.Tensor) -> torch.Tensor:
    """Per-row relative L2 error, [rows]."""
    return (x - exact).norm(dim=-1) / exact.norm(dim=-1)


def noise_of(rounded: torch.Tensor, exact: torch.Tensor) -> float:
    """RMS over rows of the rounded reference's per-row relative error."""
    return float(row_rel_err(rounded, exact).pow(2).mean().sqrt())


def kind_of(key: str) -> str:
    return key.rstrip("0123456789")
