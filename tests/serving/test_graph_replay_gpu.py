"""The captured-graph decode path (serving/graph_runner.py, serving/chain.py)
against things that are not themselves a replay: the dense fp64 reference
of tests/models/_dense_ref.py and an eager ``model.forward`` of the padded
batch that tests/serving/_graph_inputs.py derives from the runner's contract.

``DecodeGraphRunner`` is driven directly (max_bucket 16, static block tables
8 wide, scratch block = a spare block of the scenario, distinct from the
block the script pads its tables with). The script is the one of the model
tests with its second M=3 step split into n=1 and n=2
(``_graph_inputs.graph_script_steps``): prefill, mixed and the M=18 step
call ``model.forward``, every other decode step is replayed: n=3 in bucket 4
(one pad row), n=1 in bucket 1, n=2 in bucket 2, n=12 in bucket 16 (four pad
rows). Graphs are captured on the default statics (token 0, position 0,
kv_len 1, scratch block) and only ever replayed with other contents.

Rules:

* fp64: logits of the real rows and the K/V read back at the step's slots
  stay within MARGIN = 4 times the ``rounded`` noise of the checkpoint, the
  rule of test_model_forward_gpu.py (residual streams are not observable in
  a replay).
* eager: the replay's logits for all B rows and every byte of the pool
  outside the scratch block are ``torch.equal`` to an eager forward of the
  padded batch; a tight block table gives the same bits as the 8-wide one.
* NaN in every slot (scratch block included) before the first capture
  changes nothing and stays wherever the script does not write.
* a narrower replay after a fuller one of the same bucket leaves the dropped
  row's blocks alone; a replay is unchanged by a capture and replay of
  another bucket and by an eager call that shares the attention workspace.
* FP8 KV scales set after capture are the scales a replay uses.
* Mixtral: the replays of bucket 4 do not share one expert histogram, and
  none has the histogram of the capture (checked on the reference).
* ChainRunner: 20 chained steps from positions 15 / 16 / 63 (+ a pad row
  that wraps inside the scratch block) against the same steps built on the
  host from ``chain_expected``: tokens, final statics, every cache byte.

Observed maximum error/noise ratio per case over the replayed steps on an
MI355X (margin 4):

  spec / weights / KV cache           logits      k      v   chain step 1
  llama-g4-d128-wbf16-kvbf16            1.37   1.22   1.17           1.06
  llama-g4-d128-wfp8-kvbf16             1.32   1.25   1.27           1.26
  llama-g4-d128-wbf16-kvfp8             1.41   1.26   1.19           1.18
  llama-g1-d64-wbf16-kvbf16             1.17   1.26   1.30           1.11
  mixtral-g4-d128-wbf16-kvbf16          1.14   1.30   1.33           1.03
  gpt2-d64-wbf16-kvbf16                 1.12   1.14   1.14           1.01
  llama-g4-d128-wbf16-kvfp8, scales
    set after capture                   1.41   1.26   1.19              -

Every ``torch.equal`` rule held in all six cases: no kernel's arithmetic
depends on capture, on the static table width or on the pad rows' contents.
"""

from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import pytest
import torch

from dts_amd import ops
from dts_amd.llm.types import SamplingParams
from dts_amd.serving.batch import ForwardBatch
from dts_amd.serving.chain import ChainRunner
from dts_amd.serving.graph_runner import DecodeGraphRunner
from dts_amd.serving.kv_cache import KVCachePool
from tests.models import _scenarios as S
from tests.models._dense_ref import dense_forward
from tests.serving import _graph_inputs as G

pytestmark = pytest.mark.gpu

MARGIN = 4.0
DEV = "cuda"
BS = S.BLOCK_SIZE
SHUFFLE = 11

# (spec, fp8 weights, fp8 kv cache)
KV_CASE = ("llama-g4-d128", False, True)
CASES = [
    ("llama-g4-d128", False, False),
    ("llama-g4-d128", True, False),
    KV_CASE,
    ("llama-g1-d64", False, False),
    ("mixtral-g4-d128", False, False),
    ("gpt2-d64", False, False),
]

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _case_id(c):
    return f"{c[0]}-w{'fp8' if c[1] else 'bf16'}-kv{'fp8' if c[2] else 'bf16'}"


def pool_bytes(pool, scratch=None) -> torch.Tensor:
    """The stored bits [2 (K, V), layers, blocks, Hkv, 16, D] on the CPU,
    the scratch block zeroed."""
    out = torch.stack([t.view(_INT[t.element_size()]).cpu() for t in (pool.k, pool.v)])
    if scratch is not None:
        out[:, :, scratch] = 0
    return out


def slots_of(bits: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Rows of `bits` at the flat slots where bool `mask` [blocks * 16] is set."""
    per_slot = bits.permute(2, 4, 0, 1, 3, 5)  # [blocks, 16, 2, L, Hkv, D]
    return per_slot.reshape(mask.numel(), -1)[mask]


def snapshot(pool):
    return pool.k.clone(), pool.v.clone()


def restore_(pool, snap) -> None:
    pool.k.copy_(snap[0])
    pool.v.copy_(snap[1])


@dataclass
class StepOut:
    replayed: bool
    n: int
    logits: torch.Tensor  # fp32; a graphable step: all B rows of the bucket
    k: torch.Tensor  # fp32 [layers, n, Hkv, D] at the step's slots
    v: torch.Tensor


@dataclass
class Run:
    steps: list
    bits: torch.Tensor  # pool_bytes without the scratch block
    written: torch.Tensor  # bool [blocks * 16]: slots the script appended


class Case:
    """One model, its references and the replay / eager runs, once per module."""

    def __init__(self, spec_name, fp8_w, fp8_kv):
        self.id = _case_id((spec_name, fp8_w, fp8_kv))
        self.spec = S.SPECS[spec_name]
        self.fp8_kv = fp8_kv
        self.model = S.build_model(spec_name, DEV, torch.bfloat16, weight_quant=fp8_w)
        self.seqs = S.sequences_for(self.spec)
        self.steps = G.graph_script_steps()
        self.scales = S.kv_scales_for(self.spec) if fp8_kv else None
        self.exact = S.reference_for(self.model, self.seqs, self.steps)
        self.rounded = S.reference_for(
            self.model, self.seqs, self.steps, mode=torch.bfloat16, kv_scales=self.scales
        )
        self.tables, spare = S.block_tables(SHUFFLE)
        self.pad, self.scratch = spare[0], spare[1]
        owned = {b for t in self.tables.values() for b in t}
        assert self.pad != self.scratch and not {self.pad, self.scratch} & owned
        self._runs: dict = {}

    # -- pools and runners ------------------------------------------------
    def new_pool(self, nan_fill=False, default_scales=False):
        if default_scales:
            assert self.fp8_kv
            pool = KVCachePool(
                self.spec.num_layers, self.spec.num_kv_heads, self.spec.head_dim,
                S.NUM_BLOCKS, BS, dtype=torch.float8_e4m3fn, device=DEV,
            )
            assert bool((pool.scales == 1).all())
        else:
            pool = S.make_pool(self.spec, DEV, torch.bfloat16, self.fp8_kv)
        if nan_fill:
            S.fill_pool_nan_(pool)
        return pool

    def new_runner(self, pool, scratch=None):
        return DecodeGraphRunner(
            self.model, pool, DEV, self.scratch if scratch is None else scratch,
            max_blocks_per_seq=G.MAX_BLOCKS, max_bucket=G.MAX_BUCKET,
        )

    def batch_of(self, decode):
        return S.build_batch(S.Step(decode=decode), self.seqs, self.tables, self.pad)

    def padded(self, batch, B, width=G.MAX_BLOCKS):
        return G.padded_decode_batch(batch, B, self.scratch, width, BS)

    # -- the script ---------------------------------------------------------
    def run(self, mode, nan_fill=False, late_scales=False) -> Run:
        """mode 'replay': graphable steps go through runner.run; 'wide' /
        'tight': through an eager forward of the padded batch with the
        8-wide / the batch's own table. late_scales: every bucket is
        captured on the pool's default scales, which are set afterwards."""
        pool = self.new_pool(nan_fill, default_scales=late_scales)
        runner = self.new_runner(pool)
        if late_scales:
            for n in (1, 2, 3, 12):
                runner.entry_for(n)
            torch.cuda.synchronize()
            pool.set_scales(self.scales)
        outs = []
        written = torch.zeros(S.NUM_BLOCKS * BS, dtype=torch.bool)
        with torch.inference_mode():
            for st in self.steps:
                batch = S.build_batch(st, self.seqs, self.tables, self.pad)
                written[batch.slot_mapping] = True
                graphable = runner.can_run(batch)
                n = batch.num_decode_seqs
                if graphable:
                    B = runner._bucket_for(n)
                    if mode == "replay":
                        out = runner.run(batch)
                        logits = runner._graphs[B]["logits"]
                        assert out.shape[0] == n and out.data_ptr() == logits.data_ptr()
                    else:
                        width = (G.MAX_BLOCKS if mode == "wide"
                                 else batch.decode_block_tables.shape[1])
                        logits = self.model.forward(
                            self.padded(batch, B, width).to(DEV), pool
                        )
                    assert logits.shape[0] == B
                else:
                    logits = self.model.forward(batch.to(DEV), pool)
                k, v = S.read_slots(pool, batch.slot_mapping)
                outs.append(StepOut(graphable, n, logits.float().cpu().clone(), k, v))
        if mode == "replay":
            assert sorted(runner._graphs) == [1, 2, 4, 16]
        else:
            assert not runner._graphs
        return Run(outs, pool_bytes(pool, self.scratch), written)

    def cached(self, mode) -> Run:
        if mode not in self._runs:
            self._runs[mode] = self.run(mode)
        return self._runs[mode]

    def state_after(self, count):
        """A fresh pool after the first `count` steps, run eagerly."""
        pool = self.new_pool()
        with torch.inference_mode():
            for st in self.steps[:count]:
                batch = S.build_batch(st, self.seqs, self.tables, self.pad)
                self.model.forward(batch.to(DEV), pool)
        return pool


@pytest.fixture(scope="module", params=CASES, ids=_case_id)
def case(request):
    assert torch.cuda.is_available()
    c = Case(*request.param)
    yield c
    del c
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# the script: replay vs fp64, vs eager, under NaN
# ---------------------------------------------------------------------------

def test_script_takes_the_buckets_it_claims(case):
    shape = [(st.replayed, st.n) for st in case.cached("replay").steps]
    T, F = True, False
    assert shape == [(F, 0), (F, 1), (T, 3), (T, 1), (T, 2), (T, 3), (F, 0),
                     (T, 12), (T, 12), (F, 0), (F, 18), (F, 0)]
    rows = {1: 1, 2: 2, 3: 4, 12: 16}
    for st in case.cached("replay").steps:
        if st.replayed:
            assert st.logits.shape[0] == rows[st.n]


def _fp64_failures(case, run: Run, tag: str) -> list:
    L = case.spec.num_layers
    worst: dict = {}
    failures = []
    for i, (st, got) in enumerate(zip(case.steps, run.steps)):
        if not got.replayed:
            continue
        e = S.reference_step(case.exact, st, L)
        r = S.reference_step(case.rounded, st, L)
        mine = {"logits": got.logits[: got.n].double()}
        for l in range(L):
            mine[f"k{l}"] = got.k[l].double().flatten(1)
            mine[f"v{l}"] = got.v[l].double().flatten(1)
        for key, x in mine.items():
            assert x.shape == e[key].shape, (i, key)
            assert bool(torch.isfinite(x).all()), (i, key)
            noise = S.noise_of(r[key], e[key])
            assert noise > 0, (i, key)
            err = S.row_rel_err(x, e[key])
            ratio = float(err.max()) / noise
            kind = S.kind_of(key)
            worst[kind] = max(worst.get(kind, 0.0), ratio)
            if not ratio <= MARGIN:
                failures.append((i, key, int(err.argmax()), f"{ratio:.2f}", f"{noise:.2e}"))
    print(f"RATIOS {tag} {case.id} "
          + " ".join(f"{k}={v:.2f}" for k, v in sorted(worst.items())))
    return failures


def _expert_histograms(case, decode, B) -> list:
    """Per layer, how many rows of a bucket of width B each expert gets,
    pad rows (token 0 at position 0) included, from the exact reference's
    router. decode = [] is the capture: every row is a pad row."""
    k = case.spec.experts_per_token
    pad = dense_forward(case.model, [[0]])[0]["router_probs"]
    hists = []
    for l in range(case.spec.num_layers):
        rows = [case.exact[n]["router_probs"][l][p] for n, p in decode]
        rows += [pad[l][0]] * (B - len(rows))
        chosen = torch.topk(torch.stack(rows), k, dim=-1).indices.flatten()
        hists.append(torch.bincount(chosen, minlength=case.spec.num_experts).tolist())
    return hists


def test_replay_matches_dense_fp64_reference(case):
    if case.spec.arch == "mixtral":
        # otherwise the test proves nothing about capture-frozen routing
        assert S.min_routing_gap(list(case.exact.values())) >= S.ROUTING_GAP
        capture = _expert_histograms(case, [], 4)
        bucket4 = [_expert_histograms(case, st.decode, 4) for st in case.steps
                   if not st.prefill and len(st.decode) == 3]
        assert len(bucket4) == 2
        assert bucket4[0] != bucket4[1], bucket4
        for l in range(case.spec.num_layers):  # a frozen grid shows per layer
            assert bucket4[0][l] != capture[l], (l, capture[l])
            assert bucket4[1][l] != capture[l], (l, capture[l])
        experts = [
            [sorted(torch.topk(case.exact[n]["router_probs"][l][p],
                               case.spec.experts_per_token).indices.tolist())
             for l in range(case.spec.num_layers) for n, p in st.decode]
            for st in case.steps if not st.prefill and len(st.decode) == 3
        ]
        assert experts[0] != experts[1], experts
    failures = _fp64_failures(case, case.cached("replay"), "replay")
    assert not failures, failures[:12]


def _assert_runs_equal(a: Run, b: Run, what):
    assert len(a.steps) == len(b.steps)
    for i, (x, y) in enumerate(zip(a.steps, b.steps)):
        assert (x.replayed, x.n) == (y.replayed, y.n)
        assert torch.equal(x.logits, y.logits), (what, i, "logits")
        assert bool(torch.isfinite(x.logits[: max(x.n, 1)]).all()), (what, i)
        assert torch.equal(x.k, y.k) and torch.equal(x.v, y.v), (what, i, "kv")
    assert torch.equal(a.written, b.written)
    assert torch.equal(a.bits, b.bits), (what, "pool bytes")


def test_replay_equals_eager_forward_of_the_padded_batch(case):
    _assert_runs_equal(case.cached("replay"), case.cached("wide"), "replay vs eager")


def test_static_table_width_changes_no_arithmetic(case):
    _assert_runs_equal(case.cached("tight"), case.cached("wide"), "tight vs wide")


def test_nan_poisoned_pool_changes_nothing(case):
    """The warm-up forwards and the capture run on the default statics, on
    a pool that is NaN everywhere: they may touch the scratch block only."""
    poisoned = case.run("replay", nan_fill=True)
    base = case.cached("replay")
    ref_pool = case.new_pool(nan_fill=True)
    fill = pool_bytes(ref_pool, case.scratch)
    unwritten = ~base.written
    unwritten[case.scratch * BS : (case.scratch + 1) * BS] = False
    assert int(unwritten.sum()) > 0
    assert torch.equal(slots_of(poisoned.bits, unwritten), slots_of(fill, unwritten))
    # what the script wrote equals the unpoisoned run, byte for byte
    assert torch.equal(slots_of(poisoned.bits, base.written),
                       slots_of(base.bits, base.written))
    for i, (x, y) in enumerate(zip(poisoned.steps, base.steps)):
        rows = x.n if x.replayed else x.logits.shape[0]
        assert bool(torch.isfinite(x.logits[:rows]).all()), i
        assert torch.equal(x.logits[:rows], y.logits[:rows]), i
        assert torch.equal(x.k, y.k) and torch.equal(x.v, y.v), i


# ---------------------------------------------------------------------------
# staleness, interleaving, scales
# ---------------------------------------------------------------------------

def _after_shorts(case):
    """Index of the first M=12 step and the pool state in front of it."""
    at = next(i for i, st in enumerate(case.steps) if len(st.decode) == 12)
    pos = dict(case.steps[at].decode)
    assert (pos["B"], pos["A"], pos["C"], pos["S3"]) == (37, 73, 20, 3)
    return at, pos


def test_narrow_replay_after_wide_replay_of_the_same_bucket(case):
    at, pos = _after_shorts(case)
    pool = case.state_after(at)
    runner = case.new_runner(pool)
    wide = case.batch_of([("B", 37), ("C", 20), ("S3", 3), ("A", 73)])
    narrow = case.batch_of([("B", 38), ("C", 21), ("S3", 4)])
    assert wide.decode_block_tables.shape[1] == 5 > narrow.decode_block_tables.shape[1]
    with torch.inference_mode():
        runner.run(wide)
        torch.cuda.synchronize()
        # whatever row 3 would still write or read now is visible: NaN in
        # all of A's blocks
        for b in case.tables["A"]:
            for t in (pool.k, pool.v):
                if t.dtype == torch.float8_e4m3fn:
                    t.view(torch.uint8)[:, b].fill_(0x7F)
                else:
                    t[:, b].fill_(float("nan"))
        before = snapshot(pool)
        bits_before = pool_bytes(pool)
        got = runner.run(narrow).float().cpu().clone()
        bits_after = pool_bytes(pool)
        a_blocks = torch.tensor(case.tables["A"])
        assert torch.equal(bits_after[:, :, a_blocks], bits_before[:, :, a_blocks])
        entry = runner._graphs[4]
        want = case.padded(narrow, 4)
        for key, exp in G.statics_of(want).items():
            assert torch.equal(entry["static"][key].cpu(), exp), key
        restore_(pool, before)
        fresh = case.new_runner(pool)
        ref = fresh.run(narrow).float().cpu().clone()
    assert got.shape[0] == 3 and bool(torch.isfinite(got).all())
    assert torch.equal(got, ref)
    changed = (bits_after != bits_before).any(dim=0).any(dim=0).any(dim=1).any(dim=-1)
    changed[case.scratch] = False  # [blocks, 16]
    want_slots = torch.zeros(S.NUM_BLOCKS * BS, dtype=torch.bool)
    want_slots[narrow.slot_mapping] = True
    assert torch.equal(changed.reshape(-1), want_slots)


def test_replay_survives_other_bucket_and_eager_call(case):
    at, pos = _after_shorts(case)
    pool = case.state_after(at)
    other = case.state_after(at)
    start = snapshot(pool)
    runner = case.new_runner(pool)
    # not the row order of the M=12 step: bucket 16's output buffer never
    # holds these logits in its first rows
    x = case.batch_of([("A", 73), ("C", 20), ("B", 37)])
    with torch.inference_mode():
        first = runner.run(x).float().cpu().clone()
        kv_first = S.read_slots(pool, x.slot_mapping, raw=True)
        bits_first = pool_bytes(pool, case.scratch)
        # bucket 16 is captured now, into the pool bucket 4 already uses
        assert sorted(runner._graphs) == [4]
        twelve = S.build_batch(case.steps[at], case.seqs, case.tables, case.pad)
        out16 = runner.run(twelve)
        assert sorted(runner._graphs) == [4, 16] and runner._pool is not None
        assert bool(torch.isfinite(out16).all())
        # same shape as bucket 4: shares its decode-attention workspace
        y = case.batch_of([("S4", 4), ("S5", 5), ("S6", 6), ("S7", 7)])
        eager = case.model.forward(case.padded(y, 4).to(DEV), other)
        assert bool(torch.isfinite(eager).all())
        restore_(pool, start)
        again = runner.run(x).float().cpu().clone()
        kv_again = S.read_slots(pool, x.slot_mapping, raw=True)
        bits_again = pool_bytes(pool, case.scratch)
    assert bool(torch.isfinite(first).all())
    assert torch.equal(again, first)
    assert torch.equal(kv_again[0], kv_first[0]) and torch.equal(kv_again[1], kv_first[1])
    assert torch.equal(bits_again, bits_first)


def test_kv_scales_set_after_capture_are_used_by_replays():
    """A graph that captured the scale's value, not its pointer, computes
    with scales of 1.0 and fails both rules."""
    c = Case(*KV_CASE)
    assert bool((c.scales != 1).any())
    late = c.run("replay", late_scales=True)
    failures = _fp64_failures(c, late, "late-scales")
    assert not failures, failures[:12]
    _assert_runs_equal(late, c.cached("wide"), "late scales vs eager")


# ---------------------------------------------------------------------------
# ChainRunner statics
# ---------------------------------------------------------------------------

def _chain_batch(tokens, state, rows, pad, n=3) -> ForwardBatch:
    w = max(len(t) for t in rows[:n])
    return ForwardBatch(
        token_ids=torch.tensor(tokens, dtype=torch.long),
        positions=torch.tensor(state["positions"][:n], dtype=torch.long),
        slot_mapping=torch.tensor(state["slots"][:n], dtype=torch.long),
        num_decode_seqs=n,
        decode_block_tables=torch.tensor(
            [(t + [pad] * w)[:w] for t in rows[:n]], dtype=torch.int32
        ),
        decode_kv_lens=torch.tensor(state["kv_lens"][:n], dtype=torch.int32),
        sample_indices=torch.arange(n, dtype=torch.long),
    )


class ChainScene:
    def __init__(self, case, params):
        self.case = case
        self.params = params
        self.tables, self.pad, self.scratch = G.chain_layout()
        self.positions, self.rows = G.chain_start(self.tables, self.scratch)
        self.states = G.chain_expected(self.positions, self.rows, G.CHAIN_STEPS, BS)
        self.first_tokens = [case.seqs[n][l] for n, l in G.CHAIN_ROWS]
        self.prefill_slots = [
            self.tables[n][p // BS] * BS + p % BS for n, l in G.CHAIN_ROWS for p in range(l)
        ]

    def prefilled_pool(self):
        pool = self.case.new_pool(nan_fill=True)
        with torch.inference_mode():
            for name, length in G.CHAIN_ROWS:
                b = ForwardBatch.single_prefill(
                    self.case.seqs[name][:length], self.tables[name], BS
                )
                self.case.model.forward(b.to(DEV), pool)
        return pool

    def batch(self, tokens, k):
        return _chain_batch(tokens, self.states[k], self.rows, self.pad)

    def chained(self):
        """Side A. Returns tokens per step, the logits of step 1, the
        statics after the last step, the pool and the chain objects."""
        pool = self.prefilled_pool()
        runner = self.case.new_runner(pool, self.scratch)
        chain = ChainRunner(runner, DEV)
        seqs = [SimpleNamespace(params=p) for p in self.params]
        with torch.inference_mode():
            ctx = chain.prepare(self.batch(self.first_tokens, 0), seqs)
            first_logits = None
            for i in range(G.CHAIN_STEPS):
                chain.launch_step(ctx, i)
                if i == 0:
                    first_logits = ctx["entry"]["logits"].clone()
            chain.wait_step(G.CHAIN_STEPS - 1)
            torch.cuda.synchronize()
        tokens = [chain.tokens_of(ctx, i) for i in range(G.CHAIN_STEPS)]
        statics = {k: ctx["entry"]["static"][k].cpu().clone() for k in G.STATIC_KEYS}
        return tokens, first_logits.float().cpu(), statics, pool, chain, ctx

    def stepped(self):
        """Side B: the same steps built on the host from chain_expected."""
        pool = self.prefilled_pool()
        runner = self.case.new_runner(pool, self.scratch)
        B = 4
        temps = torch.zeros(B)
        tops = torch.ones(B)
        bases = torch.zeros(B, dtype=torch.long)
        for i, p in enumerate(self.params):
            temps[i], tops[i] = p.temperature, p.top_p
            bases[i] = 0 if p.seed is None else int(p.seed)
        temps, tops, bases = temps.to(DEV), tops.to(DEV), bases.to(DEV)
        seeds = torch.zeros(B, dtype=torch.long, device=DEV)
        out = torch.zeros(B, dtype=torch.long, device=DEV)
        toks = list(self.first_tokens)
        tokens = []
        with torch.inference_mode():
            for k in range(G.CHAIN_STEPS):
                runner.run(self.batch(toks, k))
                logits = runner._graphs[B]["logits"]
                host_pos = self.states[k]["positions"][:3] + [0]
                ops.derive_seeds(
                    seeds, bases, torch.tensor(host_pos, dtype=torch.long, device=DEV)
                )
                ops.top_p_sample(logits, temps, tops, seeds=seeds, out=out)
                toks = out[:3].tolist()
                tokens.append(toks)
        torch.cuda.synchronize()
        return tokens, pool


GREEDY = [SamplingParams(temperature=0.0, top_p=1.0) for _ in range(3)]


def test_chain_statics_tokens_and_cache_bytes(case):
    scene = ChainScene(case, GREEDY)
    tok_a, first_logits, statics, pool_a, chain, ctx = scene.chained()
    tok_b, pool_b = scene.stepped()
    assert tok_a == tok_b
    final = scene.states[G.CHAIN_STEPS]
    assert statics["positions"].tolist() == final["positions"]
    assert statics["kv_lens"].tolist() == final["kv_lens"]
    assert statics["slot_mapping"].tolist() == final["slots"]
    assert statics["token_ids"][:3].tolist() == tok_a[-1]
    assert statics["positions"][3].item() == G.CHAIN_STEPS
    assert statics["kv_lens"][3].item() == G.CHAIN_STEPS + 1
    lo, hi = scene.scratch * BS, (scene.scratch + 1) * BS
    assert all(lo <= st["slots"][3] < hi for st in scene.states)
    assert lo <= int(statics["slot_mapping"][3]) < hi

    bits_a, bits_b = pool_bytes(pool_a, scene.scratch), pool_bytes(pool_b, scene.scratch)
    assert torch.equal(bits_a, bits_b)
    written = torch.zeros(S.NUM_BLOCKS * BS, dtype=torch.bool)
    written[torch.tensor(scene.prefill_slots)] = True
    for st in scene.states[: G.CHAIN_STEPS]:
        written[torch.tensor(st["slots"][:3])] = True
    fill = pool_bytes(case.new_pool(nan_fill=True), scene.scratch)
    untouched = (slots_of(bits_a, torch.ones_like(written))
                 == slots_of(fill, torch.ones_like(written))).all(dim=1)
    untouched[lo:hi] = False
    outside = torch.ones_like(written)
    outside[lo:hi] = False
    # a written slot is never left at the fill pattern; everything else is
    assert torch.equal(~untouched & outside, written)
    # the pad row wrapped: it wrote all 16 slots of the scratch block
    scratch_bits = slots_of(pool_bytes(pool_a), ~outside)
    fill_bits = slots_of(pool_bytes(case.new_pool(nan_fill=True)), ~outside)
    assert bool((scratch_bits != fill_bits).any(dim=1).all())

    # step 1 against fp64: a dense reference of the three prompts + 1 token
    seqs = [case.seqs[n][: l + 1] for n, l in G.CHAIN_ROWS]
    masks = [torch.arange(l + 1) < l for _, l in G.CHAIN_ROWS]
    exact = dense_forward(case.model, seqs, prefill_masks=masks)
    rounded = dense_forward(case.model, seqs, mode=torch.bfloat16,
                            kv_scales=case.scales, prefill_masks=masks)
    e = torch.stack([r["logits"][-1] for r in exact])
    r = torch.stack([r["logits"][-1] for r in rounded])
    noise = S.noise_of(r, e)
    assert noise > 0
    ratio = float(S.row_rel_err(first_logits[:3].double(), e).max()) / noise
    print(f"RATIOS chain {case.id} logits={ratio:.2f}")
    assert ratio <= MARGIN, ratio

    # a second prepare puts every static back, pad rows at position 0
    fresh = scene.batch(tok_a[-1], G.CHAIN_STEPS)
    with torch.inference_mode():
        ctx2 = chain.prepare(fresh, [SimpleNamespace(params=p) for p in GREEDY])
        torch.cuda.synchronize()
    want = G.padded_decode_batch(fresh, 4, scene.scratch, G.MAX_BLOCKS, BS)
    for key, exp in G.statics_of(want).items():
        assert torch.equal(ctx2["entry"]["static"][key].cpu(), exp), key
    assert ctx2["entry"]["static"]["positions"][3].item() == 0


def test_chain_with_a_seeded_row_matches_host_stepping(case):
    params = [
        SamplingParams(temperature=0.0, top_p=1.0),
        SamplingParams(temperature=0.8, top_p=0.95, seed=4242),
        SamplingParams(temperature=0.0, top_p=1.0),
    ]
    scene = ChainScene(case, params)
    tok_a = scene.chained()[0]
    tok_b, _ = scene.stepped()
    assert tok_a == tok_b
