"""The graph-input helpers of _graph_inputs.py, proven without a GPU:
DecodeGraphRunner.load_batch must fill an entry's statics exactly as
padded_decode_batch says, also over a fuller earlier load, and the chain
scenario of test_graph_replay_gpu.py must cross what it claims to cross."""

import pytest
import torch

from dts_amd.serving.graph_runner import DecodeGraphRunner
from tests.models import _scenarios as S
from tests.serving import _graph_inputs as G

TABLES, SPARE = S.block_tables(11)
PAD, SCRATCH = SPARE[0], SPARE[1]  # as the GPU tests take them


class FakePool:
    block_size = S.BLOCK_SIZE


def make_runner():
    return DecodeGraphRunner(
        model=None, kv_pool=FakePool(), device="cpu", scratch_block=SCRATCH,
        max_blocks_per_seq=G.MAX_BLOCKS, max_bucket=G.MAX_BUCKET,
    )


def garbage_entry(B):
    """Statics as an earlier, unrelated replay might have left them."""
    return {
        "static": {
            "token_ids": torch.full((B,), 777, dtype=torch.long),
            "positions": torch.full((B,), 55, dtype=torch.long),
            "slot_mapping": torch.full((B,), 3, dtype=torch.long),
            "block_tables": torch.full((B, G.MAX_BLOCKS), 1, dtype=torch.int32),
            "kv_lens": torch.full((B,), 56, dtype=torch.int32),
            "sample_indices": torch.arange(B, dtype=torch.long),
        }
    }


def scripted_batch(decode):
    seqs = S.sequences_for(S.SPECS["llama-g4-d128"])
    return S.build_batch(S.Step(decode=decode), seqs, TABLES, PAD)


def assert_statics(entry, want):
    for key, exp in G.statics_of(want).items():
        got = entry["static"][key]
        assert got.dtype == exp.dtype and torch.equal(got, exp), key


DECODES = {
    "n1-b1": [("B", 35)],
    "n2-b2": [("A", 71), ("C", 18)],
    "n3-b4": [("B", 34), ("A", 70), ("C", 17)],
    "n4-b4": [("B", 36), ("A", 72), ("C", 19), ("S5", 5)],
    "n12-b16": [("B", 37), ("A", 73), ("C", 20)] + [(f"S{n}", n) for n in range(3, 12)],
    "n16-b16": [("B", 37), ("A", 73), ("C", 20)] + [(f"S{n}", n) for n in range(3, 12)]
    + [(f"X{i}", 1) for i in range(4)],
}


@pytest.mark.parametrize("name", list(DECODES))
def test_load_batch_equals_padded_decode_batch(name):
    batch = scripted_batch(DECODES[name])
    n = batch.num_decode_seqs
    r = make_runner()
    assert r.can_run(batch)
    B = r._bucket_for(n)
    assert f"n{n}-b{B}" == name
    entry = garbage_entry(B)
    r.load_batch(entry, batch)
    want = G.padded_decode_batch(batch, B, SCRATCH, G.MAX_BLOCKS, S.BLOCK_SIZE)
    assert want.num_decode_seqs == B and want.num_prefill_seqs == 0
    assert torch.equal(want.sample_indices, entry["static"]["sample_indices"])
    assert_statics(entry, want)
    # the helper itself: real rows untouched, pad rows on the scratch block
    assert torch.equal(want.token_ids[:n], batch.token_ids)
    assert torch.equal(want.slot_mapping[:n], batch.slot_mapping)
    w = batch.decode_block_tables.shape[1]
    assert torch.equal(want.decode_block_tables[:n, :w], batch.decode_block_tables)
    assert bool((want.decode_block_tables[:n, w:] == SCRATCH).all())
    assert bool((want.decode_block_tables[n:] == SCRATCH).all())
    assert want.slot_mapping[n:].tolist() == [SCRATCH * S.BLOCK_SIZE] * (B - n)
    assert want.decode_kv_lens[n:].tolist() == [1] * (B - n)
    assert want.token_ids[n:].tolist() == [0] * (B - n)
    assert want.positions[n:].tolist() == [0] * (B - n)


def test_narrow_load_after_wide_load_resets_row_and_columns():
    wide = scripted_batch([("B", 36), ("C", 19), ("S5", 5), ("A", 72)])
    narrow = scripted_batch([("S3", 3), ("S4", 4), ("S5", 6)])
    assert wide.decode_block_tables.shape[1] == 5
    assert narrow.decode_block_tables.shape[1] == 1
    r = make_runner()
    entry = garbage_entry(4)
    r.load_batch(entry, wide)
    assert_statics(entry, G.padded_decode_batch(wide, 4, SCRATCH, G.MAX_BLOCKS, 16))
    assert int(entry["static"]["kv_lens"][3]) == 73
    r.load_batch(entry, narrow)
    assert_statics(entry, G.padded_decode_batch(narrow, 4, SCRATCH, G.MAX_BLOCKS, 16))
    st = entry["static"]
    assert bool((st["block_tables"][3] == SCRATCH).all())
    assert bool((st["block_tables"][:, 1:] == SCRATCH).all())
    assert (int(st["token_ids"][3]), int(st["positions"][3]),
            int(st["kv_lens"][3])) == (0, 0, 1)
    assert int(st["slot_mapping"][3]) == SCRATCH * 16


def test_chain_scenario_crosses_what_it_claims():
    bs = S.BLOCK_SIZE
    tables, pad, scratch = G.chain_layout()
    owned = [b for t in tables.values() for b in t]
    assert len(set(owned + [pad, scratch])) == len(owned) + 2
    assert max(owned + [pad, scratch]) < S.NUM_BLOCKS
    seqs = S.sequences_for(S.SPECS["llama-g4-d128"])
    for name, length in G.CHAIN_ROWS:  # one teacher-forced token past the prompt
        assert len(seqs[name]) > length
        assert len(S.MIXTRAL_SEQUENCES[name]) > length
    positions, rows = G.chain_start(tables, scratch)
    assert positions == [15, 16, 63, 0]
    assert all(len(t) <= G.MAX_BLOCKS for t in rows)
    # raises IndexError if a state indexed a column a table does not have
    states = G.chain_expected(positions, rows, G.CHAIN_STEPS, bs)
    assert len(states) == G.CHAIN_STEPS + 1
    assert states[0]["slots"][:3] == [
        tables["C"][0] * bs + 15, tables["B"][1] * bs, tables["A"][3] * bs + 15
    ]
    crossing = 0
    for r in range(3):
        blocks = {st["positions"][r] // bs for st in states}
        assert max(blocks) < len(rows[r]) <= G.MAX_BLOCKS
        crossing += len(blocks) >= 2
        slots = [st["slots"][r] for st in states]
        assert len(set(slots)) == len(slots)
        assert all(s // bs in tables[G.CHAIN_ROWS[r][0]] for s in slots)
    assert crossing >= 2
    # 64 -> 65 keys for the row that starts at position 63
    assert [st["kv_lens"][2] for st in states[:2]] == [64, 65]
    # the pad row wraps inside the scratch block and reads a second column
    pad_states = [(st["positions"][3], st["kv_lens"][3], st["slots"][3]) for st in states]
    assert pad_states[0] == (0, 1, scratch * bs)
    assert pad_states[16] == (16, 17, scratch * bs)
    assert pad_states[-1] == (20, 21, scratch * bs + 4)
    assert all(s // bs == scratch for _, _, s in pad_states)
    assert max(p // bs for p, _, _ in pad_states) == 1 < G.MAX_BLOCKS
    # no two rows ever write the same slot
    for st in states:
        assert len(set(st["slots"])) == 4
