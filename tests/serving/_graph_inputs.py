"""What a captured decode graph must be fed, written from the contract in
the module docstring of ``dts_amd/serving/graph_runner.py`` and from the
chain's slot rule, not from the code that fills the statics.

The contract: a bucket of width ``B`` sees the ``n <= B`` rows of a decode
batch unchanged; rows ``n..B-1`` are pad rows that decode token 0 at
position 0, write its K/V to slot 0 of a reserved scratch block and attend
one key of that block. Every block table is ``max_blocks`` wide, and a
column a row does not own names the scratch block. Logits are computed for
all ``B`` rows.

The chain rule: between two replays every row, pad rows included, moves one
position on: ``position += 1``, ``kv_len += 1``,
``slot = table[position // block_size] * block_size + position % block_size``.
"""

from __future__ import annotations

import torch

from dts_amd.serving.batch import ForwardBatch

STATIC_KEYS = ("token_ids", "positions", "slot_mapping", "block_tables", "kv_lens")

MAX_BUCKET = 16
MAX_BLOCKS = 8  # width of the static block tables in these tests

# The chain scenario: (sequence of tests/models/_scenarios.py, prompt
# length). The first decode positions are the last slot of a block (15),
# the first slot of a fresh block (16) and the 64 -> 65 key boundary of the
# decode kernel's tiles (63). Bucket 4, so one pad row.
CHAIN_ROWS = (("C", 15), ("B", 16), ("A", 63))
CHAIN_STEPS = 20


def graph_script_steps() -> list:
    """script_steps() of the model tests with the second M=3 decode step
    split into its row subsets {B} and {A, C}: n = 1 is bucket 1 (no pad
    row, the M = 1 dispatch branch), n = 2 fills bucket 2 exactly. Both
    halves together write what the scripted step wrote, so every later
    step and every teacher-forced token stays as it is. Decode-only steps
    sample every row (the captured graph always does)."""
    from tests.models import _scenarios as S

    out = []
    for i, st in enumerate(S.script_steps()):
        if st.prefill:
            out.append(st)
        elif i == 3:
            assert [n for n, _ in st.decode] == ["B", "A", "C"]
            out.append(S.Step(decode=st.decode[:1]))
            out.append(S.Step(decode=st.decode[1:]))
        else:
            out.append(S.Step(decode=list(st.decode)))
    return out


def chain_layout(shuffle_seed: int = 11) -> tuple:
    """({name: [blocks]} covering prompt + CHAIN_STEPS + 1 tokens, pad
    block, scratch block) out of the scenario pool's NUM_BLOCKS."""
    from tests.models import _scenarios as S

    g = torch.Generator().manual_seed(shuffle_seed)
    ids = torch.randperm(S.NUM_BLOCKS, generator=g).tolist()
    tables, at = {}, 0
    for name, length in CHAIN_ROWS:
        nb = -(-(length + CHAIN_STEPS + 1) // S.BLOCK_SIZE)
        tables[name] = ids[at : at + nb]
        at += nb
    return tables, ids[at], ids[at + 1]


def chain_start(tables: dict, scratch_block: int, B: int = 4) -> tuple:
    """(start positions, per-row tables) of all B rows, pad rows included."""
    positions = [length for _, length in CHAIN_ROWS]
    rows = [list(tables[name]) for name, _ in CHAIN_ROWS]
    while len(positions) < B:
        positions.append(0)
        rows.append([scratch_block] * MAX_BLOCKS)
    return positions, rows


def padded_decode_batch(batch: ForwardBatch, B: int, scratch_block: int,
                        max_blocks: int, block_size: int) -> ForwardBatch:
    """The ForwardBatch a bucket of width B must see for a decode-only
    `batch` of n <= B rows (CPU tensors)."""
    n = batch.num_decode_seqs
    assert batch.num_prefill_seqs == 0 and 0 < n <= B
    width = batch.decode_block_tables.shape[1]
    assert width <= max_blocks
    tok, pos, slots, kvl, rows = [], [], [], [], []
    for i in range(B):
        if i < n:
            tok.append(int(batch.token_ids[i]))
            pos.append(int(batch.positions[i]))
            slots.append(int(batch.slot_mapping[i]))
            kvl.append(int(batch.decode_kv_lens[i]))
            own = [int(b) for b in batch.decode_block_tables[i]]
            rows.append(own + [scratch_block] * (max_blocks - width))
        else:  # pad row: token 0 at position 0 of the scratch block
            tok.append(0)
            pos.append(0)
            slots.append(scratch_block * block_size)
            kvl.append(1)
            rows.append([scratch_block] * max_blocks)
    return ForwardBatch(
        token_ids=torch.tensor(tok, dtype=torch.long),
        positions=torch.tensor(pos, dtype=torch.long),
        slot_mapping=torch.tensor(slots, dtype=torch.long),
        num_decode_seqs=B,
        decode_block_tables=torch.tensor(rows, dtype=torch.int32),
        decode_kv_lens=torch.tensor(kvl, dtype=torch.int32),
        sample_indices=torch.arange(B, dtype=torch.long),
    )


def statics_of(batch: ForwardBatch) -> dict:
    """A padded batch keyed like a graph entry's statics."""
    return {
        "token_ids": batch.token_ids,
        "positions": batch.positions,
        "slot_mapping": batch.slot_mapping,
        "block_tables": batch.decode_block_tables,
        "kv_lens": batch.decode_kv_lens,
    }


def chain_expected(positions: list, tables: list, steps: int,
                   block_size: int) -> list:
    """``steps + 1`` states of a chain over rows that start at `positions`
    with block tables `tables` (pad rows included: position 0, a table of
    scratch blocks). State k is what the statics hold after k chained
    steps, i.e. what replay k + 1 reads; state 0 is the start. Each state:
    ``{"positions": [...], "kv_lens": [...], "slots": [...]}``. A table
    column that does not exist raises IndexError."""
    states = []
    for k in range(steps + 1):
        pos = [p + k for p in positions]
        states.append(
            {
                "positions": pos,
                "kv_lens": [p + 1 for p in pos],
                "slots": [
                    tables[r][p // block_size] * block_size + p % block_size
                    for r, p in enumerate(pos)
                ],
            }
        )
    return states
