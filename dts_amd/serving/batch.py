"""Flattened forward-batch metadata shared by scheduler and models.

One engine step runs ONE model forward over a flat token batch that mixes
prefill chunks and decode tokens (token-level continuous batching,
SURVEY.md §2.3 "Continuous-batching scheduler"). Prefill tokens come first,
then one decode token per running sequence.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class ForwardBatch:
    # flat inputs [T]
    token_ids: torch.Tensor
    positions: torch.Tensor
    slot_mapping: torch.Tensor  # flat cache slot per token
    # prefill section (first sum(q_lens) tokens of the batch)
    num_prefill_seqs: int = 0
    num_prefill_tokens: int = 0
    cu_q: Optional[torch.Tensor] = None  # [P+1] int32
    prefill_block_tables: Optional[torch.Tensor] = None  # [P, max_blocks]
    prefill_kv_lens: Optional[torch.Tensor] = None  # [P]
    # decode section
    num_decode_seqs: int = 0
    decode_block_tables: Optional[torch.Tensor] = None  # [D, max_blocks]
    decode_kv_lens: Optional[torch.Tensor] = None  # [D]
    # rows of the flat batch to compute logits for (last token of each
    # prefill chunk that completed its prompt + every decode token)
    sample_indices: Optional[torch.Tensor] = None

    @classmethod
    def single_prefill(
        cls, token_ids: list, block_table: list, block_size: int, start: int = 0
    ) -> "ForwardBatch":
        """One sequence's prefill chunk `token_ids` at positions start..,
        written to and attending over the blocks of `block_table`; logits
        for the chunk's last token."""
        n = len(token_ids)
        pos = torch.arange(start, start + n, dtype=torch.long)
        table = torch.tensor(block_table, dtype=torch.long)
        slots = table[pos // block_size] * block_size + pos % block_size
        return cls(
            token_ids=torch.tensor(token_ids, dtype=torch.long),
            positions=pos,
            slot_mapping=slots,
            num_prefill_seqs=1,
            num_prefill_tokens=n,
            cu_q=torch.tensor([0, n], dtype=torch.int32),
            prefill_block_tables=table.to(torch.int32).unsqueeze(0),
            prefill_kv_lens=torch.tensor([start + n], dtype=torch.int32),
            sample_indices=torch.tensor([n - 1], dtype=torch.long),
        )

    @property
    def num_tokens(self) -> int:
        return int(self.token_ids.shape[0])

    def to(self, device) -> "ForwardBatch":
        def mv(t):
            return t.to(device, non_blocking=True) if t is not None else None

        return ForwardBatch(
            token_ids=mv(self.token_ids),
            positions=mv(self.positions),
            slot_mapping=mv(self.slot_mapping),
            num_prefill_seqs=self.num_prefill_seqs,
            num_prefill_tokens=self.num_prefill_tokens,
            cu_q=mv(self.cu_q),
            prefill_block_tables=mv(self.prefill_block_tables),
            prefill_kv_lens=mv(self.prefill_kv_lens),
            num_decode_seqs=self.num_decode_seqs,
            decode_block_tables=mv(self.decode_block_tables),
            decode_kv_lens=mv(self.decode_kv_lens),
            sample_indices=mv(self.sample_indices),
        )
