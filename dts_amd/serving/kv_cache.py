"""Paged KV cache: block pool + prefix-sharing block manager.

This is the MI355X-native replacement for the reference's remote-API
statelessness (SURVEY.md §2.3 "Paged KV-block manager with shared-prefix
refcounting / copy-on-write"): tree branches forked from one node share
their conversation prefix (ref tree.py:59-65 lineage), sibling rollouts and
repeated per-turn prompts reuse prefill, and identical judge prompts (3
judges per trajectory, ref evaluator.py:171-172) prefill once.

Mechanism: fixed-size token blocks; full blocks are content-addressed by a
chain hash (hash of parent-hash + the block's token ids) and refcounted.
  - allocate(prompt): longest-prefix match against the hash table — hit
    blocks are shared (ref++), only the tail is scheduled for prefill;
  - fork(): child shares all full blocks, copy-on-write of the partial
    tail block (the only mutable block);
  - free(): ref--; zero-ref hashed blocks stay cached in an LRU pool and
    are evicted only when allocation runs dry.

Cache layout (per layer): K and V each [num_blocks, n_kv_heads,
block_size, head_dim] — one (block, kv-head) is a contiguous
[block_size, head_dim] tile (16x128 bf16 = 4 KiB), the unit the CDNA4
decode-attention kernel streams through LDS.

An FP8 (e4m3) pool also owns static power-of-two scales, fp32 [layers, 2
(K, V), kv_heads]: a cached value is code * scale. Scales never change
once a block holds data, so copy_block and the prefix cache ignore them.
"""

from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional

import torch

DEFAULT_BLOCK_SIZE = 16

FP8_E4M3_MAX = 448.0
KV_SCALE_MIN_EXP = -20
KV_SCALE_MAX_EXP = 20


def pow2_ceil_scales(values: torch.Tensor) -> torch.Tensor:
    """Round positive finite fp32 values UP to the next power of two,
    clamped to [2^-20, 2^20] (a power of two maps to itself). frexp gives
    the exponent exactly — no log2 rounding at the boundaries, the
    construction quantize_fp8_rowwise uses for weights."""
    v = torch.as_tensor(values, dtype=torch.float32)
    if not bool(torch.isfinite(v).all()) or not bool((v > 0).all()):
        raise ValueError("KV scales must be positive and finite")
    mant, exp = torch.frexp(v)  # v = mant * 2^exp, mant in [0.5, 1)
    exp = torch.where(mant == 0.5, exp - 1, exp)
    exp = exp.clamp(KV_SCALE_MIN_EXP, KV_SCALE_MAX_EXP)
    return torch.ldexp(torch.ones_like(v), exp)


def scales_from_amax(amax: torch.Tensor, headroom: float = 2.0) -> torch.Tensor:
    """scale = 2^ceil(log2(headroom * amax / 448)); amax = 0 gives 1.0."""
    a = torch.as_tensor(amax, dtype=torch.float32)
    target = a * (float(headroom) / FP8_E4M3_MAX)
    ok = target > 0
    scales = pow2_ceil_scales(torch.where(ok, target, torch.ones_like(target)))
    return torch.where(ok, scales, torch.ones_like(scales))


def unpack_kv_layer(kv_layer: tuple) -> tuple:
    """(k_cache, v_cache, kv_scale, observe) from KVCachePool.layer(i) or
    from a hand-built (k_cache, v_cache): the last two default to None."""
    n = len(kv_layer)
    return (
        kv_layer[0],
        kv_layer[1],
        kv_layer[2] if n > 2 else None,
        kv_layer[3] if n > 3 else None,
    )


def chain_hash(prev_hash: int, tokens: tuple) -> int:
    return hash((prev_hash, tokens))


@dataclass
class Block:
    id: int
    ref_count: int = 0
    hash: Optional[int] = None  # set once full + registered
    token_ids: tuple = ()  # content of a full registered block (for verify)


class BlockManager:
    """Refcounted block allocator with content-addressed prefix cache."""

    def __init__(self, num_blocks: int, block_size: int = DEFAULT_BLOCK_SIZE) -> None:
        self.num_blocks = num_blocks
        self.block_size = block_size
        self.blocks = [Block(i) for i in range(num_blocks)]
        self.free_ids = list(range(num_blocks - 1, -1, -1))  # pop() -> low ids first
        self.hash_table: dict = {}  # hash -> block_id
        self.evictable: OrderedDict = OrderedDict()  # block_id -> None (LRU)
        # stats
        self.cache_hit_tokens = 0
        self.cache_miss_tokens = 0

    # -- allocation core ------------------------------------------------
    def num_free(self) -> int:
        return len(self.free_ids) + len(self.evictable)

    def _pop_free_block(self) -> Block:
        if self.free_ids:
            return self.blocks[self.free_ids.pop()]
        if self.evictable:
            bid, _ = self.evictable.popitem(last=False)  # LRU
            block = self.blocks[bid]
            if block.hash is not None and self.hash_table.get(block.hash) == bid:
                del self.hash_table[block.hash]
            block.hash = None
            block.token_ids = ()
            return block
        raise MemoryError("KV block pool exhausted")

    def _acquire(self, block: Block) -> None:
        if block.ref_count == 0 and block.id in self.evictable:
            del self.evictable[block.id]
        block.ref_count += 1

    def allocate_fresh(self) -> int:
        block = self._pop_free_block()
        block.ref_count = 1
        return block.id

    def free_block(self, block_id: int) -> None:
        block = self.blocks[block_id]
        assert block.ref_count > 0, "double free"
        block.ref_count -= 1
        if block.ref_count == 0:
            if block.hash is not None:
                self.evictable[block.id] = None  # keep cached, evict LRU
            else:
                self.free_ids.append(block.id)

    # -- prefix cache ----------------------------------------------------
    def match_prefix(self, tokens: list) -> tuple:
        """Longest cached prefix of `tokens` in full-block units.

        Returns (block_ids, n_matched_tokens); matched blocks are acquired.
        """
        matched: list = []
        prev = 0
        n = 0
        for start in range(0, len(tokens) - self.block_size + 1, self.block_size):
            chunk = tuple(tokens[start : start + self.block_size])
            h = chain_hash(prev, chunk)
            bid = self.hash_table.get(h)
            if bid is None or self.blocks[bid].token_ids != chunk:
                break
            self._acquire(self.blocks[bid])
            matched.append(bid)
            prev = h
            n += self.block_size
        return matched, n

    def register_full_block(self, block_id: int, prev_hash: int, tokens: tuple) -> int:
        """Content-register a block that just became full; returns its hash."""
        block = self.blocks[block_id]
        h = chain_hash(prev_hash, tokens)
        block.hash = h
        block.token_ids = tokens
        # first writer wins; a duplicate block stays usable, just unshared
        self.hash_table.setdefault(h, block_id)
        return h


class KVCachePool:
    """Owns the cache tensors for every layer of one model replica."""

    def __init__(
        self,
        num_layers: int,
        num_kv_heads: int,
        head_dim: int,
        num_blocks: int,
        block_size: int = DEFAULT_BLOCK_SIZE,
        dtype: torch.dtype = torch.bfloat16,
        device: str = "cpu",
    ) -> None:
        self.block_size = block_size
        self.num_blocks = num_blocks
        shape = (num_layers, num_blocks, num_kv_heads, block_size, head_dim)
        self.k = torch.zeros(shape, dtype=dtype, device=device)
        self.v = torch.zeros(shape, dtype=dtype, device=device)
        # FP8 pool only: static scales, ones until set. The tensor is
        # allocated once and only ever updated in place, so the per-layer
        # views handed to the kernels (and captured graphs) stay valid.
        self.scales: Optional[torch.Tensor] = None
        if dtype == torch.float8_e4m3fn:
            self.scales = torch.ones(
                (num_layers, 2, num_kv_heads), dtype=torch.float32, device=device
            )
        # calibration only: amax [layers, 2, kv_heads] of what is appended
        self._observed: Optional[torch.Tensor] = None

    def layer(self, i: int) -> tuple:
        """(k, v) of layer i; an FP8 pool adds its [2, kv_heads] scales,
        and an observing pool the layer's amax recorder."""
        if self._observed is not None:
            scales = self.scales[i] if self.scales is not None else None
            return self.k[i], self.v[i], scales, self._observer(i)
        if self.scales is not None:
            return self.k[i], self.v[i], self.scales[i]
        return self.k[i], self.v[i]

    def set_scales(self, scales: torch.Tensor) -> None:
        """In-place update with [layers, 2, kv_heads] (or [layers, 2],
        broadcast over heads) powers of two. The caller guarantees that no
        block holds data."""
        if self.scales is None:
            raise ValueError("KV scales need an FP8 KV cache")
        s = torch.as_tensor(scales, dtype=torch.float32)
        if s.dim() == 2:
            s = s.unsqueeze(-1)
        if s.dim() != 3 or s.shape[:2] != self.scales.shape[:2] or s.shape[2] not in (
            1,
            self.scales.shape[2],
        ):
            raise ValueError(
                f"KV scales must be [layers, 2, kv_heads] = "
                f"{list(self.scales.shape)} or [layers, 2]; got {list(s.shape)}"
            )
        self.scales.copy_(s.expand_as(self.scales))

    # -- calibration observer -------------------------------------------
    def start_observing(self) -> None:
        self._observed = torch.zeros(
            (self.k.shape[0], 2, self.k.shape[2]),
            dtype=torch.float32,
            device=self.k.device,
        )

    def stop_observing(self) -> torch.Tensor:
        obs, self._observed = self._observed, None
        return obs

    def _observer(self, i: int):
        rec = self._observed[i]

        def observe(k: torch.Tensor, v: torch.Tensor) -> None:
            # k, v: [T, kv_heads, D], the values a bf16 cache would hold
            torch.maximum(rec[0], k.float().abs().amax(dim=(0, 2)), out=rec[0])
            torch.maximum(rec[1], v.float().abs().amax(dim=(0, 2)), out=rec[1])

        return observe

    def copy_block(self, src: int, dst: int) -> None:
        """COW copy for fork of a partial tail block."""
        self.k[:, dst].copy_(self.k[:, src])
        self.v[:, dst].copy_(self.v[:, src])

    @staticmethod
    def blocks_for_memory(
        bytes_budget: int,
        num_layers: int,
        num_kv_heads: int,
        head_dim: int,
        block_size: int = DEFAULT_BLOCK_SIZE,
        dtype_bytes: int = 2,
    ) -> int:
        per_block = 2 * num_layers * num_kv_heads * block_size * head_dim * dtype_bytes
        return max(1, bytes_budget // per_block)
