"""bench.py --dump-outputs: the arrays written for one search result."""

import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

from dts_amd.llm.types import Message
from dts_amd.search.types import (
    DialogueNode,
    DTSRunResult,
    NodeStats,
    NodeStatus,
    Strategy,
)

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("_bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _result():
    root = DialogueNode(id="root", messages=[Message.user("hi")])
    a = DialogueNode(
        id="a",
        parent_id="root",
        strategy=Strategy("A", "first"),
        messages=[Message.user("hi"), Message.assistant("héllo")],
        stats=NodeStats(visits=1, value_mean=7.5, judge_scores=[7.0, 8.0],
                        aggregated_score=7.5),
    )
    b = DialogueNode(
        id="b",
        parent_id="root",
        strategy=Strategy("B", "second"),
        status=NodeStatus.PRUNED,
        messages=[Message.user("hi"), Message.assistant(None), Message.user("x")],
        stats=NodeStats(visits=1, value_mean=3.0, judge_scores=[3.0],
                        aggregated_score=3.0),
    )
    return DTSRunResult(
        best_node_id="a", best_score=7.5, best_messages=a.messages,
        all_nodes=[root, a, b], pruned_count=1, total_rounds=1,
    )


def test_dump_outputs_arrays(bench, tmp_path):
    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(_result(), str(out))
    arrs = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert set(arrs) == {
        "aggregated_score", "judge_scores", "value_mean", "visits", "pruned",
        "best", "message_bytes", "message_lengths",
    }
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    # one row per strategy branch, root excluded, tree order kept
    np.testing.assert_array_equal(arrs["aggregated_score"], [7.5, 3.0])
    np.testing.assert_array_equal(arrs["judge_scores"], [[7.0, 8.0], [3.0, -1.0]])
    np.testing.assert_array_equal(arrs["pruned"], [0.0, 1.0])
    np.testing.assert_array_equal(arrs["best"], [0.0, 7.5])
    np.testing.assert_array_equal(arrs["message_lengths"], [[2, 6, -1], [2, 0, 1]])
    row0 = arrs["message_bytes"][0]
    assert bytes(row0[row0 >= 0].astype(np.uint8)) == "hi\x1ehéllo".encode()
    row1 = arrs["message_bytes"][1]
    assert bytes(row1[row1 >= 0].astype(np.uint8)) == b"hi\x1e\x1ex"


def test_dump_outputs_respects_byte_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "_DUMP_MAX_BYTES", 4 * 10)
    bench.dump_outputs(_result(), str(tmp_path))
    # second row would widen the array past the budget: dropped whole
    assert np.load(tmp_path / "message_bytes.npy").shape == (1, 9)
    assert np.load(tmp_path / "message_lengths.npy").shape == (2, 3)


def _lockstep_search(bench, monkeypatch, tmp_path, name):
    """One tiny search through bench.run_search on a fresh CPU engine."""
    import asyncio

    import torch

    from dts_amd.llm import LLM
    from dts_amd.parallel.dp import DPContext
    from dts_amd.serving import LocalBackend, ServingEngine

    monkeypatch.setattr(sys, "argv", ["bench.py", "--branches-per-gpu", "2",
                                      "--turns", "1"])
    args = bench.parse_args()
    engine = ServingEngine(
        model_name="llama-tiny", device="cpu", dtype=torch.float32,
        kv_memory_bytes=128 << 20, weight_seed=0,
    )
    backend = LocalBackend({"llama-tiny": engine}, default_model="llama-tiny")
    backend.shutdown()
    assert engine._thread is None  # nothing but the driver steps the engine
    llm = LLM(backend, default_model="llama-tiny")
    cfg = bench.build_config(args, 1, seed=7)
    scored, _, result = asyncio.run(
        bench.run_search(llm, cfg, DPContext(), [engine], rounds=1)
    )
    assert scored == 2 and engine.steps > 0
    out = tmp_path / name
    bench.dump_outputs(result, str(out))
    return {p.stem: np.load(p) for p in out.glob("*.npy")}


def test_lockstep_search_repeats_exactly(bench, monkeypatch, tmp_path):
    a = _lockstep_search(bench, monkeypatch, tmp_path, "a")
    b = _lockstep_search(bench, monkeypatch, tmp_path, "b")
    assert a.keys() == b.keys() and a["message_bytes"].shape[0] == 2
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_cli_options(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4",
                                      "--warmup", "2"])
    args = bench.parse_args()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (4, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse_args()
    assert args.full and args.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
