"""Cost of the top-k / min-p sampling path against the unfiltered sampler.

Times whole sampler calls (all their kernels and memsets) at the
vocabularies and decode widths the engine runs (gridded kernels: V >= 4096,
S <= 32), two ways, both with a host clock around work that ends in a device
synchronise:

  us_median        ITERS back-to-back eager calls. At these sizes the host
                   enqueues slower than the device drains, so this is the
                   cost of a call where the host is on the critical path
                   (the per-step sampler).
  graph_us_median  GRAPH_CALLS calls captured into one hipGraph, replayed
                   GRAPH_REPLAYS times: launch cost is gone, what is left is
                   the device-side time of a call (what the chained decode
                   loop, whose host runs ahead of the device, pays).

The variants are alternated inside every round, in one process, so drift of
the shared machine hits all of them alike; each figure is the median of
ROUNDS rounds with max - min as the spread.

Variants:
  baseline  the existing top_p_sample_v2 (what every figure is compared to)
  disabled  sample_filtered_v2, every row top_k = 0 and min_p = 0
  top_k     top_k = 50
  min_p     min_p = 0.05
  all       top_k = 50, top_p = 0.9, min_p = 0.05

Prints one JSON line per (V, S, variant); --out FILE also appends them there.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from dts_amd import ops  # noqa: E402
from dts_amd.ops import _hip_ext_loader  # noqa: E402

ROUNDS = 5
ITERS = 500
GRAPH_CALLS = 20
GRAPH_REPLAYS = 50
VOCABS = (128256, 32000)
WIDTHS = (1, 6, 16)
VARIANTS = {
    # name: (filtered entry point?, top_k, top_p, min_p)
    "baseline": (False, 0, 0.95, 0.0),
    "disabled": (True, 0, 0.95, 0.0),
    "top_k": (True, 50, 0.95, 0.0),
    "min_p": (True, 0, 0.95, 0.05),
    "all": (True, 50, 0.9, 0.05),
}


def make_call(ext, logits, name):
    filtered, top_k, top_p, min_p = VARIANTS[name]
    S = logits.shape[0]
    dev = logits.device
    out = torch.empty(S, dtype=torch.long, device=dev)
    temps = torch.full((S,), 0.7, device=dev)
    top_ps = torch.full((S,), top_p, device=dev)
    seeds = torch.arange(1, S + 1, dtype=torch.long, device=dev)
    ws = ops._sampler_workspace(S, dev)
    if not filtered:
        return lambda: ext.top_p_sample_v2(out, logits, temps, top_ps, seeds, *ws)
    top_ks = torch.full((S,), top_k, dtype=torch.int32, device=dev)
    min_ps = torch.full((S,), min_p, device=dev)
    fws = ops._sampler_filter_workspace(S, dev)
    return lambda: ext.sample_filtered_v2(
        out, logits, temps, top_ps, top_ks, min_ps, seeds, *ws, *fws
    )


def capture(fn):
    """GRAPH_CALLS consecutive calls of fn as one graph (a linear chain)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_CALLS):
            fn()
    return graph


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU run cannot give these times")
    ext = _hip_ext_loader.load()
    sink = open(args.out, "a") if args.out else None
    g = torch.Generator().manual_seed(0)
    for V in VOCABS:
        for S in WIDTHS:
            # the spread of real lm_head logits at T=0.7 is a few units
            logits = (torch.randn(S, V, generator=g) * 2.0).to("cuda:0")
            calls = {name: make_call(ext, logits, name) for name in VARIANTS}
            for fn in calls.values():  # warm every variant
                for _ in range(20):
                    fn()
            torch.cuda.synchronize()
            graphs = {name: capture(fn) for name, fn in calls.items()}
            for graph in graphs.values():
                graph.replay()
            torch.cuda.synchronize()
            times = {name: [] for name in VARIANTS}
            gtimes = {name: [] for name in VARIANTS}
            for _ in range(ROUNDS):
                for name, fn in calls.items():
                    t0 = time.perf_counter()
                    for _ in range(ITERS):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / ITERS * 1e6)
                for name, graph in graphs.items():
                    t0 = time.perf_counter()
                    for _ in range(GRAPH_REPLAYS):
                        graph.replay()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    gtimes[name].append(dt / (GRAPH_REPLAYS * GRAPH_CALLS) * 1e6)
            base, gbase = median(times["baseline"]), median(gtimes["baseline"])
            for name, ts in times.items():
                gts = gtimes[name]
                row = {
                    "probe": "sampler_filters", "V": V, "S": S, "variant": name,
                    "us_median": round(median(ts), 2),
                    "us_spread": round(max(ts) - min(ts), 2),
                    "ratio_to_baseline": round(median(ts) / base, 3),
                    "graph_us_median": round(median(gts), 2),
                    "graph_us_spread": round(max(gts) - min(gts), 2),
                    "graph_ratio_to_baseline": round(median(gts) / gbase, 3),
                    "rounds": ROUNDS, "iters": ITERS,
                    "graph_calls": GRAPH_CALLS, "graph_replays": GRAPH_REPLAYS,
                }
                line = json.dumps(row)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
