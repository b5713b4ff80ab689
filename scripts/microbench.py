"""Engine-step breakdown microbench (run on the GPU box via gpurun).

Times the three phases of ServingEngine.step — schedule (host), forward
(GPU), sample (GPU+host sync) — under a pure-decode load at several batch
widths, plus a prefill-throughput probe. Prints one JSON line per probe.
"""

from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from dts_amd.llm.types import SamplingParams  # noqa: E402
from dts_amd.serving import ServingEngine  # noqa: E402


def timed_steps(engine, n_steps):
    t_sched = t_fwd = t_samp = 0.0
    steps = 0
    sampled = 0
    prefilled = 0
    for _ in range(n_steps):
        t0 = time.perf_counter()
        with engine._lock:
            batch = engine.scheduler.schedule()
        if batch is None:
            break
        t1 = time.perf_counter()
        if engine._graph_runner is not None and engine._graph_runner.can_run(batch):
            logits = engine._graph_runner.run(batch)
        else:
            dev_batch = batch.to(engine.device)
            with torch.inference_mode():
                logits = engine.model.forward(dev_batch, engine.kv_pool)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        seqs = batch._sampled_seqs
        toks = engine.sampler.sample(logits, seqs) if seqs else []
        t3 = time.perf_counter()
        with engine._lock:
            engine.scheduler.advance_computed(batch)
            for seq, tok in zip(seqs, toks):
                engine._handle_sampled(seq, tok)
        t_sched += t1 - t0
        t_fwd += t2 - t1
        t_samp += t3 - t2
        steps += 1
        sampled += len(toks)
        prefilled += batch.num_prefill_tokens
    return dict(
        steps=steps,
        sampled=sampled,
        prefilled=prefilled,
        sched_ms=t_sched / max(1, steps) * 1e3,
        fwd_ms=t_fwd / max(1, steps) * 1e3,
        samp_ms=t_samp / max(1, steps) * 1e3,
    )


def _time_us(fn, n_variants, iters=50, reps=3):
    """Median-of-reps wall time per call (us) of fn(i), i cycling through
    n_variants operand sets so that weights larger than the 256 MB
    Infinity Cache really stream from HBM, as they do across the 32
    layers of a decode step."""
    for i in range(max(3, n_variants)):
        fn(i % n_variants)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(iters):
            fn(i % n_variants)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / iters * 1e6)
    return sorted(ts)[len(ts) // 2]


def kernel_probes(ext):
    """Decode-kernel probes at the shapes the flagship really runs:
    skinny-GEMM tiles-per-workgroup sweep on every Llama-3-8B projection
    (incl. the fused gate_up N=28672 and lm_head N=128256), the fused
    SwiGLU epilogue vs GEMM + silu_mul, and decode attention."""
    dev = "cuda"
    bf16 = torch.bfloat16
    # ---- skinny GEMM NT sweep (+ fused SwiGLU on the gate_up shape)
    shapes = (
        ("qkv", 4096, 6144),
        ("o", 4096, 4096),
        ("gate_up", 4096, 28672),
        ("down", 14336, 4096),
        ("lm_head", 4096, 128256),
    )
    for name, K, N in shapes:
        copies = max(2, min(8, (1 << 30) // (N * K * 2) + 1))
        ws = [torch.randn(N, K, dtype=bf16, device=dev) for _ in range(copies)]
        for M in (1, 4, 8, 16):
            x = torch.randn(M, K, dtype=bf16, device=dev)
            out = torch.empty(M, N, dtype=bf16, device=dev)
            rec = {"probe": f"skinny_{name}_M{M}_K{K}_N{N}", "copies": copies}
            for nt in (1, 2, 4):
                t = _time_us(
                    lambda i: ext.gemm_skinny_bf16(out, x, ws[i], tiles_per_wg=nt),
                    copies,
                )
                rec[f"nt{nt}_us"] = round(t, 1)
                rec[f"nt{nt}_TBps"] = round(N * K * 2 / t / 1e6, 2)
            for ku in (4, 8):  # k-chunks in flight, at one tile per workgroup
                t = _time_us(
                    lambda i: ext.gemm_skinny_bf16(
                        out, x, ws[i], tiles_per_wg=1, unroll=ku
                    ),
                    copies,
                )
                rec[f"nt1_ku{ku}_us"] = round(t, 1)
            t = _time_us(lambda i: ext.gemm_skinny_bf16(out, x, ws[i]), copies)
            rec["auto_us"] = round(t, 1)
            if name == "gate_up":
                act = torch.empty(M, N // 2, dtype=bf16, device=dev)

                def two_kernels(i):
                    ext.gemm_skinny_bf16(out, x, ws[i], tiles_per_wg=1)
                    ext.silu_mul(act, out)

                rec["gemm_nt1_plus_silu_mul_us"] = round(
                    _time_us(two_kernels, copies), 1
                )
                t = _time_us(
                    lambda i: ext.gemm_skinny_swiglu_bf16(act, x, ws[i]), copies
                )
                rec["fused_swiglu_us"] = round(t, 1)
                rec["fused_swiglu_TBps"] = round(N * K * 2 / t / 1e6, 2)
            print(json.dumps(rec), flush=True)
        del ws

    # ---- decode attention (Llama-3-8B heads: Hq=32, Hkv=8, D=128)
    Hq, Hkv, D, BS = 32, 8, 128, 16
    for B in (1, 6, 16):
        for kv in (512, 2048, 12288):
            pages = kv // BS
            layers = 8  # distinct caches, cycled like a step's layers
            NB = B * pages
            kcs = [torch.randn(NB, Hkv, BS, D, dtype=bf16, device=dev) for _ in range(layers)]
            vcs = [torch.randn(NB, Hkv, BS, D, dtype=bf16, device=dev) for _ in range(layers)]
            bt = torch.randperm(NB, device=dev).to(torch.int32).view(B, pages)
            kvl = torch.full((B,), kv, dtype=torch.int32, device=dev)
            kvl -= torch.arange(B, dtype=torch.int32, device=dev) * 3  # ragged
            q = torch.randn(B, Hq, D, dtype=bf16, device=dev)
            out = torch.empty_like(q)
            rec = {"probe": f"attn_decode_B{B}_kv{kv}",
                   "kv_MB": round(2 * B * kv * Hkv * D * 2 / 1e6, 1)}
            t = _time_us(
                lambda i: ext.attn_decode_paged(
                    out, q, kcs[i], vcs[i], bt, kvl, D**-0.5
                ),
                layers,
            )
            rec["decode_plus_combine_us"] = round(t, 1)
            print(json.dumps(rec), flush=True)
            del kcs, vcs


def fp8_kernel_probes(ext):
    """W8A16 skinny GEMM on the five Llama-3-8B shapes: tiles-per-workgroup
    and unroll sweeps, the fused SwiGLU crossover, and the bf16 kernel's
    auto dispatch on the same shape in the same process. The yardstick is
    bytes: TB/s counts the weight bytes each dtype really moves. Weights
    cycle through enough copies to exceed the 256 MB Infinity Cache, as in
    kernel_probes (FP8 copies are half the size, so there are more)."""
    dev = "cuda"
    bf16 = torch.bfloat16
    shapes = (
        ("qkv", 4096, 6144),
        ("o", 4096, 4096),
        ("gate_up", 4096, 28672),
        ("down", 14336, 4096),
        ("lm_head", 4096, 128256),
    )
    for name, K, N in shapes:
        copies = max(2, min(32, (512 << 20) // (N * K) + 1))
        ws = []
        for _ in range(copies):  # finite e4m3 codes, random sign
            c = torch.randint(0, 127, (N, K), dtype=torch.uint8, device=dev)
            c += torch.randint(0, 2, (N, K), dtype=torch.uint8, device=dev) * 128
            ws.append(c.view(torch.float8_e4m3fn))
        del c
        scale = torch.rand(N, device=dev) + 0.5
        copies16 = max(2, min(8, (1 << 30) // (N * K * 2) + 1))
        ws16 = [torch.randn(N, K, dtype=bf16, device=dev) for _ in range(copies16)]
        for M in (1, 4, 8, 16):
            x = torch.randn(M, K, dtype=bf16, device=dev)
            out = torch.empty(M, N, dtype=bf16, device=dev)
            rec = {"probe": f"skinny_w8_{name}_M{M}_K{K}_N{N}", "copies": copies}
            for nt in (1, 2, 4):
                for ku in (4, 8):
                    t = _time_us(
                        lambda i: ext.gemm_skinny_w8_bf16(
                            out, x, ws[i], scale, tiles_per_wg=nt, unroll=ku
                        ),
                        copies,
                    )
                    rec[f"nt{nt}_ku{ku}_us"] = round(t, 1)
                    rec[f"nt{nt}_ku{ku}_TBps"] = round(N * K / t / 1e6, 2)
            t = _time_us(
                lambda i: ext.gemm_skinny_w8_bf16(out, x, ws[i], scale), copies
            )
            rec["auto_us"] = round(t, 1)
            rec["auto_TBps"] = round(N * K / t / 1e6, 2)
            t = _time_us(lambda i: ext.gemm_skinny_bf16(out, x, ws16[i]), copies16)
            rec["bf16_auto_us"] = round(t, 1)
            rec["bf16_auto_TBps"] = round(N * K * 2 / t / 1e6, 2)
            if name == "gate_up":
                act = torch.empty(M, N // 2, dtype=bf16, device=dev)

                def two_kernels(i):
                    ext.gemm_skinny_w8_bf16(out, x, ws[i], scale)
                    ext.silu_mul(act, out)

                rec["gemm_auto_plus_silu_mul_us"] = round(
                    _time_us(two_kernels, copies), 1
                )
                t = _time_us(
                    lambda i: ext.gemm_skinny_swiglu_w8_bf16(act, x, ws[i], scale),
                    copies,
                )
                rec["fused_swiglu_us"] = round(t, 1)
                rec["fused_swiglu_TBps"] = round(N * K / t / 1e6, 2)
            print(json.dumps(rec), flush=True)
        del ws, ws16


def fp4_kernel_probes(ext):
    """W4A16 (MXFP4) skinny GEMM on the five Llama-3-8B shapes next to the
    W8A16 and bf16 kernels' auto dispatch: the three dtypes alternate in this
    process, three rounds each; every figure is the median round and
    *_spread_us is max - min. The MXFP4 kernel is swept over
    tiles-per-workgroup x unroll, plus its auto dispatch and, on gate_up,
    the fused SwiGLU against GEMM + silu_mul. TB/s counts the weight bytes
    each dtype really moves (codes + block scales for MXFP4). Weights cycle
    through enough copies to exceed the 256 MB Infinity Cache."""
    dev = "cuda"
    bf16 = torch.bfloat16
    shapes = (
        ("qkv", 4096, 6144),
        ("o", 4096, 4096),
        ("gate_up", 4096, 28672),
        ("down", 14336, 4096),
        ("lm_head", 4096, 128256),
    )
    rounds = 3

    def med(ts):
        return round(sorted(ts)[len(ts) // 2], 1), round(max(ts) - min(ts), 1)

    for name, K, N in shapes:
        w4_bytes = N * K // 2 + N * K // 32
        c4 = max(2, min(64, (512 << 20) // w4_bytes + 1))
        c8 = max(2, min(32, (512 << 20) // (N * K) + 1))
        c16 = max(2, min(8, (1 << 30) // (N * K * 2) + 1))
        ws4 = [torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=dev)
               for _ in range(c4)]
        sc4 = torch.randint(117, 123, (N, K // 32), dtype=torch.uint8, device=dev)
        ws8 = []
        for _ in range(c8):  # finite e4m3 codes
            c = torch.randint(0, 127, (N, K), dtype=torch.uint8, device=dev)
            ws8.append(c.view(torch.float8_e4m3fn))
        del c
        sc8 = torch.rand(N, device=dev) + 0.5
        ws16 = [torch.randn(N, K, dtype=bf16, device=dev) for _ in range(c16)]
        for M in (1, 4, 8, 16):
            x = torch.randn(M, K, dtype=bf16, device=dev)
            out = torch.empty(M, N, dtype=bf16, device=dev)
            act = torch.empty(M, N // 2, dtype=bf16, device=dev)
            kus = [u for u in (4, 8, 16) if K % (128 * u) == 0]
            fns = {
                "bf16_auto": (lambda i: ext.gemm_skinny_bf16(out, x, ws16[i]), c16),
                "fp8_auto": (lambda i: ext.gemm_skinny_w8_bf16(out, x, ws8[i], sc8), c8),
                "auto": (lambda i: ext.gemm_skinny_w4_bf16(out, x, ws4[i], sc4), c4),
            }
            for nt in (1, 2, 4):
                for ku in kus:
                    fns[f"nt{nt}_ku{ku}"] = (
                        lambda i, nt=nt, ku=ku: ext.gemm_skinny_w4_bf16(
                            out, x, ws4[i], sc4, tiles_per_wg=nt, unroll=ku), c4)
            if name == "gate_up":
                def two_kernels(i):
                    ext.gemm_skinny_w4_bf16(out, x, ws4[i], sc4)
                    ext.silu_mul(act, out)

                fns["gemm_auto_plus_silu_mul"] = (two_kernels, c4)
                fns["fused_swiglu"] = (
                    lambda i: ext.gemm_skinny_swiglu_w4_bf16(act, x, ws4[i], sc4), c4)
            ts = {k: [] for k in fns}
            for _ in range(rounds):
                for k, (fn, copies) in fns.items():
                    ts[k].append(_time_us(fn, copies, reps=1))
            rec = {"probe": f"skinny_w4_{name}_M{M}_K{K}_N{N}", "copies": c4}
            for k in fns:
                rec[f"{k}_us"], rec[f"{k}_spread_us"] = med(ts[k])
            rec["bf16_auto_TBps"] = round(N * K * 2 / rec["bf16_auto_us"] / 1e6, 2)
            rec["fp8_auto_TBps"] = round(N * K / rec["fp8_auto_us"] / 1e6, 2)
            rec["auto_TBps"] = round(w4_bytes / rec["auto_us"] / 1e6, 2)
            pinned = {k: rec[f"{k}_us"] for k in fns if k.startswith("nt")}
            rec["best_pinned"] = min(pinned, key=pinned.get)
            rec["best_pinned_us"] = pinned[rec["best_pinned"]]
            print(json.dumps(rec), flush=True)
        del ws4, ws8, ws16


def kv_fp8_probes(ext):
    """Decode attention on an FP8 (e4m3) paged KV cache against the bf16
    kernel: the B x kv grid and the 8 cycled caches of kernel_probes, both
    dtypes in this process, alternating, three rounds each (median). TB/s
    counts the K/V bytes each dtype really moves. The scaled row is the FP8
    kernel reading per-head power-of-two scales from device memory
    (kv_scale) on the same codes; *_spread_us is max - min of the rounds."""
    dev = "cuda"
    bf16 = torch.bfloat16
    Hq, Hkv, D, BS = 32, 8, 128, 16
    layers = 8
    for B in (1, 6, 16):
        for kv in (512, 2048, 12288):
            pages = kv // BS
            NB = B * pages
            shape = (NB, Hkv, BS, D)
            k16 = [torch.randn(shape, dtype=bf16, device=dev) for _ in range(layers)]
            v16 = [torch.randn(shape, dtype=bf16, device=dev) for _ in range(layers)]
            # the same values, stored as the append kernel would store them
            k8 = [t.float().clamp(-448, 448).to(torch.float8_e4m3fn) for t in k16]
            v8 = [t.float().clamp(-448, 448).to(torch.float8_e4m3fn) for t in v16]
            bt = torch.randperm(NB, device=dev).to(torch.int32).view(B, pages)
            kvl = torch.full((B,), kv, dtype=torch.int32, device=dev)
            kvl -= torch.arange(B, dtype=torch.int32, device=dev) * 3  # ragged
            q = torch.randn(B, Hq, D, dtype=bf16, device=dev)
            out = torch.empty_like(q)
            elems = 2 * int(kvl.sum()) * Hkv * D
            rec = {"probe": f"attn_decode_kv_fp8_B{B}_kv{kv}",
                   "kv_MB_bf16": round(elems * 2 / 1e6, 1),
                   "kv_MB_fp8": round(elems / 1e6, 1)}
            kv_scale = torch.tensor(
                [[2.0 ** (h - 4) for h in range(Hkv)],
                 [2.0 ** (3 - h) for h in range(Hkv)]],
                dtype=torch.float32, device=dev)
            t16, t8, t8s = [], [], []
            for _ in range(3):
                t16.append(_time_us(
                    lambda i: ext.attn_decode_paged(
                        out, q, k16[i], v16[i], bt, kvl, D**-0.5),
                    layers, reps=1))
                t8.append(_time_us(
                    lambda i: ext.attn_decode_paged(
                        out, q, k8[i], v8[i], bt, kvl, D**-0.5),
                    layers, reps=1))
                t8s.append(_time_us(
                    lambda i: ext.attn_decode_paged(
                        out, q, k8[i], v8[i], bt, kvl, D**-0.5, kv_scale),
                    layers, reps=1))
            a, b = sorted(t16)[1], sorted(t8)[1]
            rec["bf16_us"] = round(a, 1)
            rec["fp8_us"] = round(b, 1)
            rec["bf16_TBps"] = round(elems * 2 / a / 1e6, 2)
            rec["fp8_TBps"] = round(elems / b / 1e6, 2)
            rec["speedup"] = round(a / b, 3)
            rec["fp8_scaled_us"] = round(sorted(t8s)[1], 1)
            rec["fp8_spread_us"] = round(max(t8) - min(t8), 1)
            rec["fp8_scaled_spread_us"] = round(max(t8s) - min(t8s), 1)
            print(json.dumps(rec), flush=True)
            del k16, v16, k8, v8


def persistent_probes(ext):
    """Persistent skinny GEMM (one workgroup per CU, activation in LDS)
    against the current auto dispatch with the persistent path pinned off,
    on the K=4096 Llama-3-8B shapes: qkv, gate_up (plain and fused SwiGLU)
    and lm_head at M = 1, 4, 8, 16. The two alternate in this process, five
    rounds each; every figure is the median round and *_spread_us is
    max - min. Weights cycle through enough copies to exceed the 256 MB
    Infinity Cache."""
    dev = "cuda"
    bf16 = torch.bfloat16
    shapes = (("qkv", 4096, 6144), ("gate_up", 4096, 28672),
              ("lm_head", 4096, 128256))
    rounds = 5

    def med(ts):
        return round(sorted(ts)[len(ts) // 2], 1), round(max(ts) - min(ts), 1)

    for name, K, N in shapes:
        copies = max(2, min(8, (1 << 30) // (N * K * 2) + 1))
        ws = [torch.randn(N, K, dtype=bf16, device=dev) for _ in range(copies)]
        for M in (1, 4, 8, 16):
            x = torch.randn(M, K, dtype=bf16, device=dev)
            out = torch.empty(M, N, dtype=bf16, device=dev)
            act = torch.empty(M, N // 2, dtype=bf16, device=dev)
            fns = {
                "current": lambda i: ext.gemm_skinny_bf16(
                    out, x, ws[i], persistent=0),
                "persistent": lambda i: ext.gemm_skinny_bf16(
                    out, x, ws[i], persistent=1),
            }
            if name == "gate_up":
                fns["swiglu_current"] = lambda i: ext.gemm_skinny_swiglu_bf16(
                    act, x, ws[i], persistent=0)
                fns["swiglu_persistent"] = lambda i: ext.gemm_skinny_swiglu_bf16(
                    act, x, ws[i], persistent=1)

                def plain_plus_silu(i):
                    ext.gemm_skinny_bf16(out, x, ws[i], persistent=1)
                    ext.silu_mul(act, out)

                fns["persistent_plus_silu_mul"] = plain_plus_silu
            ts = {k: [] for k in fns}
            for _ in range(rounds):
                for k, fn in fns.items():
                    ts[k].append(_time_us(fn, copies, reps=1))
            rec = {"probe": f"skinny_persistent_{name}_M{M}_K{K}_N{N}",
                   "copies": copies}
            for k in fns:
                rec[f"{k}_us"], rec[f"{k}_spread_us"] = med(ts[k])
            rec["persistent_TBps"] = round(
                N * K * 2 / rec["persistent_us"] / 1e6, 2)
            print(json.dumps(rec), flush=True)
        del ws


def stream_probes(ext):
    """Stream skinny GEMM (unroll=16|32: a ring of load groups in flight per
    wave) against the current auto dispatch on the three Llama-3-8B decode
    projections it is meant for — o, qkv (one and two tiles per workgroup)
    and down — at M = 1, 4, 6, 8, 16. The variants alternate in this process,
    five rounds each; every figure is the median round and *_spread_us is
    max - min. Weights cycle through enough copies to exceed the 256 MB
    Infinity Cache. `auto` is the dispatcher as built (it includes the
    stream rule once one is set); `current` pins the pre-stream choice."""
    dev = "cuda"
    bf16 = torch.bfloat16
    shapes = (("o", 4096, 4096), ("qkv", 4096, 6144), ("down", 14336, 4096))
    rounds = 5

    def med(ts):
        return round(sorted(ts)[len(ts) // 2], 1), round(max(ts) - min(ts), 1)

    for name, K, N in shapes:
        copies = max(2, min(16, (1 << 30) // (N * K * 2) + 1))
        ws = [torch.randn(N, K, dtype=bf16, device=dev) for _ in range(copies)]
        for M in (1, 4, 6, 8, 16):
            x = torch.randn(M, K, dtype=bf16, device=dev)
            out = torch.empty(M, N, dtype=bf16, device=dev)
            # what the dispatcher chose before the stream kernel existed
            nt = 2 if (name == "qkv" and M >= 8) else 1
            ku = 8 if K >= 8192 else 4

            def call(**pins):
                return lambda i: ext.gemm_skinny_bf16(out, x, ws[i], **pins)

            fns = {
                "current": call(tiles_per_wg=nt, unroll=ku),
                "auto": call(),
                "stream16": call(tiles_per_wg=1, unroll=16),
                "stream32": call(tiles_per_wg=1, unroll=32),
            }
            if name == "qkv":
                fns["stream16_nt2"] = call(tiles_per_wg=2, unroll=16)
            ts = {k: [] for k in fns}
            for _ in range(rounds):
                for k, fn in fns.items():
                    ts[k].append(_time_us(fn, copies, iters=200, reps=1))
            rec = {"probe": f"skinny_stream_{name}_M{M}_K{K}_N{N}",
                   "copies": copies, "current_nt": nt, "current_unroll": ku}
            for k in fns:
                rec[f"{k}_us"], rec[f"{k}_spread_us"] = med(ts[k])
            best = min((k for k in fns if k.startswith("stream")),
                       key=lambda k: rec[f"{k}_us"])
            rec["best_stream"] = best
            rec["best_stream_TBps"] = round(
                N * K * 2 / rec[f"{best}_us"] / 1e6, 2)
            rec["current_TBps"] = round(N * K * 2 / rec["current_us"] / 1e6, 2)
            print(json.dumps(rec), flush=True)
        del ws


def moe_tiled_probes(ext):
    """Tiled grouped MoE GEMM against the per-expert loop at one Mixtral-8x7B
    layer (E = 8, H = 4096, I = 14336, top_k = 2; 2.8 GB of experts, far past
    the Infinity Cache, so weights are cold without cycling). Per T and
    routing (near-uniform; skewed = half the assignments on two experts) it
    times the whole MoEMLP.forward with `tiled` False and True, and the two
    GEMM calls alone (moe_grouped_gemm with fused SwiGLU, then down) against
    F.linear + silu_mul + F.linear per expert on host-known segments; the
    tiled variants run with 64-row blocks (`tiled`, `gemms_tiled`) and with
    the 128-row LDS-shared blocks (`tiled128`, `gemms_tiled128`). The
    variants alternate in this process, five rounds; every figure is the
    median round and *_spread_us is max - min. `parent` names what the rule
    of the commit before the 128-row kernel runs at that size (`tiled` inside
    66..1024 rows, else `loop`); `tiled128_wins` is the 3x-spread rule
    against it, `bit_equal` whether both block sizes give the same bits."""
    import torch.nn.functional as F

    from dts_amd import ops
    from dts_amd.models.config import ModelSpec
    from dts_amd.models.mixtral import MoEMLP
    from dts_amd.parallel.tp import TPContext

    E, H, I, TOP_K = 8, 4096, 14336, 2
    spec = ModelSpec(
        name="moe-bench", arch="mixtral", vocab_size=512, hidden_size=H,
        intermediate_size=I, num_layers=1, num_heads=32, num_kv_heads=8,
        head_dim=128, rope_theta=1e4, max_position=2048,
        num_experts=E, experts_per_token=TOP_K,
    )
    moe = MoEMLP(spec, TPContext.single(), torch.bfloat16).to("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        moe.gate_up_w.normal_(0, 0.02, generator=g)
        moe.down_w.normal_(0, 0.02, generator=g)
        # expert e's logit is 4 x[:, e]: the first E columns of x pick the
        # experts, the other columns are ordinary activations
        moe.router_w.zero_()
        moe.router_w[:, :E] = 4.0 * torch.eye(E, device="cuda")

    def routed_x(T, skewed):
        t = torch.arange(T)
        if skewed:  # tokens 0, 2, 4, ... take experts (0, 1)
            rest = t // 2
            e1 = torch.where(t % 2 == 0, 0, 2 + rest % 6)
            e2 = torch.where(t % 2 == 0, 1, 2 + (rest + 1 + (rest // 6) % 5) % 6)
        else:
            e1 = t % E
            e2 = (t + 1 + (t // E) % (E - 1)) % E
        x = torch.randn(T, H, generator=torch.Generator().manual_seed(T))
        x[:, :E] = 0.0
        x[t, e1], x[t, e2] = 4.0, 3.5
        return x.to(torch.bfloat16).cuda(), torch.bincount(
            torch.cat([e1, e2]), minlength=E).tolist()

    def med(ts):
        return round(sorted(ts)[len(ts) // 2], 1), round(max(ts) - min(ts), 1)

    for T in (33, 64, 128, 256, 512, 1024, 2048, 4096):
        for routing in ("uniform", "skewed"):
            x, hist = routed_x(T, routing == "skewed")
            counts = torch.tensor(hist, dtype=torch.int32, device="cuda")
            offsets = (torch.cumsum(counts, 0) - counts).to(torch.int32)
            segs = [(int(o), int(o) + c) for o, c in zip(offsets.tolist(), hist)]
            xs = torch.randn(T * TOP_K, H, dtype=torch.bfloat16, device="cuda")

            def forward(tiled, block=64):
                def fn(_):
                    moe.tiled, moe.tiled_block = tiled, block
                    with torch.inference_mode():
                        return moe(x)
                return fn

            def gemms_tiled(_, block=64):
                act = ops.moe_grouped_gemm(
                    xs, moe.gate_up_w, counts, offsets, True, block)
                return ops.moe_grouped_gemm(act, moe.down_w, counts, offsets, block=block)

            def gemms_linear(_):
                for e, (a, b) in enumerate(segs):
                    F.linear(ops.silu_mul(F.linear(xs[a:b], moe.gate_up_w[e])),
                             moe.down_w[e])

            fns = {"loop": forward(False), "tiled": forward(True),
                   "tiled128": forward(True, 128),
                   "gemms_linear": gemms_linear, "gemms_tiled": gemms_tiled,
                   "gemms_tiled128": lambda _: gemms_tiled(_, 128)}
            out64 = fns["tiled"](0)
            assert out64.isfinite().all()
            bit_equal = bool(torch.equal(out64, fns["tiled128"](0))) and bool(
                torch.equal(gemms_tiled(0), gemms_tiled(0, 128)))
            iters = 20 if T <= 512 else 8
            ts = {k: [] for k in fns}
            for _ in range(5):
                for k, fn in fns.items():
                    ts[k].append(_time_us(fn, 1, iters=iters, reps=1))
            rec = {"probe": f"moe_tiled_T{T}_{routing}", "rows": T * TOP_K,
                   "K": H, "N": I, "hist": hist}
            for k in fns:
                rec[f"{k}_us"], rec[f"{k}_spread_us"] = med(ts[k])
            spread = max(rec["loop_spread_us"], rec["tiled_spread_us"])
            rec["tiled_wins"] = rec["loop_us"] - rec["tiled_us"] > 3 * spread
            rec["parent"] = "tiled" if 66 <= T * TOP_K <= 1024 else "loop"
            spread = max(rec[rec["parent"] + "_spread_us"], rec["tiled128_spread_us"])
            rec["tiled128_wins"] = (
                rec[rec["parent"] + "_us"] - rec["tiled128_us"] > 3 * spread
            )
            rec["bit_equal"] = bit_equal
            print(json.dumps(rec), flush=True)
    moe.tiled_block = 0


def moe_route_probes(ext):
    """Fused MoE routing glue (MoEMLP.fused_route: moe_route, moe_sort_gather,
    moe_combine) against the torch chain at one Mixtral-8x7B layer (E = 8,
    H = 4096, I = 14336, top_k = 2), near-uniform routing. Per T the whole
    MoEMLP.forward is timed with the flag off and on, eager and as a captured
    graph that is replayed; T <= 32 runs the grouped skinny GEMM, above that
    the tiled grouped GEMM (ops.moe_tiled_rule). The four variants alternate
    in this process, five rounds; every figure is the median round and
    *_spread_us is max - min. The router's logits are 16, 14 and 0, so both
    routers pick the same experts; `bit_equal` says whether the two outputs
    are the same bits."""
    from dts_amd.models.config import ModelSpec
    from dts_amd.models.mixtral import MoEMLP
    from dts_amd.parallel.tp import TPContext

    E, H, I, TOP_K = 8, 4096, 14336, 2
    spec = ModelSpec(
        name="moe-bench", arch="mixtral", vocab_size=512, hidden_size=H,
        intermediate_size=I, num_layers=1, num_heads=32, num_kv_heads=8,
        head_dim=128, rope_theta=1e4, max_position=2048,
        num_experts=E, experts_per_token=TOP_K,
    )
    moe = MoEMLP(spec, TPContext.single(), torch.bfloat16).to("cuda")
    moe.tiled = None
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        moe.gate_up_w.normal_(0, 0.02, generator=g)
        moe.down_w.normal_(0, 0.02, generator=g)
        moe.router_w.zero_()
        moe.router_w[:, :E] = 4.0 * torch.eye(E, device="cuda")

    def med(ts):
        return round(sorted(ts)[len(ts) // 2], 1), round(max(ts) - min(ts), 1)

    for T in (1, 6, 16, 33, 128, 512):
        t = torch.arange(T)
        x = torch.randn(T, H, generator=torch.Generator().manual_seed(T))
        x[:, :E] = 0.0
        x[t, t % E], x[t, (t + 1 + (t // E) % (E - 1)) % E] = 4.0, 3.5
        x = x.to(torch.bfloat16).cuda()

        fns, outs = {}, {}
        for name, fused in (("torch", False), ("fused", True)):
            def eager(_, fused=fused):
                moe.fused_route = fused
                with torch.inference_mode():
                    return moe(x)

            moe.fused_route = fused
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.inference_mode():
                for _ in range(2):
                    moe(x)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.inference_mode(), torch.cuda.graph(graph):
                outs[f"graph_{name}"] = moe(x)
            outs[f"eager_{name}"] = eager(0)
            fns[f"eager_{name}"] = eager
            fns[f"graph_{name}"] = lambda _, graph=graph: graph.replay()
        for fn in fns.values():
            fn(0)
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(5):
            for k, fn in fns.items():
                ts[k].append(_time_us(fn, 1, iters=50, reps=1))
        rec = {"probe": f"moe_route_T{T}", "rows": T * TOP_K,
               "path": "grouped" if T * TOP_K <= 64 else "tiled"}
        for k in fns:
            rec[f"{k}_us"], rec[f"{k}_spread_us"] = med(ts[k])
        for mode in ("eager", "graph"):
            a, b = outs[f"{mode}_torch"], outs[f"{mode}_fused"]
            rec[f"{mode}_bit_equal"] = bool(torch.equal(a, b))
            spread = max(rec[f"{mode}_torch_spread_us"], rec[f"{mode}_fused_spread_us"])
            rec[f"{mode}_fused_wins"] = (
                rec[f"{mode}_torch_us"] - rec[f"{mode}_fused_us"] > 3 * spread
            )
        print(json.dumps(rec), flush=True)
    moe.fused_route = False


def persistent_pmc_target(ext, which):
    """The target of a counter run: the Llama-3-8B gate_up at M=8, plain and
    fused SwiGLU, four calls each on four different weights, with the
    persistent path pinned off (which = 'current') or on ('persistent')."""
    pin = {"current": 0, "persistent": 1}[which]
    K, N, M = 4096, 28672, 8
    bf16 = torch.bfloat16
    ws = [torch.randn(N, K, dtype=bf16, device="cuda") for _ in range(4)]
    x = torch.randn(M, K, dtype=bf16, device="cuda")
    out = torch.empty(M, N, dtype=bf16, device="cuda")
    act = torch.empty(M, N // 2, dtype=bf16, device="cuda")
    for w in ws:
        ext.gemm_skinny_bf16(out, x, w, persistent=pin)
    for w in ws:
        ext.gemm_skinny_swiglu_bf16(act, x, w, persistent=pin)
    torch.cuda.synchronize()


def main():
    if "--persistent-pmc" in sys.argv:
        # python scripts/microbench.py --persistent-pmc current|persistent
        from dts_amd.ops import _hip_ext_loader

        persistent_pmc_target(
            _hip_ext_loader.load(), sys.argv[sys.argv.index("--persistent-pmc") + 1]
        )
        return
    if "--moe-tiled-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        moe_tiled_probes(_hip_ext_loader.load())
        return
    if "--moe-route-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        moe_route_probes(_hip_ext_loader.load())
        return
    if "--stream-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        stream_probes(_hip_ext_loader.load())
        return
    if "--persistent-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        persistent_probes(_hip_ext_loader.load())
        return
    if "--kv-fp8-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        kv_fp8_probes(_hip_ext_loader.load())
        return
    if "--fp4-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        fp4_kernel_probes(_hip_ext_loader.load())
        return
    if "--fp8-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        fp8_kernel_probes(_hip_ext_loader.load())
        return
    if "--kernels-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        kernel_probes(_hip_ext_loader.load())
        return
    engine = ServingEngine(
        model_name="llama-3-8b",
        device="cuda:0",
        dtype=torch.bfloat16,
        kv_memory_bytes=32 << 30,
        max_batch_tokens=16384,
        weight_seed=0,
    )
    torch.manual_seed(0)

    # ---- decode probes at different batch widths (and one long-context)
    for B, plen in ((1, 512), (4, 512), (8, 512), (16, 512), (32, 512), (64, 512), (1, 12288), (6, 2048)):
        futs = []
        for i in range(B):
            prompt = [int(x) for x in torch.randint(300, 100000, (plen,))]
            futs.append(
                engine.submit_tokens(
                    prompt, SamplingParams(max_tokens=4096, seed=i, temperature=0.7)
                )
            )
        # drain prefill
        for _ in range(200):
            with engine._lock:
                b = engine.scheduler.schedule()
            if b is None:
                break
            db = b.to(engine.device)
            with torch.inference_mode():
                lg = engine.model.forward(db, engine.kv_pool)
            tk = engine.sampler.sample(lg, b._sampled_seqs) if b._sampled_seqs else []
            with engine._lock:
                engine.scheduler.advance_computed(b)
                for s, t in zip(b._sampled_seqs, tk):
                    engine._handle_sampled(s, t)
            if all(s.num_computed >= s.num_prompt_tokens for s in engine.scheduler.running):
                break
        # warm the graph bucket (capture excluded from timing)
        timed_steps(engine, 4)
        torch.cuda.synchronize()
        r = timed_steps(engine, 64)
        r["probe"] = f"decode_B{B}_kv{plen}"
        r["tok_per_s"] = r["sampled"] / max(
            1e-9, (r["sched_ms"] + r["fwd_ms"] + r["samp_ms"]) / 1e3 * r["steps"]
        )
        print(json.dumps(r))
        # abort the batch (scheduler-agnostic)
        with engine._lock:
            for s in list(engine.scheduler.running):
                engine.scheduler.abort(s)
            engine._futures.clear()

    # ---- GEMV vs hipBLASLt A/B at decode shapes
    from dts_amd.ops import _hip_ext_loader

    ext = _hip_ext_loader.load()
    for M in (1, 2, 4, 8, 16, 24, 32, 64):
        for K, N in ((4096, 14336), (4096, 6144), (14336, 4096)):
            x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda")
            w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda")
            out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
            t_gemv = None
            if M <= 8:
                for _ in range(3):
                    ext.gemv_bf16(out, x, w)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(50):
                    ext.gemv_bf16(out, x, w)
                torch.cuda.synchronize()
                t_gemv = (time.perf_counter() - t0) / 50
            t_skinny = None
            if M <= 16:
                for _ in range(3):
                    ext.gemm_skinny_bf16(out, x, w)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(50):
                    ext.gemm_skinny_bf16(out, x, w)
                torch.cuda.synchronize()
                t_skinny = (time.perf_counter() - t0) / 50
            for _ in range(3):
                torch.nn.functional.linear(x, w)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(50):
                torch.nn.functional.linear(x, w)
            torch.cuda.synchronize()
            t_blas = (time.perf_counter() - t0) / 50
            print(json.dumps({
                "probe": f"gemm_M{M}_K{K}_N{N}",
                "gemv_us": round(t_gemv * 1e6, 1) if t_gemv else None,
                "skinny_us": round(t_skinny * 1e6, 1) if t_skinny else None,
                "skinny_TBps": (
                    round(N * K * 2 / t_skinny / 1e12, 2) if t_skinny else None
                ),
                "hipblaslt_us": round(t_blas * 1e6, 1),
                "blas_TBps": round(N * K * 2 / t_blas / 1e12, 2),
            }))

    kernel_probes(ext)

    # ---- prefill probe: one long prompt
    prompt = [int(x) for x in torch.randint(300, 100000, (8192,))]
    fut = engine.submit_tokens(prompt, SamplingParams(max_tokens=1, seed=0))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    engine.run_until_idle()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(
        json.dumps(
            {
                "probe": "prefill_8k",
                "seconds": round(dt, 4),
                "tok_per_s": round(8192 / dt, 1),
            }
        )
    )


if __name__ == "__main__":
    main()
