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


def main():
    if "--kv-fp8-only" in sys.argv:
        from dts_amd.ops import _hip_ext_loader

        kv_fp8_probes(_hip_ext_loader.load())
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
