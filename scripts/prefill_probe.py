"""Isolated prefill-attention kernel probe (TF + for PMC runs).

One sequence, q_len=N self-attention (causal), Llama-3-8B shapes.
FLOPs = 2 ops x (QK^T + PV) x Hq x N^2/2 x D.
"""

import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from dts_amd.ops import _hip_ext_loader  # noqa: E402

ext = _hip_ext_loader.load()


def probe(N=4096, Hq=32, Hkv=8, D=128, iters=20):
    torch.manual_seed(0)
    BS = 16
    n_blocks = N // BS + 2
    q = torch.randn(N, Hq, D, dtype=torch.bfloat16, device="cuda")
    kc = torch.randn(n_blocks, Hkv, BS, D, dtype=torch.bfloat16, device="cuda")
    vc = torch.randn_like(kc)
    bt = torch.arange(1, n_blocks + 1, dtype=torch.int32, device="cuda").unsqueeze(0)
    kvl = torch.tensor([N], dtype=torch.int32, device="cuda")
    cu_q = torch.tensor([0, N], dtype=torch.int32, device="cuda")
    q_pos = torch.arange(N, dtype=torch.long, device="cuda")
    out = torch.empty_like(q)
    scale = D ** -0.5
    flops = 2 * 2 * Hq * (N * N / 2) * D
    results = {}
    # numerics FIRST (and flushed) so a kernel fault localizes to its
    # variant instead of discarding block-buffered timing output
    out_ref = torch.empty_like(q)
    ext.attn_prefill_paged(out_ref, q, cu_q, q_pos, kc, vc, bt, kvl, scale, 0)
    torch.cuda.synchronize()
    print(f"numerics N={N}: v1 ok", flush=True)
    for var in (4, 5):
        out_v = torch.empty_like(q)
        ext.attn_prefill_paged(out_v, q, cu_q, q_pos, kc, vc, bt, kvl, scale, var)
        torch.cuda.synchronize()
        err = float((out_ref.float() - out_v.float()).abs().max())
        print(f"numerics N={N}: variant {var} max_abs_err={err}", flush=True)
    # within-probe interleaved A/B (guide §5.4 rule 24): 6 rounds each
    for swz in (0, 4, 5, 0, 4, 5):
        for _ in range(2):
            ext.attn_prefill_paged(out, q, cu_q, q_pos, kc, vc, bt, kvl,
                                   scale, swz)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            ext.attn_prefill_paged(out, q, cu_q, q_pos, kc, vc, bt, kvl,
                                   scale, swz)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
        results.setdefault(swz, []).append(round(flops / dt / 1e12, 1))
    # numerics: v2 must match v1 closely (different tile size changes
    # the online-softmax accumulation order, so not bitwise)
    out0 = torch.empty_like(q)
    out1 = torch.empty_like(q)
    ext.attn_prefill_paged(out0, q, cu_q, q_pos, kc, vc, bt, kvl, scale, 0)
    ext.attn_prefill_paged(out1, q, cu_q, q_pos, kc, vc, bt, kvl, scale, 4)
    max_err = float((out0.float() - out1.float()).abs().max())
    print(  # noqa
        json.dumps(
            {
                "probe": f"prefill_attn_N{N}",
                "TF_v1": results[0],
                "TF_v5k32": results.get(4),
                "TF_v5k64": results.get(5),
                "v1_v5_max_abs_err": max_err,
            }
        ),
        flush=True,
    )


def probe_kv_fp8(N=4096, Hq=32, Hkv=8, D=128, iters=20):
    """FP8 (e4m3) KV cache against the bf16 cache holding the same values,
    variants 0/4/5, interleaved in one process (two rounds each)."""
    torch.manual_seed(0)
    BS = 16
    n_blocks = N // BS + 2
    q = torch.randn(N, Hq, D, dtype=torch.bfloat16, device="cuda")
    caches = {}
    k8 = torch.randn(n_blocks, Hkv, BS, D, device="cuda").to(torch.float8_e4m3fn)
    v8 = torch.randn(n_blocks, Hkv, BS, D, device="cuda").to(torch.float8_e4m3fn)
    caches["fp8"] = (k8, v8)
    caches["bf16"] = (k8.to(torch.bfloat16), v8.to(torch.bfloat16))
    bt = torch.arange(1, n_blocks + 1, dtype=torch.int32, device="cuda").unsqueeze(0)
    kvl = torch.tensor([N], dtype=torch.int32, device="cuda")
    cu_q = torch.tensor([0, N], dtype=torch.int32, device="cuda")
    q_pos = torch.arange(N, dtype=torch.long, device="cuda")
    out = torch.empty_like(q)
    scale = D ** -0.5
    flops = 2 * 2 * Hq * (N * N / 2) * D
    rec = {"probe": f"prefill_attn_kv_fp8_N{N}"}
    for var in (0, 4, 5):
        outs = {}
        for name, (kc, vc) in caches.items():
            outs[name] = torch.empty_like(q)
            ext.attn_prefill_paged(outs[name], q, cu_q, q_pos, kc, vc, bt, kvl,
                                   scale, var)
        torch.cuda.synchronize()
        rec[f"v{var}_bit_equal"] = bool(torch.equal(outs["fp8"], outs["bf16"]))
    for _ in range(2):
        for var in (0, 4, 5):
            for name, (kc, vc) in caches.items():
                for _ in range(2):
                    ext.attn_prefill_paged(out, q, cu_q, q_pos, kc, vc, bt, kvl,
                                           scale, var)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    ext.attn_prefill_paged(out, q, cu_q, q_pos, kc, vc, bt, kvl,
                                           scale, var)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / iters
                rec.setdefault(f"TF_v{var}_{name}", []).append(
                    round(flops / dt / 1e12, 1)
                )
    print(json.dumps(rec), flush=True)


V6_VARIANTS = {"v5": 5, "v6_reads": 7, "v6_prefetch": 6}


def _median_spread(xs):
    s = sorted(xs)
    return round(s[len(s) // 2], 1), round(s[-1] - s[0], 1)


def _timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters  # us per call


def probe_v6_square(N, Hq=32, Hkv=8, D=128, iters=10, rounds=5):
    """v5 / v6 reads-only / v6 reads+prefetch on the square causal probe,
    alternating in one process: median TF over the rounds and max-min."""
    torch.manual_seed(0)
    BS = 16
    n_blocks = N // BS + 2
    q = torch.randn(N, Hq, D, dtype=torch.bfloat16, device="cuda")
    kc = torch.randn(n_blocks, Hkv, BS, D, dtype=torch.bfloat16, device="cuda")
    vc = torch.randn_like(kc)
    bt = torch.arange(1, n_blocks + 1, dtype=torch.int32, device="cuda").unsqueeze(0)
    kvl = torch.tensor([N], dtype=torch.int32, device="cuda")
    cu_q = torch.tensor([0, N], dtype=torch.int32, device="cuda")
    q_pos = torch.arange(N, dtype=torch.long, device="cuda")
    scale = D ** -0.5
    flops = 2 * 2 * Hq * (N * N / 2) * D
    outs = {}
    for name, var in V6_VARIANTS.items():
        outs[name] = torch.empty_like(q)
        ext.attn_prefill_paged(outs[name], q, cu_q, q_pos, kc, vc, bt, kvl, scale, var)
    torch.cuda.synchronize()
    rec = {
        "probe": f"prefill_v6_square_N{N}",
        "bit_equal": all(torch.equal(outs["v5"], o) for o in outs.values()),
    }
    out = torch.empty_like(q)
    tf = {name: [] for name in V6_VARIANTS}
    for _ in range(rounds):
        for name, var in V6_VARIANTS.items():
            def call():
                ext.attn_prefill_paged(out, q, cu_q, q_pos, kc, vc, bt, kvl, scale, var)
            call()
            tf[name].append(flops / (_timed(call, iters) * 1e-6) / 1e12)
    for name in V6_VARIANTS:
        rec[f"TF_{name}"], rec[f"TF_{name}_spread"] = _median_spread(tf[name])
    print(json.dumps(rec), flush=True)
    return rec


def probe_v6_short_chunks(Hq=32, Hkv=8, D=128, iters=24, rounds=5):
    """A short new chunk over a long cached prefix — the call shape that
    launches 8-64 workgroups. Every call walks a different window of a 1 GiB
    K+V pool, so a window is reused only after the whole pool, four times
    the 256 MB Infinity Cache, has gone by. Median us per call and max-min
    over the rounds, the three variants alternating in one process."""
    torch.manual_seed(0)
    BS = 16
    pool_blocks = (512 << 20) // (Hkv * BS * D * 2)
    kc = torch.randn(pool_blocks, Hkv, BS, D, dtype=torch.bfloat16, device="cuda")
    vc = torch.randn_like(kc)
    scale = D ** -0.5
    recs = []
    for P in (1, 2):
        for prefix in (4096, 8192, 12288):
            for chunk in (16, 32, 48, 272):
                kv_len = prefix + chunk
                max_blocks = (kv_len + BS - 1) // BS
                n_win = pool_blocks // (P * max_blocks)
                tables = torch.arange(
                    n_win * P * max_blocks, dtype=torch.int32, device="cuda"
                ).view(n_win, P, max_blocks)
                q = torch.randn(P * chunk, Hq, D, dtype=torch.bfloat16, device="cuda")
                kvl = torch.full((P,), kv_len, dtype=torch.int32, device="cuda")
                cu_q = torch.arange(P + 1, dtype=torch.int32, device="cuda") * chunk
                q_pos = torch.arange(prefix, kv_len, dtype=torch.long, device="cuda").repeat(P)
                outs = {}
                for name, var in V6_VARIANTS.items():
                    outs[name] = torch.empty_like(q)
                    ext.attn_prefill_paged(
                        outs[name], q, cu_q, q_pos, kc, vc, tables[0], kvl, scale, var
                    )
                torch.cuda.synchronize()
                rec = {
                    "probe": "prefill_v6_short_chunk",
                    "seqs": P, "prefix": prefix, "chunk": chunk,
                    "workgroups": ((P * chunk + 15) // 16) * P * Hkv,
                    "bit_equal": all(torch.equal(outs["v5"], o) for o in outs.values()),
                }
                out = torch.empty_like(q)
                us = {name: [] for name in V6_VARIANTS}
                win = [0]
                for _ in range(rounds):
                    for name, var in V6_VARIANTS.items():
                        def call():
                            win[0] = (win[0] + 1) % n_win
                            ext.attn_prefill_paged(
                                out, q, cu_q, q_pos, kc, vc, tables[win[0]], kvl, scale, var
                            )
                        call()
                        us[name].append(_timed(call, iters))
                for name in V6_VARIANTS:
                    rec[f"us_{name}"], rec[f"us_{name}_spread"] = _median_spread(us[name])
                print(json.dumps(rec), flush=True)
                recs.append(rec)
    return recs


def pmc_target(which, variant):
    """One shape, one variant, a few calls: the target of a counter run.
    which = 'square' (N=4k) or 'short' (a 16-token chunk on a 12k prefix)."""
    torch.manual_seed(0)
    BS, Hq, Hkv, D = 16, 32, 8, 128
    prefix, chunk = (0, 4096) if which == "square" else (12288, 16)
    kv_len = prefix + chunk
    n_blocks = (kv_len + BS - 1) // BS
    q = torch.randn(chunk, Hq, D, dtype=torch.bfloat16, device="cuda")
    kc = torch.randn(n_blocks + 1, Hkv, BS, D, dtype=torch.bfloat16, device="cuda")
    vc = torch.randn_like(kc)
    bt = torch.arange(1, n_blocks + 1, dtype=torch.int32, device="cuda").unsqueeze(0)
    kvl = torch.tensor([kv_len], dtype=torch.int32, device="cuda")
    cu_q = torch.tensor([0, chunk], dtype=torch.int32, device="cuda")
    q_pos = torch.arange(prefix, kv_len, dtype=torch.long, device="cuda")
    out = torch.empty_like(q)
    for _ in range(4):
        ext.attn_prefill_paged(out, q, cu_q, q_pos, kc, vc, bt, kvl, D ** -0.5, variant)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if "--v6" in sys.argv:
        # python scripts/prefill_probe.py --v6 [out.jsonl]
        recs = probe_v6_short_chunks()
        recs += [probe_v6_square(n) for n in (2048, 4096, 8192)]
        path = sys.argv[sys.argv.index("--v6") + 1:]
        if path:
            Path(path[0]).write_text("".join(json.dumps(r) + "\n" for r in recs))
        sys.exit(0)
    if "--pmc" in sys.argv:
        # python scripts/prefill_probe.py --pmc square|short VARIANT
        i = sys.argv.index("--pmc")
        pmc_target(sys.argv[i + 1], int(sys.argv[i + 2]))
        sys.exit(0)
    for n in (2048, 4096, 8192):
        if "--kv-fp8" in sys.argv:
            probe_kv_fp8(N=n)
        else:
            probe(N=n)
