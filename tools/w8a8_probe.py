"""A/B of ``weight_dtype="w8a8"`` against the bf16 routes, both arms in one process and interleaved.

``kernel``: the four Llama-3-8B TP = 1 layer projections (qkv, o, gate_up + SiLU-mul, down) at M = 16 .. 4096:
``ops.gemm_w8a8`` alone, ``ops.quant_rows_fp8 + ops.gemm_w8a8``, and what the bf16 model runs at that row
count (``ops.skinny_packed`` on the granule-packed copy up to 24 rows, ``ops.linear`` above).  us per call from
device events around back-to-back launches, median and minimum of 5 interleaved windows, and TFLOP/s of the
median.  Up to 256 rows every arm rotates over enough copies of its weights to exceed the 256 MB infinity cache,
so the weight stream comes from HBM as in a model step; above, one copy (compute-bound).

``model``: ``LlamaTP`` (Llama-3-8B, TP = 1, random weights) with bf16 and with w8a8 weights side by side: prefill
at ``--prefill B`` x 512 tokens and ms per decode step at ``--batches``, interleaved windows.

One JSON line per measurement on stdout (kept in profiles/w8a8_ab.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}  # N, K
CACHE_BYTES = 600 << 20


def _warm(fn, ms):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        fn()
        torch.cuda.synchronize()


def _window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _ab(arms, warm_ms, windows=5):
    """us per call of every arm: ``windows`` interleaved windows of >= ~20 ms each after a warm floor."""
    _warm(lambda: [f() for f in arms.values()], warm_ms)
    n = {a: max(10, min(400, int(2e4 / max(_window(f, 5), 1.0)))) for a, f in arms.items()}
    times = {a: [] for a in arms}
    for _ in range(windows):
        for a, f in arms.items():
            times[a].append(_window(f, n[a]))
    return {a: (float(np.median(v)), float(min(v))) for a, v in times.items()}


def bench_kernel(args):
    from mlmicroservicetemplate_amd import ops

    dev = torch.device("cuda:0")
    ws = torch.empty(32 << 20, device=dev, dtype=torch.float32)
    for name in args.projections:
        N, K = SHAPES[name]
        act = ops.ACT_SILU_MUL if name == "gate_up" else ops.ACT_NONE
        torch.manual_seed(0)
        w = (torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16)
        wq, wsc = ops.pack_w8(w)
        for M in args.rows:
            stream = M <= 256
            n16 = -(-CACHE_BYTES // (N * K * 2)) if stream else 1
            n8 = -(-CACHE_BYTES // (N * K)) if stream else 1
            packed = M <= 24
            w16 = [ops.pack_skinny(w) if packed else w.clone() for _ in range(n16)]
            w8 = [wq.clone() for _ in range(n8)]
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            xq, xs = ops.quant_rows_fp8(x)
            it = {"b": 0, "g": 0, "q": 0}

            def bf16():
                it["b"] += 1
                wt = w16[it["b"] % n16]
                if packed:
                    return ops.skinny_packed(x, wt, N, act=act)
                return ops.linear(x, wt, act=act, workspace=ws)

            def gemm():
                it["g"] += 1
                return ops.gemm_w8a8(xq, xs, w8[it["g"] % n8], wsc, N, act=act, variant=args.variant, workspace=ws)

            def quant_gemm():
                it["q"] += 1
                q, s = ops.quant_rows_fp8(x)
                return ops.gemm_w8a8(q, s, w8[it["q"] % n8], wsc, N, act=act, variant=args.variant, workspace=ws)

            res = _ab({"bf16": bf16, "gemm_w8a8": gemm, "quant_gemm_w8a8": quant_gemm}, args.warm_ms)
            flop = 2.0 * M * N * K
            line = {"bench": "w8a8-kernel", "proj": name, "M": M, "N": N, "K": K, "variant": args.variant,
                    "bf16_route": "skinny_packed" if packed else "linear", "weights_from": "hbm" if stream else "cache"}
            for a, (med, mn) in res.items():
                line[a + "_us"] = round(med, 2)
                line[a + "_us_min"] = round(mn, 2)
                line[a + "_tflops"] = round(flop / med / 1e6, 1)
            line["speedup_gemm"] = round(res["bf16"][0] / res["gemm_w8a8"][0], 3)
            line["speedup_quant_gemm"] = round(res["bf16"][0] / res["quant_gemm_w8a8"][0], 3)
            print(json.dumps(line), flush=True)
            del w16, w8


def bench_model(args):
    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B, LlamaTP, init_llama_shard

    dev = torch.device("cuda:0")
    t0 = time.time()
    p = init_llama_shard(LLAMA3_8B, 1, 0, seed=0, device=dev)
    B_max = max(args.batches + args.prefill)
    models = {wd: LlamaTP(dict(p), LLAMA3_8B, backend="fused", device=dev, max_batch=B_max, max_seq=args.max_seq,
                          weight_dtype=wd) for wd in ("bf16", "w8a8")}
    del p
    print(json.dumps({"bench": "w8a8-model", "init_s": round(time.time() - t0, 1),
                      **{wd + "_layer_weight_bytes": m.layer_weight_bytes() for wd, m in models.items()}}), flush=True)
    S = args.prompt
    for B in args.prefill:
        ids = torch.randint(1000, 100000, (B, S), device=dev, dtype=torch.int32)
        lens = torch.full((B,), S, device=dev, dtype=torch.int32)
        pos = torch.arange(S, device=dev, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
        arms = {wd: (lambda m=m: m.step(ids, pos, lens, decode=False, k=1)) for wd, m in models.items()}
        res = _ab(arms, args.warm_ms)
        print(json.dumps({"bench": "w8a8-model", "phase": "prefill", "batch": B, "prompt": S,
                          **{wd + "_ms": round(v[0] / 1e3, 3) for wd, v in res.items()},
                          **{wd + "_ms_min": round(v[1] / 1e3, 3) for wd, v in res.items()},
                          **{wd + "_tok_s": round(B * S / v[0] * 1e6, 1) for wd, v in res.items()},
                          "speedup": round(res["bf16"][0] / res["w8a8"][0], 3)}), flush=True)
    for B in args.batches:
        lens = torch.full((B,), S, device=dev, dtype=torch.int32)
        tok =torch.randint(1000, 100000, (B, 1), device=dev, dtype=torch.int32)
        cur = lens.view(B, 1).clone()
        for m in models.values():  # the cache rows are whatever they hold: a step's time does not depend on them
            for _ in range(3):
                m.decode_step(tok, cur, 1, max_ctx=S + 1)
        arms = {wd: (lambda m=m: m.decode_step(tok, cur, 1, max_ctx=S + 1)) for wd, m in models.items()}
        res = _ab(arms, args.warm_ms)
        print(json.dumps({"bench": "w8a8-model", "phase": "decode", "batch": B, "context": S,
                          **{wd + "_ms_per_step": round(v[0] / 1e3, 3) for wd, v in res.items()},
                          **{wd + "_ms_per_step_min": round(v[1] / 1e3, 3) for wd, v in res.items()},
                          "speedup": round(res["bf16"][0] / res["w8a8"][0], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("which", choices=["kernel", "model"])
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 32, 128, 256, 512, 4096])
    ap.add_argument("--projections", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--variant", type=int, default=0, help="kernel: force a gemm_w8a8 tile (0: the launcher's pick)")
    ap.add_argument("--prefill", type=int, nargs="*", default=[1, 8], help="model: prefill batches of --prompt tokens")
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 32, 128], help="model: decode batch sizes")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--max-seq", type=int, default=1024)
    ap.add_argument("--warm-ms", type=float, default=200.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8a8_probe measures on the GPU: none found")
    (bench_kernel if args.which == "kernel" else bench_model)(args)


if __name__ == "__main__":
    main()
