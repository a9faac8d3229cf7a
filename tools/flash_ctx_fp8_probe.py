"""Context attention (the chunk path) on the bf16 cache vs on the FP8 (e4m3) cache, graph-timed,
alternating arms: ``ops.flash_attention_ctx`` against ``ops.flash_attention_ctx_fp8``.

Llama-3-8B TP=1 head geometry (32 q heads, 8 kv heads, D=128), paged head-major caches with a shuffled
page table, the shapes of the prefix-caching table (docs/PERF_NOTES.md): 1 x 16..64 queries against 4 k
and 16 k cached rows, 8 x 64 against 4 k, and 8 x 512 at past = 0; each with the split count
``LlamaTP.ctx_split_rule`` routes it to.  One JSON line per (shape, arm): the median of ``--reps``
alternating timings, their spread, and the achieved bytes/s of cache rows -- bytes counted from the
shapes: the K and V rows below lens read once (+ the fp32 scales for fp8); the re-reads by the other
query heads of a KV group and by further query tiles are not counted.

    python tools/flash_ctx_fp8_probe.py --out profiles/kv_fp8_ctx_ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1, 16, 4096), (1, 32, 4096), (1, 64, 4096), (1, 16, 16384), (1, 32, 16384), (1, 64, 16384),
          (8, 64, 4096), (8, 512, 0)]  # (B, S, past)


def kv_bytes(B: int, L: int, Hkv: int, D: int, fp8: bool) -> int:
    return B * L * Hkv * 2 * ((D + 4) if fp8 else D * 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.models.llama import LlamaTP
    from mlmicroservicetemplate_amd.ops import reference as R
    from mlmicroservicetemplate_amd.ops.autotune import _time

    if not torch.cuda.is_available():
        raise SystemExit("flash_ctx_fp8_probe: needs the GPU (no CPU fallback for a timing)")
    dev = torch.device("cuda:0")
    Hq, Hkv, D = 32, 8, 128
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for B, S, P in SHAPES:
        L = P + S
        pps = -(-L // 64)
        pages = B * pps + 1
        g = torch.Generator(device=dev).manual_seed(B * 100003 + L)
        kp = torch.randn(pages, Hkv, 64, D, device=dev, generator=g).to(torch.bfloat16)
        vp = torch.randn(pages, Hkv, 64, D, device=dev, generator=g).to(torch.bfloat16)
        k8, ks = R.kv_quant_fp8(kp)
        v8, vs = R.kv_quant_fp8(vp)
        table = (1 + torch.randperm(pages - 1, device=dev, generator=g)).view(B, pps).to(torch.int32)
        qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
        past = torch.full((B,), P, device=dev, dtype=torch.int32)
        lens = past + S
        out = torch.empty(B * S, Hq * D, device=dev, dtype=torch.bfloat16)
        splits = LlamaTP.ctx_split_rule(B, S, Hq, L)
        kw = dict(page_table=table, out=out)
        if splits > 1:
            kw.update(splits=splits, max_ctx=L,
                      workspace=torch.empty(ops.flash_ctx_workspace_elems(B, S, Hq, D, splits), device=dev))
        arms = {
            "bf16": lambda: ops.flash_attention_ctx(qkv, kp, vp, past, lens, B, S, Hq, Hkv, D, **kw),
            "fp8": lambda: ops.flash_attention_ctx_fp8(qkv, k8, v8, ks, vs, past, lens, B, S, Hq, Hkv, D, **kw),
        }
        o16 = arms["bf16"]().float().clone()
        o8 = arms["fp8"]().float().clone()
        dev_rel = ((o8 - o16).abs().max() / o16.abs().max()).item()
        for fn in arms.values():  # warm clocks and caches before the first timed repetition
            _time(fn, iters=args.iters)
        times = {a: [] for a in arms}
        for _ in range(args.reps):  # alternate the arms
            for a, fn in arms.items():
                times[a].append(_time(fn, iters=args.iters) * 1e3)  # us
        for a in arms:
            t = statistics.median(times[a])
            nbytes = kv_bytes(B, L, Hkv, D, a == "fp8")
            emit({"probe": "flash_attention_ctx", "kv_dtype": a, "B": B, "S": S, "past": P, "splits": splits,
                  "us": round(t, 2), "us_min": round(min(times[a]), 2), "us_max": round(max(times[a]), 2),
                  "reps": args.reps, "kv_bytes": nbytes, "kv_gb_s": round(nbytes / (t * 1e-6) / 1e9, 1),
                  "fp8_vs_bf16_out_rel": round(dev_rel, 5)})
        del kp, vp, k8, v8, ks, vs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
