"""Decode attention on the bf16 cache vs on the FP8 (e4m3) cache, graph-timed, alternating arms.

Llama-3-8B TP=1 head geometry (32 q heads, 8 kv heads, D=128), head-major caches, rope/append mode
as the model's decode step runs it, the split the model picks (64 rows below batch 32, 128 from
there).  One JSON line per (batch, context, arm): the median of ``--reps`` alternating timings, their
spread, and the achieved KV bytes/s -- bytes counted from the shapes: K and V rows read once
(+ the fp32 scales for fp8).  ``--flush-mb N`` evicts the L2s between calls (ops.autotune).

    python tools/kv_fp8_probe.py --out profiles/kv_fp8_decode_ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kv_bytes(B: int, L: int, Hkv: int, D: int, fp8: bool) -> int:
    """bytes of cache the attention has to read: K and V rows of every sequence, once"""
    return B * L * Hkv * 2 * ((D + 4) if fp8 else D * 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 128])
    ap.add_argument("--contexts", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--flush-mb", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.flush_mb:
        os.environ["MLS_TUNE_FLUSH_MB"] = str(args.flush_mb)

    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.ops import reference as R
    from mlmicroservicetemplate_amd.ops.autotune import _time

    if not torch.cuda.is_available():
        raise SystemExit("kv_fp8_probe: needs the GPU (no CPU fallback for a timing)")
    dev = torch.device("cuda:0")
    Hq, Hkv, D = 32, 8, 128
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for L in args.contexts:
        cos, sin = R.rope_tables(L, D, 500000.0, dev)
        for B in args.batches:
            chunk = 128 if B >= 32 else 64
            g = torch.Generator(device=dev).manual_seed(B * 100003 + L)
            kc = torch.randn(B, Hkv, L, D, device=dev, generator=g).to(torch.bfloat16)
            vc = torch.randn(B, Hkv, L, D, device=dev, generator=g).to(torch.bfloat16)
            k8, ks = R.kv_quant_fp8(kc)
            v8, vs = R.kv_quant_fp8(vc)
            qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
            lens = torch.full((B,), L, device=dev, dtype=torch.int32)
            pos = lens - 1
            ws = torch.empty(B * Hq * (-(-L // chunk)) * (D + 2), device=dev)
            cnt = torch.zeros(B * Hkv, device=dev, dtype=torch.int32)
            out = torch.empty(B, Hq * D, device=dev, dtype=torch.bfloat16)
            kw = dict(chunk=chunk, workspace=ws, counters=cnt, out=out, positions=pos, cos=cos, sin=sin, max_len=L)
            arms = {
                "bf16": lambda: ops.decode_attention(qkv, kc, vc, lens, Hq, Hkv, D, head_major=True, impl="mfma", **kw),
                "fp8": lambda: ops.decode_attention_fp8(qkv, k8, v8, ks, vs, lens, Hq, Hkv, D, **kw),
            }
            # results must not change beyond the quantisation: the two arms on the same rows
            o16 = arms["bf16"]().float().clone()
            o8 = arms["fp8"]().float().clone()
            dev_rel = ((o8 - o16).abs().max() / o16.abs().max()).item()
            times = {a: [] for a in arms}
            for _ in range(args.reps):  # alternate the arms
                for a, fn in arms.items():
                    times[a].append(_time(fn, iters=args.iters) * 1e3)  # us
            for a in arms:
                t = statistics.median(times[a])
                nbytes = kv_bytes(B, L, Hkv, D, a == "fp8")
                emit({"probe": "decode_attention", "kv_dtype": a, "B": B, "L": L, "chunk": chunk, "rope": True,
                      "flush_mb": args.flush_mb, "us": round(t, 2), "us_min": round(min(times[a]), 2),
                      "us_max": round(max(times[a]), 2), "reps": args.reps, "kv_bytes": nbytes,
                      "kv_gb_s": round(nbytes / (t * 1e-6) / 1e9, 1), "fp8_vs_bf16_out_rel": round(dev_rel, 5)})
            del kc, vc, k8, v8, ks, vs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
