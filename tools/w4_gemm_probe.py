"""A/B of ``ops.gemm_w4a16`` (int4 codes) against ``ops.linear`` on a bf16 matrix of the same shape -- the route
``w4_rows="decode"`` takes above 32 rows -- on the four Llama-3-8B projection shapes.  Cold weights: each arm is
one graph of ``--mats`` calls on distinct matrices (random codes / values: the timing does not depend on them);
the arms' replays are interleaved in one process after a warm-up.  One JSON line per (shape, M, arm):
median / min / max microseconds per call and TB/s of the weight bytes the arm reads.

    python tools/w4_gemm_probe.py --out profiles/w4_gemm_ab.jsonl [--variants 0 1 4] [--rows 33 64 ...]

``--model``: Llama-3-8B TP = 1 (random weights) in three arms held side by side in one process -- bf16, int4 with
``w4_rows`` decode and all -- decode ms / step at ``--batches`` rows (context ``--ctx``), prefill 1 x 512 and
8 x 512, timed in interleaved rounds after a warm-up (median, min, max), then ``--serve N``: one run per arm of N
requests (128-token prompts, 64 new tokens) through a ``--slots``-slot continuous-batching engine.  Every line
carries the arm's ``layer_weight_bytes`` and the device memory its construction took.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"qkv": (6144, 4096, None), "o": (4096, 4096, None), "gate_up": (28672, 4096, "silu_mul"),
          "down": (4096, 14336, None)}


def graph_of(calls):
    for f in calls:  # warm-up outside the capture (workspaces, counters)
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in calls:
            f()
    return g


def timed(fn) -> float:
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def model_ab(args, out) -> int:
    import time

    import numpy as np

    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B, GenParams, LlamaTP, init_llama_shard
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    dev = torch.device("cuda:0")
    B = max(args.batches + [args.slots, 8])
    arms, meta = {}, {}
    for arm, kw in (("bf16", {}), ("int4_decode", dict(weight_dtype="int4")),
                    ("int4_all", dict(weight_dtype="int4", w4_rows="all"))):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        arms[arm] = LlamaTP(init_llama_shard(LLAMA3_8B, 1, 0, seed=0, device=dev), LLAMA3_8B, backend="fused", device=dev,
                            max_batch=B, max_seq=max(args.ctx + 8, 520), **kw)
        torch.cuda.empty_cache()
        meta[arm] = {"layer_weight_bytes": arms[arm].layer_weight_bytes(),
                     "model_bytes_allocated": torch.cuda.memory_allocated(dev) - before}

    def emit(**kw):
        print(json.dumps({"probe": "w4_model", **kw, **meta[kw["arm"]]}), file=out, flush=True)

    cases = [("prefill", b, 512) for b in (1, 8)] + [("decode", b, args.ctx) for b in args.batches]
    for kind, b, S in cases:
        ids = torch.randint(1000, 100000, (b, S), device=dev, dtype=torch.int32)
        lens = torch.full((b,), S, device=dev, dtype=torch.int32)
        pos = torch.arange(S, device=dev, dtype=torch.int32).unsqueeze(0).expand(b, S).contiguous()
        tok, cur = torch.randint(1000, 100000, (b, 1), device=dev, dtype=torch.int32), lens.view(b, 1).clone()
        n = 1 if kind == "prefill" else 20

        def run(m):
            for _ in range(n):
                m.step(ids, pos, lens, decode=False, k=1) if kind == "prefill" else m.decode_step(tok, cur, 1, max_ctx=S + 1)

        times = {a: [] for a in arms}
        for rep in range(args.reps + 2):
            for a, m in arms.items():  # interleaved
                if rep == 0:
                    m.step(ids, pos, lens, decode=False, k=1)  # fills the cache rows the decode steps attend
                t = timed(lambda: run(m)) / n
                if rep >= 2:
                    times[a].append(t)
        for a, t in times.items():
            emit(arm=a, case=kind, batch=b, tokens=S, ms=round(statistics.median(t), 3), ms_min=round(min(t), 3),
                 ms_max=round(max(t), 3), reps=len(t))
    for a, m in arms.items() if args.serve else ():
        eng = ContinuousLlama(m).start()
        rng = np.random.default_rng(0)
        [f.result() for f in [eng.submit(rng.integers(1000, 100000, 128).tolist(), GenParams(4)) for _ in range(args.slots)]]
        t0 = time.perf_counter()
        futs = [eng.submit(rng.integers(1000, 100000, 128).tolist(), GenParams(64)) for _ in range(args.serve)]
        toks = sum(len(f.result()) for f in futs)
        dt = time.perf_counter() - t0
        eng.stop()
        emit(arm=a, case="serve", slots=args.slots, requests=args.serve, prompt=128, new_tokens=64,
             tokens_per_s=round(toks / dt, 1), runs=1)
    return 0


def main(argv=None) -> int:
    from mlmicroservicetemplate_amd import ops

    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, nargs="+", default=[33, 64, 128, 256, 512, 4096])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--variants", type=int, nargs="+", default=[0], help="gemm_w4a16 tile variants to time")
    ap.add_argument("--mats", type=int, default=32)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", action="store_true", help="the Llama-3-8B three-arm A/B instead of the kernel A/B")
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 64, 128, 256], help="--model: decode rows")
    ap.add_argument("--ctx", type=int, default=128, help="--model: context of the decode steps")
    ap.add_argument("--slots", type=int, default=256, help="--model --serve: engine slots")
    ap.add_argument("--serve", type=int, default=0, help="--model: requests of the serving run (0: none)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    out = open(args.out, "a") if args.out else sys.stdout
    if args.model:
        return model_ab(args, out)
    for name in args.shapes:
        N, K, act = SHAPES[name]
        act = act or ops.ACT_NONE
        wb = [(torch.randn(N, K, device=dev) * K**-0.5).to(torch.bfloat16) for _ in range(args.mats)]
        wq = [torch.randint(0, 256, (N * K // 2,), device=dev, dtype=torch.uint8) for _ in range(args.mats)]
        sc = [(torch.rand(N * K // 128, device=dev) * 0.01 + 0.001).to(torch.bfloat16) for _ in range(args.mats)]
        ws = torch.empty(32 << 20, device=dev, dtype=torch.float32)
        for M in args.rows:
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            arms = {"bf16_linear": graph_of([lambda w=w: ops.linear(x, w, act=act, workspace=ws) for w in wb])}
            for v in args.variants:
                arms[f"w4a16_v{v}"] = graph_of([lambda q=q, s=s: ops.gemm_w4a16(x, q, s, N, act=act, variant=v, workspace=ws)
                                                for q, s in zip(wq, sc)])
            times = {a: [] for a in arms}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for rep in range(args.reps + 3):
                for a, g in arms.items():  # interleaved
                    ev[0].record()
                    g.replay()
                    ev[1].record()
                    ev[1].synchronize()
                    if rep >= 3:
                        times[a].append(ev[0].elapsed_time(ev[1]) * 1e3 / args.mats)
            for a, t in times.items():
                nbytes = N * K * 2 if a == "bf16_linear" else N * K // 2 + N * K // 64
                med = statistics.median(t)
                print(json.dumps({"probe": "w4_gemm", "shape": name, "N": N, "K": K, "M": M, "arm": a, "mats": args.mats,
                                  "us": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                                  "weight_bytes": nbytes, "tb_s": round(nbytes / med / 1e6, 3)}), file=out, flush=True)
        del wb, wq, sc
    return 0


if __name__ == "__main__":
    sys.exit(main())
