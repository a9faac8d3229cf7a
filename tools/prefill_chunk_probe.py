"""Chunked prefill, measured: the context-attention kernel alone, and /generate serving with it.

``kernel``: ``ops.flash_attention_ctx`` (K / V from the cache, per-slot and paged) against
``ops.flash_attention`` (K / V from the fused qkv) at the Llama-3-8B TP = 1 heads (32 / 8, D = 128),
B x S queries at ``--pasts`` rows of context.  Graph-timed (``ops.autotune._time``), the arms
alternating ``--reps`` times; one JSON line per (past, arm) with the median us and the achieved
TFLOP/s -- FLOPs counted from the shapes: 4 D per (query, visible key, q head), causal.
``--batch`` / ``--seq`` take several values (small S: the shape a prefix-cache hit leaves); with
``--splits n ...`` the arms are the paged unsplit kernel and its split-KV launch (combine included) at
each n -- the table ``LlamaTP.ctx_splits`` is set from (docs/PERF_NOTES.md "Prefix caching").

``serve``: Llama-3-8B (random weights) behind ``ContinuousLlama`` with ``--slots`` slots kept full of
short requests while a ``--long``-token prompt arrives every ``--every`` iterations.  The scheduler
loop is stepped from this process, each iteration timed on the host clock (an iteration ends in its
device -> host read-back).  One engine per ``--chunks`` value on the same model, the arms alternating
``--reps`` times over the same seeded arrivals; one JSON line per (chunk, rep) with the iteration-time
distribution and tokens/s.

    python tools/prefill_chunk_probe.py kernel --out profiles/prefill_chunk_ab.jsonl
    python tools/prefill_chunk_probe.py serve --out profiles/prefill_chunk_ab.jsonl
    python tools/prefill_chunk_probe.py kernel --batch 1 8 --seq 16 64 256 --pasts 1024 4096 16384 \
        --splits 2 4 8 16 --out profiles/prefix_cache_ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def attn_flops(B: int, S: int, past: int, Hq: int, D: int) -> int:
    """QK^T and PV of causal attention: query i of a row sees past + i + 1 keys"""
    return 4 * D * Hq * B * (S * past + S * (S + 1) // 2)


def _emitter(path):
    sink = open(path, "a") if path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    return emit


def kernel(args):
    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.ops import reference as R
    from mlmicroservicetemplate_amd.ops.autotune import _time

    dev = torch.device("cuda:0")
    emit = _emitter(args.out)
    for B in args.batch:
        for S in args.seq:
            for past in args.pasts:
                _kernel_case(args, ops, R, _time, emit, dev, B, S, past)


def _kernel_case(args, ops, R, _time, emit, dev, B, S, past):
    Hq, Hkv, D = 32, 8, 128
    L = past + S
    g = torch.Generator(device=dev).manual_seed(L)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
    kc = torch.randn(B, Hkv, L, D, device=dev, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, L, D, device=dev, generator=g).to(torch.bfloat16)
    _q, k, v = R.split_qkv(qkv, Hq, Hkv, D)  # the chunk's own rows, as rope_kv_ appends them
    kc[:, :, past:] = k.view(B, S, Hkv, D).transpose(1, 2)
    vc[:, :, past:] = v.view(B, S, Hkv, D).transpose(1, 2)
    pps = -(-L // 64)
    table = (1 + torch.randperm(B * pps, device=dev, generator=g)).view(B, pps).to(torch.int32)
    kp = torch.zeros(B * pps + 1, Hkv, 64, D, device=dev, dtype=torch.bfloat16)
    vp = torch.zeros_like(kp)
    pad = pps * 64 - L
    kp[table.long().view(-1)] = torch.nn.functional.pad(kc, (0, 0, 0, pad)).view(B, Hkv, pps, 64, D).transpose(
        1, 2).reshape(B * pps, Hkv, 64, D)
    vp[table.long().view(-1)] = torch.nn.functional.pad(vc, (0, 0, 0, pad)).view(B, Hkv, pps, 64, D).transpose(
        1, 2).reshape(B * pps, Hkv, 64, D)
    pst = torch.full((B,), past, device=dev, dtype=torch.int32)
    lens = torch.full((B,), L, device=dev, dtype=torch.int32)
    out = torch.empty(B * S, Hq * D, device=dev, dtype=torch.bfloat16)
    arms = {
        "ctx": lambda: ops.flash_attention_ctx(qkv, kc, vc, pst, lens, B, S, Hq, Hkv, D, out=out),
        "ctx_paged": lambda: ops.flash_attention_ctx(qkv, kp, vp, pst, lens, B, S, Hq, Hkv, D, page_table=table,
                                                     out=out),
    }
    o_ctx = arms["ctx"]().float().clone()
    paged_equal = bool(torch.equal(arms["ctx_paged"]().float(), o_ctx))
    split_rel = {}
    if args.splits:  # the sweep: the paged unsplit kernel (the baseline) against its split-KV launches
        del arms["ctx"]
        for n in args.splits:
            ws = torch.empty(ops.flash_ctx_workspace_elems(B, S, Hq, D, n), device=dev, dtype=torch.float32)
            arms[f"ctx_paged_split{n}"] = (lambda n=n, ws=ws: ops.flash_attention_ctx(
                qkv, kp, vp, pst, lens, B, S, Hq, Hkv, D, page_table=table, out=out, splits=n, max_ctx=L,
                workspace=ws))
            o_n = arms[f"ctx_paged_split{n}"]().float()
            split_rel[f"ctx_paged_split{n}"] = round(((o_n - o_ctx).abs().max() / o_ctx.abs().max()).item(), 5)
    rel_one = None
    if past == 0:  # the baseline exists only here: the one-shot kernel has no context to read
        arms["flash_attention"] = lambda: ops.flash_attention(qkv, B, S, Hq, Hkv, D, causal=True, out=out)
        o_one = arms["flash_attention"]().float().clone()
        rel_one = ((o_ctx - o_one).abs().max() / o_one.abs().max()).item()
    times = {a: [] for a in arms}
    for _ in range(args.reps):  # alternate the arms
        for a, fn in arms.items():
            times[a].append(_time(fn, iters=args.iters) * 1e3)  # us
    fl = attn_flops(B, S, past, Hq, D)
    for a in arms:
        t = statistics.median(times[a])
        emit({"probe": "flash_attention_ctx", "arm": a, "B": B, "S": S, "past": past, "Hq": Hq, "Hkv": Hkv,
              "us": round(t, 2), "us_min": round(min(times[a]), 2), "us_max": round(max(times[a]), 2),
              "reps": args.reps, "flops": fl, "tflops": round(fl / (t * 1e-6) / 1e12, 1),
              "paged_equals_per_slot": paged_equal, "split_vs_unsplit_rel": split_rel.get(a),
              "ctx_vs_flash_attention_rel": None if rel_one is None else round(rel_one, 5)})
    del kc, vc, kp, vp
    torch.cuda.empty_cache()


def serve(args):
    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B, GenParams, LlamaTP, init_llama_shard
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    dev = torch.device("cuda:0")
    emit = _emitter(args.out)
    B = args.slots
    p = init_llama_shard(LLAMA3_8B, 1, 0, seed=0, device=dev)
    m = LlamaTP(p, LLAMA3_8B, backend="fused", device=dev, max_batch=B, max_seq=args.max_seq, kv_pages=args.kv_pages)
    del p

    def run(chunk: int, iters: int, timed: bool):
        """``iters`` scheduler iterations over seeded arrivals: the queue is topped up with short
        requests (prompt 32..256, 32..160 new tokens) so the slots stay full, and one long prompt
        joins it every ``--every`` iterations (the first after the initial fill)."""
        rng = np.random.default_rng(7)
        eng = ContinuousLlama(m, max_queue=1 << 20, prefill_chunk=chunk)
        futs, dts = [], []
        tok0 = t_all = 0
        for i in range(iters + args.warm_iters):
            if i % args.every == args.every - 1:  # not with the initial fill: B x long padded rows in one forward
                futs.append(eng.submit(rng.integers(1000, 100000, args.long).tolist(), GenParams(32)))
            while len(eng._pending) + sum(s is not None for s in eng.slots) < B + 8:
                futs.append(eng.submit(rng.integers(1000, 100000, int(rng.integers(32, 257))).tolist(),
                                       GenParams(int(rng.integers(32, 161)))))
            if i == args.warm_iters:
                torch.cuda.synchronize()
                tok0, t_all = eng.tokens, time.perf_counter()
            t0 = time.perf_counter()
            eng.run_iteration(eng._leader_admissions())
            if i >= args.warm_iters:
                dts.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t_all = time.perf_counter() - t_all
        toks = eng.tokens - tok0
        # drain: every slot retires before the next arm starts on this model
        for f in futs:
            f.cancel()
        eng._pending.clear()
        while any(s is not None for s in eng.slots):
            eng.run_iteration([])
        if not timed:
            return None
        d = np.array(dts)
        return {"iters": iters, "iter_ms_p50": round(float(np.percentile(d, 50)), 3),
                "iter_ms_p90": round(float(np.percentile(d, 90)), 3), "iter_ms_p99": round(float(np.percentile(d, 99)), 3),
                "iter_ms_max": round(float(d.max()), 3), "iter_ms_mean": round(float(d.mean()), 3),
                "tokens": int(toks), "tokens_per_s": round(toks / t_all, 1), "dev_mode": bool(eng.dev_mode),
                "failures": eng.failures}

    for chunk in args.chunks:  # untimed: graph captures, GEMM algorithm picks for the shapes of each arm
        run(chunk, args.iters // 2, False)
    for rep in range(args.reps):  # alternate the arms
        for chunk in args.chunks:
            rec = run(chunk, args.iters, True)
            emit({"bench": "llama3-8b-continuous-long-prompts", "prefill_chunk": chunk, "rep": rep, "slots": B,
                  "long_prompt": args.long, "long_every_iters": args.every, "kv_pages": args.kv_pages,
                  "max_seq": args.max_seq, "warm_iters": args.warm_iters, **rec})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("which", choices=["kernel", "serve"])
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="kernel: calls per timing; serve: timed iterations per run")
    ap.add_argument("--batch", type=int, nargs="+", default=[8])
    ap.add_argument("--seq", type=int, nargs="+", default=[512])
    ap.add_argument("--splits", type=int, nargs="*", default=[], help="kernel: split-KV arms at these split counts")
    ap.add_argument("--pasts", type=int, nargs="+", default=[0, 512, 2048, 7680])
    ap.add_argument("--chunks", type=int, nargs="+", default=[0, 256, 512, 1024])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--long", type=int, default=4096)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--warm-iters", type=int, default=100)
    ap.add_argument("--max-seq", type=int, default=4352)
    ap.add_argument("--kv-pages", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefill_chunk_probe: needs the GPU (no CPU fallback for a timing)")
    {"kernel": kernel, "serve": serve}[args.which](args)


if __name__ == "__main__":
    main()
