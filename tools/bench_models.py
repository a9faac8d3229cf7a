"""Throughput of the BERT (config 3) and Llama-3-8B (config 5) paths on one MI355X.

bert : sequences/s at (batch, seq) through the GpuEngine (hipGraph per bucket), fused kernels
       vs stock PyTorch-ROCm (hipBLASLt + SDPA) on the same random weights.
llama: TP=1 (all of Llama-3-8B on one GPU): prefill tokens/s and decode ms/step at several
       batch sizes with the fused kernels.  ``--speculate K``: also ms per verify step of K + 1 positions
       (both attention routes) interleaved with the decode step, and with ``--spec-accept P`` tokens/s of
       ``generate(speculate=K)`` under a synthetic drafter that is right with probability P.
One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _warm(step, ms):
    """Run ``step`` until ``ms`` of load have passed (the GPU's clocks ramp up over tens of ms of
    load after idling: bench.py's warmup floor, docs/PERF_NOTES.md round 6)."""
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < ms:
        step()
    torch.cuda.synchronize()


def _closed_loop(eng, x, n):
    pend = []
    for _ in range(n):
        pend.append(eng.submit(x))
        if len(pend) >= eng.inflight:
            pend.pop(0).wait()
    for t in pend:
        t.wait()


def synthetic_drafter(prompts, continuations, p_right, vocab, seed=0):
    """A drafter that is right with probability ``p_right`` per draft, for models whose prompt-lookup
    acceptance means nothing (random weights): ``continuations[b]`` is a recorded run from ``prompts[b]``
    (distinct prompts of one length).  Draws are keyed by (seed, sequence, position), so every rerun drafts
    alike; a wrong draft is never the recorded token; a sequence that left its record gets a plain guess."""
    import random

    L = len(prompts[0])
    row = {tuple(p): b for b, p in enumerate(prompts)}
    conts = [list(c) for c in continuations]

    def draft(tokens, n_draft):
        toks = list(tokens)
        b = row.get(tuple(toks[:L]), -1)
        e = len(toks) - L
        if b < 0 or toks[L:] != conts[b][:e]:
            return [toks[-1]] * n_draft
        out = []
        for t in range(n_draft):
            right = conts[b][e + t] if e + t < len(conts[b]) else toks[-1]
            ok = random.Random(seed * 1000003 + b * 10007 + e + t).random() < p_right
            out.append(right if ok else (right + 1) % vocab)
        return out

    return draft


def bench_verify_attn(args):
    """Kernel alone: ``ops.decode_attention_multi`` at T = 2, 3, 4 against ``ops.decode_attention`` (one query,
    matrix-core kernel, no RoPE / append prologue: q and the cache are used as they are) and
    ``ops.flash_attention_ctx`` at S = T.  Hq 32 / Hkv 8; every arm interleaved after a warm floor; us per call
    from events around ``--steps`` back-to-back launches, median and minimum of 5 windows.  The same K / V are
    re-read by every launch, so the numbers are L2-warm."""
    from mlmicroservicetemplate_amd import ops

    dev = torch.device("cuda:0")
    Hq, Hkv, D, N = 32, 8, 128, args.steps

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / N

    for paged in (False, True):
        for B in args.batches:
            for ctx in args.contexts:
                rows = ctx + 64
                g = torch.Generator(device=dev).manual_seed(0)
                table = None
                if paged:
                    pps = rows // 64
                    kc = torch.randn(B * pps + 1, Hkv, 64, D, device=dev, generator=g).to(torch.bfloat16)
                    table = (1 + torch.randperm(B * pps, device=dev, generator=g)).view(B, pps).to(torch.int32)
                else:
                    kc = torch.randn(B, Hkv, rows, D, device=dev, generator=g).to(torch.bfloat16)
                vc = torch.randn_like(kc)
                lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                W = (Hq + 2 * Hkv) * D
                q1 = torch.randn(B, W, device=dev, generator=g).to(torch.bfloat16)
                ws1 = torch.empty(B * Hq * (rows // 64 + 1) * (D + 2), device=dev, dtype=torch.float32)
                o1 = torch.empty(B, Hq * D, device=dev, dtype=torch.bfloat16)
                arms = {"decode_T1": lambda: ops.decode_attention(q1, kc, vc, lens, Hq, Hkv, D, chunk=64, head_major=True,
                                                                  workspace=ws1, out=o1, max_len=ctx, page_table=table)}
                for T in (2, 3, 4):
                    past = torch.full((B,), ctx - T, dtype=torch.int32, device=dev)
                    qT = torch.randn(B * T, W, device=dev, generator=g).to(torch.bfloat16)
                    wsT = torch.empty(B * T * Hq * (rows // 64 + 1) * (D + 2), device=dev, dtype=torch.float32)
                    oT = torch.empty(B * T, Hq * D, device=dev, dtype=torch.bfloat16)
                    oC = torch.empty_like(oT)
                    arms[f"multi_T{T}"] = (lambda T=T, past=past, qT=qT, wsT=wsT, oT=oT: ops.decode_attention_multi(
                        qT, kc, vc, past, lens, B, T, Hq, Hkv, D, page_table=table, max_len=ctx, workspace=wsT, out=oT))
                    arms[f"ctx_S{T}"] = (lambda T=T, past=past, qT=qT, oC=oC: ops.flash_attention_ctx(
                        qT, kc, vc, past, lens, B, T, Hq, Hkv, D, page_table=table, out=oC))
                _warm(lambda: [fn() for fn in arms.values()], args.warm_ms)
                res = {a: [] for a in arms}
                for _ in range(5):
                    for a, fn in arms.items():
                        res[a].append(window(fn))
                print(json.dumps({"bench": "verify_attention_kernel", "Hq": Hq, "Hkv": Hkv, "batch": B, "ctx": ctx,
                                  "paged": paged, "launches_per_window": N,
                                  **{a + "_us": round(sorted(v)[2], 2) for a, v in res.items()},
                                  **{a + "_us_min": round(min(v), 2) for a, v in res.items()}}), flush=True)
                del kc, vc


def bench_bert(args):
    from mlmicroservicetemplate_amd.engine.worker import GpuEngine
    from mlmicroservicetemplate_amd.models import bert

    dev = torch.device("cuda:0")
    cfg = bert.BertConfig()
    p = bert.init_bert(cfg, 0)
    models = {"fused": lambda: bert.BertFused(p, dev, cfg), "eager": lambda: bert.BertEager(p, dev, cfg)}
    models = {k: v() for k, v in models.items() if k in args.backends}
    for S in args.seqs:
        for B in args.batches:
            rng = np.random.default_rng(0)
            toks = [list(rng.integers(1000, 30000, S)) for _ in range(B)]
            packed = bert.pack_requests(toks, S).numpy()
            for name, model in models.items():
                def fwd(x, model=model, S=S, name=name):
                    if name == "fused":  # the serving path (plugins/text_classifier.py): packed rows, fused top-k
                        return model.classify_packed(x, S, 2)
                    ids, tt, lens = bert.unpack_requests(x, S)
                    logits = model(ids, tt, lens)
                    v, i = torch.topk(torch.softmax(logits.float(), -1), 2, dim=-1)
                    return v, i.to(torch.int32)

                eng = GpuEngine(fwd, dev, (2 * S + 1,), torch.int32, buckets=[B], inflight=args.inflight, concurrent=True,
                                cu_partitions=args.cu_partition)
                eng.warmup(capture=True)
                for _ in range(5):
                    eng.run(packed)
                _warm(lambda: _closed_loop(eng, packed, 2 * eng.inflight), args.warm_ms)
                n = args.steps
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pend = []
                for _ in range(n):
                    pend.append(eng.submit(packed))
                    if len(pend) >= eng.inflight:  # a partitioned engine may hold fewer slots
                        pend.pop(0).wait()
                for t in pend:
                    t.wait()
                dt = (time.perf_counter() - t0) / n
                print(json.dumps({"bench": "bert-base", "backend": name, "batch": B, "seq": S, "inflight": eng.inflight,
                                  "cu_partitions": eng.cu_partitions,
                                  "ms_per_batch": round(dt * 1e3, 3), "seq_per_s": round(B / dt, 1),
                                  "tokens_per_s": round(B * S / dt, 1)}), flush=True)
                del eng


def bench_llama_prefix(args):
    """``llama --shared-prefix N --suffix LO HI``: requests of an N-token prefix + a LO..HI-token suffix
    (``--new`` tokens each), ``batches[0]`` of them kept in flight through ``ContinuousLlama`` stepped from
    this process.  Arms, alternating ``--reps`` times on one model: ``off`` (prefix_cache off) with the
    shared prefix; with ``--prefix-cache`` also ``hit`` (on, shared prefix), ``miss`` (on, every prompt its
    own random prefix: what the lookup and the index cost when nothing hits) and ``off_unshared`` (off, the
    ``miss`` arm's prompts) and ``hit_unsplit`` (``hit`` with the suffix attention forced to the unsplit
    kernel: what the split-KV route is worth in service).  Per (arm, rep): time to first token p50 / p99
    (submit -> the iteration that emits it), tokens/s, the pages sequences hold (mean over the iterations)
    and ``ctx_splits_forced``, the forced split count the arm ran under (0: the routing rule)."""
    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B, GenParams, LlamaTP, init_llama_shard
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    dev = torch.device("cuda:0")
    B, N = args.batches[0], args.shared_prefix
    lo, hi = args.suffix[0], args.suffix[-1]
    if not args.kv_pages:
        raise SystemExit("--shared-prefix measures the paged cache: give --kv-pages")
    p = init_llama_shard(LLAMA3_8B, 1, 0, seed=0, device=dev)
    m = LlamaTP(p, LLAMA3_8B, backend="fused", device=dev, max_batch=B, max_seq=args.max_seq, kv_pages=args.kv_pages,
                kv_dtype=args.kv_dtype, weight_dtype=args.weight_dtype,
                kv_prefill=args.kv_prefill)
    del p
    shared = np.random.default_rng(1).integers(1000, 100000, N).tolist()

    def run(arm, n_req, seed):
        on, share = arm in ("hit", "miss", "hit_unsplit"), arm in ("off", "hit", "hit_unsplit")
        forced, m.ctx_splits_forced = m.ctx_splits_forced, 1 if arm == "hit_unsplit" else m.ctx_splits_forced
        rng = np.random.default_rng(seed)
        eng = ContinuousLlama(m, max_queue=1 << 20, prefix_cache=on, prefill_chunk=args.prefill_chunk)
        if on and share:  # the steady state: an earlier request has left the prefix in the index (untimed)
            f = eng.submit(shared + [7], GenParams(1))
            while not f.done():
                eng.run_iteration(eng._leader_admissions())
        left, ttft, held, seen = n_req, [], [], set()
        torch.cuda.synchronize()
        tok0, t0 = eng.tokens, time.perf_counter()
        while left or eng._pending or any(s is not None for s in eng.slots):
            while left and len(eng._pending) + sum(s is not None for s in eng.slots) < B:
                head = shared if share else rng.integers(1000, 100000, N).tolist()
                eng.submit(head + rng.integers(1000, 100000, int(rng.integers(lo, hi + 1))).tolist(), GenParams(args.new))
                left -= 1
            live = [s for s in list(eng._pending) + eng.slots if s is not None]
            eng.run_iteration(eng._leader_admissions())
            now = time.perf_counter()  # the iteration ended in its device -> host read-back
            for s in live:
                if s.out and id(s) not in seen:
                    seen.add(id(s))
                    ttft.append((now - s.t_submit) * 1e3)
            held.append(m.pages.num_pages - 1 - m.pages.free_pages)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = eng.stats()
        rec = {"requests": n_req, "ttft_ms_p50": round(float(np.percentile(ttft, 50)), 2),
               "ttft_ms_p99": round(float(np.percentile(ttft, 99)), 2),
               "tokens_per_s": round((eng.tokens - tok0) / dt, 1), "wall_s": round(dt, 3),
               "pages_held_mean": round(float(np.mean(held)), 1), "pages_held_max": int(max(held)),
               "iterations": eng.iterations, "failures": eng.failures, "dev_mode": bool(eng.dev_mode),
               "ctx_splits_forced": m.ctx_splits_forced,
               **{k: v for k, v in st.items() if k.startswith("prefix")}}
        eng.detach_prefix_cache()  # the next arm's engine takes the model over
        m.ctx_splits_forced = forced
        return rec

    arms = ["off"] + (["hit", "miss", "off_unshared", "hit_unsplit"] if args.prefix_cache else [])
    for arm in arms:  # untimed: graph captures and GEMM algorithm picks for each arm's shapes
        run(arm, B, 99)
    for r in range(args.reps):
        for arm in arms:
            print(json.dumps({"bench": "llama3-8b-prefix-cache", "arm": arm, "rep": r, "in_flight": B,
                              "shared_prefix": N, "suffix": [lo, hi], "new_tokens": args.new,
                              "prefill_chunk": args.prefill_chunk, "kv_pages": args.kv_pages, "max_seq": args.max_seq,
                              **run(arm, args.requests, r)}), flush=True)


def bench_llama(args):
    """``--emulate-tp N``: rank 0's shard of a TP=N model with the collectives stubbed out
    (:class:`ShardEmulationComm`) -- the per-rank kernel time of config 5 on one GPU."""
    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B, LlamaTP, ShardEmulationComm, init_llama_shard

    if args.shared_prefix:
        return bench_llama_prefix(args)
    if args.lora:
        return bench_llama_lora(args)

    dev = torch.device("cuda:0")
    t0 = time.time()
    tp = args.emulate_tp
    p = init_llama_shard(LLAMA3_8B, tp, 0, seed=0, device=dev)
    comm = ShardEmulationComm(tp) if tp > 1 else None
    m = LlamaTP(p, LLAMA3_8B, tp=tp, rank=0, comm=comm, backend="fused", device=dev, max_batch=max(args.batches),
                max_seq=args.max_seq, kv_pages=args.kv_pages, kv_dtype=args.kv_dtype, weight_dtype=args.weight_dtype,
                kv_prefill=args.kv_prefill)
    if m.pages is not None and args.shuffle_pages:  # pages scattered as in a long-running server
        import random

        random.Random(0).shuffle(m.pages._free)
    print(json.dumps({"bench": "llama3-8b", "tp": tp, "collectives": "stubbed" if tp > 1 else "none",
                      "skinny_max_split": args.skinny_max_split, "kv_pages": args.kv_pages, "kv_dtype": args.kv_dtype,
                      "kv_prefill": args.kv_prefill,
                      "weight_dtype": args.weight_dtype, "layer_weight_bytes": m.layer_weight_bytes(),
                      "init_s": round(time.time() - t0, 1)}), flush=True)
    for B in args.batches:
        S = args.prompt
        if m.pages is not None:
            m.pages.reset()
            for b in range(B):
                m.pages.assign(b, S + 1)
        ids = torch.randint(1000, 100000, (B, S), device=dev, dtype=torch.int32)
        lens = torch.full((B,), S, device=dev, dtype=torch.int32)
        pos = torch.arange(S, device=dev, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
        for _ in range(2):
            m.step(ids, pos, lens, decode=False, k=1)
        _warm(lambda: (m.step(ids, pos, lens, decode=False, k=1), torch.cuda.synchronize()), args.warm_ms)
        t1 = time.perf_counter()
        for _ in range(3):
            m.step(ids, pos, lens, decode=False, k=1)
        torch.cuda.synchronize()
        pre = (time.perf_counter() - t1) / 3
        tok = torch.randint(1000, 100000, (B, 1), device=dev, dtype=torch.int32)
        cur = lens.view(B, 1).clone()
        for _ in range(3):
            m.decode_step(tok, cur, 1, max_ctx=S + 1)
        _warm(lambda: (m.decode_step(tok, cur, 1, max_ctx=S + 1), torch.cuda.synchronize()), args.warm_ms)
        t2 = time.perf_counter()
        n = args.steps
        for _ in range(n):
            m.decode_step(tok, cur, 1, max_ctx=S + 1)
        torch.cuda.synchronize()
        dec = (time.perf_counter() - t2) / n
        print(json.dumps({"bench": "llama3-8b", "tp": tp, "batch": B, "prompt": S, "kv_pages": args.kv_pages,
                          "kv_dtype": args.kv_dtype, "kv_prefill": args.kv_prefill, "weight_dtype": args.weight_dtype, "prefill_ms": round(pre * 1e3, 2), "prefill_tok_s": round(B * S / pre, 1),
                          "decode_ms_per_step": round(dec * 1e3, 3), "decode_tok_s": round(B / dec, 1)}), flush=True)
        for K in args.speculate:
            _bench_speculate(m, args, K, B, S, ids, lens, tok, cur)


def bench_llama_lora(args):
    """``--lora N --lora-rank R --lora-mix none same distinct``: Llama-3-8B with N random rank-R q/k/v adapters
    against a model built without ``lora=`` (arm ``plain``: the default path), the arms interleaved ``--reps``
    times in this process (medians).  Decode ms/step per batch, prefill of ``8 x --prompt``, and the two LoRA
    launches of one layer alone (events over 200 calls)."""
    import statistics

    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B, LlamaTP, init_llama_shard, random_lora_adapter

    dev, cfg = torch.device("cuda:0"), LLAMA3_8B
    t0 = time.time()
    p = init_llama_shard(cfg, 1, 0, seed=0, device=dev)
    kw = dict(backend="fused", device=dev, max_batch=max(max(args.batches), 8), max_seq=args.max_seq,
              kv_pages=args.kv_pages, kv_dtype=args.kv_dtype, weight_dtype=args.weight_dtype, kv_prefill=args.kv_prefill)
    plain = LlamaTP(p, cfg, **kw)
    m = LlamaTP(p, cfg, lora={"max_adapters": args.lora, "max_rank": args.lora_rank}, **kw)
    for a in range(args.lora):
        m.load_adapter(a, *random_lora_adapter(cfg, args.lora_rank, seed=100 + a, device=dev))
    head = {"bench": "llama3-8b-lora", "adapters": args.lora, "rank": args.lora_rank, "weight_dtype": args.weight_dtype,
            "kv_dtype": args.kv_dtype, "kv_pages": args.kv_pages}
    print(json.dumps(dict(head, init_s=round(time.time() - t0, 1))), flush=True)
    mixes = {"none": lambda b: -1, "same": lambda b: 0, "distinct": lambda b: b % args.lora}
    arms = [("plain", plain, None)] + [(mix, m, mixes[mix]) for mix in args.lora_mix]

    def set_arm(model, f):
        if f is not None:
            for b in range(model.max_batch):
                model.set_slot_adapter(b, f(b))

    def timed(fn, n):
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n

    S = args.prompt
    for B in args.batches:
        tok = torch.randint(1000, 100000, (B, 1), device=dev, dtype=torch.int32)
        cur = torch.full((B, 1), S, device=dev, dtype=torch.int32)
        res = {name: [] for name, _, _ in arms}
        for rep in range(args.reps + 1):  # round 0 warms every arm (graph capture) and is dropped
            for name, model, f in arms:
                set_arm(model, f)
                step = lambda model=model: model.decode_step(tok, cur, 1, max_ctx=S + 1)  # noqa: E731
                _warm(lambda: (step(), torch.cuda.synchronize()), args.warm_ms if rep else 0)
                dt = timed(step, args.steps)
                if rep:
                    res[name].append(dt * 1e3)
        print(json.dumps(dict(head, what="decode", batch=B, ctx=S, **{f"{k}_ms_per_step": round(statistics.median(v), 4)
                                                                      for k, v in res.items()})), flush=True)
    B = 8
    ids = torch.randint(1000, 100000, (B, S), device=dev, dtype=torch.int32)
    lens = torch.full((B,), S, device=dev, dtype=torch.int32)
    pos = torch.arange(S, device=dev, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
    res = {name: [] for name, _, _ in arms}
    for rep in range(args.reps + 1):
        for name, model, f in arms:
            set_arm(model, f)
            dt = timed(lambda model=model: model.step(ids, pos, lens, decode=False, k=1), 3)
            if rep:
                res[name].append(dt * 1e3)
    print(json.dumps(dict(head, what="prefill", batch=B, prompt=S, **{f"{k}_ms": round(statistics.median(v), 3)
                                                                      for k, v in res.items()})), flush=True)
    # the two launches of one layer alone, every row on its own adapter (distinct) / on adapter 0 (same)
    pack, N = m.lora_pack, m.qkv_width
    for rows_B, rows_S in [(b, 1) for b in args.batches] + [(8, S)]:
        if rows_B > m.max_batch:
            continue
        qkv = torch.randn(rows_B * rows_S, N, device=dev).to(torch.bfloat16)
        r = torch.randn(rows_B * rows_S, cfg.hidden, device=dev).to(torch.bfloat16)
        ns = ops.lora_split(rows_B, rows_S, cfg.hidden, pack.rcap)
        ws = torch.empty(pack.workspace_elems(rows_B * rows_S, ns), device=dev)
        for mix in ("same", "distinct"):
            set_arm(m, mixes[mix])
            out = {}
            for name, fn in (("shrink", lambda: ops.lora_shrink(r, pack, 0, m.lora_slot, rows_B, rows_S, workspace=ws)),
                             ("expand", lambda: ops.lora_expand_(qkv, pack, 0, m.lora_slot, rows_B, rows_S,
                                                                 workspace=ws, eps=cfg.eps))):
                for _ in range(20):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out[f"{name}_us"] = round(e0.elapsed_time(e1) * 1e3 / 200, 2)
            print(json.dumps(dict(head, what="kernels", B=rows_B, S=rows_S, mix=mix, nsplit=ns, **out)), flush=True)


def _bench_speculate(m, args, K, B, S, ids, lens, tok, cur):
    """Verify step (K + 1 positions per sequence) against the decode step, both arms interleaved in this
    process after a warm floor; then, with --spec-accept, generate() with and without speculation."""
    from mlmicroservicetemplate_amd.models.llama import GenParams

    dev = ids.device
    T = K + 1
    m.check_speculate(K)
    if m.pages is not None:
        for b in range(B):
            m.pages.assign(b, S + T)
    feed = torch.randint(1000, 100000, (B, T), device=dev, dtype=torch.int32)
    n = torch.full((B,), T, device=dev, dtype=torch.int32)
    arms = {"decode": lambda: m.decode_step(tok, cur, 1, max_ctx=S + 1)}
    for route in ("multi", "ctx"):  # the verify step's two attention routes (LlamaTP.verify_attn; a graph per route)
        def step(route=route):
            m.verify_attn = route
            return m.verify_step(feed, lens, n, 1, max_ctx=S + T)

        step()
        arms["verify_" + route] = step
    times = {a: [] for a in arms}
    _warm(lambda: [f() for f in arms.values()], args.warm_ms)
    for _ in range(5):  # interleaved windows: a drift of the clocks hits every arm alike
        for a, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            torch.cuda.synchronize()
            times[a].append((time.perf_counter() - t0) / args.steps * 1e3)
    m.verify_attn = "multi"
    med = {a: float(np.median(v)) for a, v in times.items()}
    print(json.dumps({"bench": "llama3-8b-verify", "batch": B, "prompt": S, "T": T, "kv_pages": args.kv_pages,
                      "weight_dtype": args.weight_dtype, "kv_dtype": args.kv_dtype, "kv_prefill": args.kv_prefill,
                      **{a + "_ms": round(v, 3) for a, v in med.items()},
                      **{a + "_ms_min": round(min(times[a]), 3) for a in times},
                      # accepted drafts per step above which a verify step yields more tokens per ms than a decode step
                      "break_even_accepted_per_step": round(med["verify_multi"] / med["decode"] - 1, 3)}), flush=True)
    if args.spec_device:
        _bench_spec_device(m, args, K, B, S, ids, lens)
    if not args.spec_accept:
        return
    if m.pages is not None:
        m.pages.reset()  # generate() assigns its own pages
    gp = GenParams(args.new)
    prompts = [ids[b].tolist() for b in range(B)]
    m.generate(ids, lens, gp)  # warm-up of the plain arm
    # the recorded run the drafter is right about: one token per verify step (every draft a token the step
    # does not pick), i.e. plain decoding's schedule through the verify step's own kernels -- on random
    # weights, where near-ties are everywhere, a record from the single-token route would diverge from what
    # the verify route picks within a few tokens and no draft would ever be "right"
    rec = m.generate(ids, lens, gp, speculate=K, drafter=lambda toks, n: [(toks[-1] + 1) % 100000] * n).tolist()
    arms = {"plain": {}}
    for P in args.spec_accept:
        arms[f"accept_{P}"] = dict(speculate=K, drafter=synthetic_drafter(prompts, rec, P, 100000, seed=0))
    res, stats = {}, {}
    for rnd in range(3):  # round 0 warms every arm's graphs and is dropped
        for name, kw in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(ids, lens, gp, **kw)
            torch.cuda.synchronize()
            if rnd:
                res.setdefault(name, []).append(B * args.new / (time.perf_counter() - t0))
            stats[name] = dict(m.spec_stats)
    for name in arms:
        if name != "plain":
            print(json.dumps({"bench": "llama3-8b-speculate", "batch": B, "prompt": S, "new_tokens": args.new,
                              "speculate": K, "spec_accept": float(name.split("_")[1]), "kv_pages": args.kv_pages,
                              "weight_dtype": args.weight_dtype, "plain_tok_s": round(max(res["plain"]), 1),
                              "speculative_tok_s": round(max(res[name]), 1), **stats[name]}), flush=True)
    if m.pages is not None:
        for b in range(B):
            m.pages.assign(b, S + 1)


def _bench_spec_device(m, args, K, B, S, ids, lens):
    """``--spec-device``: ``generate(speculate=K)`` with the host loop and with the on-device drafter and
    acceptance, and plain ``generate`` -- the default prompt-lookup drafter in both speculative arms, so the same
    tokens and the same acceptance by construction; interleaved in this process after a warm round.  Two prompt
    sets: the random ids (prompt lookup finds nothing: every draft wrong) and a 16-token block repeated."""
    from mlmicroservicetemplate_amd.models.llama import GenParams

    if m.pages is not None:
        m.pages.reset()  # generate() assigns its own pages
    gp = GenParams(args.new)
    rep_ids = ids[:, :16].repeat(1, -(-S // 16))[:, :S].contiguous()
    arms = {"plain": {}, "host": dict(speculate=K), "device": dict(speculate=K, spec_device=True)}
    for kind, x in (("random", ids), ("repeat", rep_ids)):
        res, stats, toks = {}, {}, {}
        for rnd in range(4):  # round 0 warms every arm's graphs and is dropped
            for name, kw in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = m.generate(x, lens, gp, **kw)
                torch.cuda.synchronize()
                if rnd:
                    res.setdefault(name, []).append(B * args.new / (time.perf_counter() - t0))
                stats[name], toks[name] = dict(m.spec_stats), out.to(torch.int32).cpu()
        print(json.dumps({"bench": "llama3-8b-spec-device", "batch": B, "prompt": S, "prompts": kind,
                          "new_tokens": args.new, "speculate": K, "kv_pages": args.kv_pages,
                          "weight_dtype": args.weight_dtype, "kv_dtype": args.kv_dtype,
                          **{a + "_tok_s": round(float(np.median(v)), 1) for a, v in res.items()},
                          **{a + "_tok_s_max": round(max(v), 1) for a, v in res.items()},
                          "host_stats": stats["host"], "device_stats": stats["device"],
                          "same_tokens": bool(torch.equal(toks["host"], toks["device"]))}), flush=True)
    if m.pages is not None:
        for b in range(B):
            m.pages.assign(b, S + 1)


def bench_llama_serve(args):
    """Continuous batching throughput: ``--requests`` generate requests (prompt ``--prompt``,
    ``--new`` tokens each) submitted at once to a ``max_batch = batches[0]`` engine."""
    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B, GenParams, LlamaTP, init_llama_shard
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    dev = torch.device("cuda:0")
    B = args.batches[0]
    p = init_llama_shard(LLAMA3_8B, 1, 0, seed=0, device=dev)
    m = LlamaTP(p, LLAMA3_8B, backend="fused", device=dev, max_batch=B, max_seq=args.max_seq, kv_pages=args.kv_pages,
                kv_dtype=args.kv_dtype, weight_dtype=args.weight_dtype,
                kv_prefill=args.kv_prefill)
    eng = ContinuousLlama(m).start()
    rng = np.random.default_rng(0)
    warm = [eng.submit(rng.integers(1000, 100000, args.prompt).tolist(), GenParams(4)) for _ in range(B)]
    [f.result() for f in warm]
    t0 = time.perf_counter()
    futs = [eng.submit(rng.integers(1000, 100000, args.prompt).tolist(), GenParams(args.new))
            for _ in range(args.requests)]
    lat = []
    for f in futs:
        f.result()
        lat.append(time.perf_counter() - t0)
    dt = time.perf_counter() - t0
    toks = sum(len(f.result()) for f in futs)
    eng.stop()
    print(json.dumps({"bench": "llama3-8b-continuous", "max_batch": B, "kv_pages": args.kv_pages,
                      "kv_dtype": args.kv_dtype, "kv_prefill": args.kv_prefill, "weight_dtype": args.weight_dtype, "requests": args.requests,
                      "prompt": args.prompt, "new_tokens": args.new, "tokens_per_s": round(toks / dt, 1),
                      "requests_per_s": round(args.requests / dt, 2), "p50_latency_s": round(float(np.median(lat)), 3),
                      "iterations": eng.iterations}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", choices=["bert", "llama", "llama-serve", "verify-attn"])
    ap.add_argument("--contexts", type=int, nargs="+", default=[512, 2048, 8192], help="verify-attn: context lengths")
    ap.add_argument("--requests", type=int, default=128)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--seqs", type=int, nargs="+", default=[128])
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warm-ms", type=float, default=200.0, help="untimed load before each timed window (0 = off)")
    ap.add_argument("--inflight", type=int, default=5, help="bert: batches in flight (co-running engine slots)")
    ap.add_argument("--backends", nargs="+", default=["fused", "eager"], help="bert: which implementations")
    ap.add_argument("--emulate-tp", type=int, default=1)
    ap.add_argument("--cu-partition", type=int, default=0,
                    help="bert: CU-masked partitions for the engine slots (engine/worker.py; 0 = off)")
    ap.add_argument("--skinny-max-split", type=int, default=0)
    ap.add_argument("--kv-pages", type=int, default=0, help="llama: paged KV pool of N 64-row pages (0: per-slot)")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="llama: KV cache rows in bf16, or e4m3 with one fp32 scale per (row, KV head)")
    ap.add_argument("--kv-prefill", choices=["rows", "cache"], default="rows",
                    help="llama, --kv-dtype fp8: prefill attends its own bf16 rows, or the e4m3 cache rows (which "
                         "chunked prefill, prefix caching and speculation need)")
    ap.add_argument("--weight-dtype", choices=["bf16", "int4", "w8a8"], default="bf16",
                    help="llama: layer projections in bf16, W4A16 (4-bit codes, one bf16 scale per row and 128 k), or "
                         "W8A8 (e4m3 weights per channel, e4m3 activations per row, block-scaled MFMA)")
    ap.add_argument("--max-seq", type=int, default=2048, help="llama: cache rows per sequence")
    ap.add_argument("--speculate", type=int, nargs="*", default=[],
                    help="llama: also time the verify step of K + 1 positions per sequence (speculative decoding)")
    ap.add_argument("--spec-accept", type=float, nargs="*", default=[],
                    help="llama --speculate: generate() tokens/s with a synthetic drafter right with probability P")
    ap.add_argument("--spec-device", action="store_true",
                    help="llama --speculate: generate() tokens/s, host loop vs on-device drafter + acceptance vs plain")
    ap.add_argument("--shuffle-pages", action="store_true", help="llama: hand out pages in random order")
    ap.add_argument("--shared-prefix", type=int, default=0,
                    help="llama: serve requests that share an N-token prefix (time to first token, tokens/s)")
    ap.add_argument("--suffix", type=int, nargs="+", default=[32, 128], help="llama --shared-prefix: suffix tokens LO HI")
    ap.add_argument("--prefix-cache", action="store_true", help="llama --shared-prefix: add the prefix_cache arms")
    ap.add_argument("--prefill-chunk", type=int, default=0, help="llama --shared-prefix: chunked prefill width")
    ap.add_argument("--lora", type=int, default=0, help="llama: N random LoRA adapters on q/k/v (0: off)")
    ap.add_argument("--lora-rank", type=int, default=16, help="llama --lora: their rank")
    ap.add_argument("--lora-mix", nargs="+", choices=["none", "same", "distinct"], default=["none", "same", "distinct"],
                    help="llama --lora: slots on the base model / all on adapter 0 / slot b on adapter b %% N")
    ap.add_argument("--reps", type=int, default=3, help="llama --shared-prefix: alternations of the arms")
    args = ap.parse_args()
    if args.skinny_max_split:
        from mlmicroservicetemplate_amd.ops import _lib

        _lib.lib().mls_skinny_set_max_split(args.skinny_max_split)
    {"bert": bench_bert, "llama": bench_llama, "llama-serve": bench_llama_serve,
     "verify-attn": bench_verify_attn}[args.which](args)


if __name__ == "__main__":
    main()
