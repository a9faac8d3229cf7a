"""Child process for test_llama_tp_gpu.py: one TP rank of the fused (native-kernel) Llama; all
ranks share cuda:0 and talk over gloo (host-staged collectives)."""
import json
import os
import sys

import torch
import torch.distributed as dist


def serve(m, rank, world, cfg):
    """MODE=serve: the /generate serving path -- ContinuousLlama on every rank, rank 0 scheduling
    and publishing admissions (plugins/llm.py control channel / follower_loop), the device-
    resident iterations; counts the device -> host copies the iterations make.  STALL_RANK: that
    rank's stream stalls before its first decode step (the peers' one-shot waits time out): every
    in-flight request must fail with TPCommError, none may return tokens."""
    import types

    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.models.llama import GenParams
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    plug = LlamaPlugin()
    plug.model = m
    plug.comm_dev = torch.device("cpu")  # gloo
    plug.ctx = types.SimpleNamespace(rank=rank)
    eng = ContinuousLlama(m, channel=plug)
    plug.engine = eng
    stall_rank = int(os.environ.get("STALL_RANK", "-1"))
    if rank == stall_rank:
        if m.comm.car is not None and os.environ.get("MLS_AR_TIMEOUT_ITERS_STALL"):
            m.comm.car.timeout = int(os.environ["MLS_AR_TIMEOUT_ITERS_STALL"])
        orig_iter = eng.iteration
        state = {"n": 0}

        def stalled(admit):
            if state["n"] == 1:  # the first pure decode iteration
                ops.gpu_sleep(int(os.environ.get("STALL_US", "300000")))
            state["n"] += 1
            return orig_iter(admit)

        eng.iteration = stalled
    elif stall_rank >= 0 and m.comm.car is not None and os.environ.get("MLS_AR_TIMEOUT_ITERS_STALL"):
        m.comm.car.timeout = int(os.environ["MLS_AR_TIMEOUT_ITERS_STALL"])
    calls = []
    orig = torch.Tensor.cpu

    def counting_cpu(self, *a, **kw):
        if self.is_cuda:
            calls.append(tuple(self.shape))
        return orig(self, *a, **kw)

    torch.Tensor.cpu = counting_cpu
    results = []
    reqs = []
    try:
        if rank == 0:
            g = torch.Generator().manual_seed(11)
            # SERVE_NREQ requests of SERVE_MAXNEW + (i % SERVE_SPREAD) new tokens each (the TP=8 case
            # runs 12 of 10-16 tokens through the 4 slots: admissions keep arriving while others decode)
            nreq, base, spread = (int(os.environ.get(k, d)) for k, d in
                                  (("SERVE_NREQ", "6"), ("SERVE_MAXNEW", "6"), ("SERVE_SPREAD", "3")))
            for i in range(nreq):
                n = int(torch.randint(3, 30, (1,), generator=g))
                reqs.append((torch.randint(3, cfg.vocab - 1, (n,), generator=g).tolist(),
                             GenParams(max_new_tokens=base + i % spread, top_k=[1, 8][i % 2], temperature=0.8,
                                       seed=i)))
            eng.start()
            futs = [eng.submit(ids, gp) for ids, gp in reqs]
            for f in futs:
                try:
                    results.append(f.result(timeout=200))
                except Exception as e:  # noqa: BLE001
                    results.append(type(e).__name__)
            eng.stop()  # announces STOP to the followers
        else:
            plug.follower_loop()
    finally:
        torch.Tensor.cpu = orig
    info = {"iterations": eng.iterations, "host_reads": eng.host_reads, "cpu_calls": len(calls),
            "dev_mode": int(eng.dev_mode), "failures": eng.failures, "car": int(m.comm.car is not None),
            "follower": getattr(plug, "follower_stats", None), "proto": eng.proto}
    reqs_json = json.dumps([[ids, [gp.max_new_tokens, gp.top_k, gp.temperature, gp.seed]] for ids, gp in reqs]
                           if rank == 0 else [])
    torch.save({"results": json.dumps(results), "info": json.dumps(info), "reqs": reqs_json},
               os.environ["OUT"] + f".serve.{rank}.pt")


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, TPComm, init_llama_shard, tiny_config

    cfg = tiny_config(**json.loads(os.environ["TP_CFG"]))
    p = init_llama_shard(cfg, world, rank, seed=3, device="cuda")
    m = LlamaTP(p, cfg, tp=world, rank=rank, comm=TPComm(None, world, device="cuda"), backend="fused",
                device="cuda", max_batch=4, max_seq=256)
    if os.environ.get("MODE") == "serve":
        serve(m, rank, world, cfg)
        dist.destroy_process_group()
        return 0
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, cfg.vocab - 1, (3, 24), generator=g)
    lens = torch.tensor([24, 11, 3])
    pos = torch.arange(24, dtype=torch.int32).unsqueeze(0).expand(3, 24).contiguous().cuda()
    for c in m.k_cache + m.v_cache:
        c.zero_()
    vals, idx = m.step(ids.cuda(), pos, lens.cuda(), decode=False, k=8)
    allv = m.comm.all_gather(vals)
    alli = m.comm.all_gather(idx)
    kv_over = [c.clone() for c in m.k_cache + m.v_cache]
    # the overlapped TP prefill (two batch halves, all-reduces started early) vs the plain layer loop
    overlap_on = m.tp_overlap
    m.tp_overlap = False
    for c in m.k_cache + m.v_cache:
        c.zero_()
    vals0, idx0 = m.step(ids.cuda(), pos, lens.cuda(), decode=False, k=8)
    m.tp_overlap = overlap_on
    overlap_diff = float((vals0.float() - vals.float()).abs().max())
    # ... and the KV cache rows each wrote (the halves append through offset cache views): the
    # same rows, values equal up to the halves' own GEMM tile choices
    kv_diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(kv_over, m.k_cache + m.v_cache))
    kv_nz = [bool((a != 0).any().item()) == bool((b != 0).any().item()) for a, b in zip(kv_over, m.k_cache + m.v_cache)]
    kv_rows_same = all(torch.equal((a != 0).any(-1), (b != 0).any(-1)) for a, b in zip(kv_over, m.k_cache + m.v_cache))
    del kv_over
    failed = ""
    stall_rank = int(os.environ.get("STALL_RANK", "-1"))
    if stall_rank >= 0:
        # fault injection: one rank's stream stalls past the peers' one-shot wait bound; every rank
        # must fail the request (TPCommError), not return tokens computed from partial sums
        from mlmicroservicetemplate_amd import ops
        from mlmicroservicetemplate_amd.models.llama import TPCommError

        # the prefill checks above ran with the default (~1 s) peer-wait bound: two ranks
        # time-sharing one GPU can miss a few-ms bound on any small all-reduce; only the stalled
        # request runs with the tight bound
        if m.comm.car is not None and os.environ.get("MLS_AR_TIMEOUT_ITERS_STALL"):
            m.comm.car.timeout = int(os.environ["MLS_AR_TIMEOUT_ITERS_STALL"])
        if rank == stall_rank:
            ops.gpu_sleep(int(os.environ.get("STALL_US", "300000")))
        try:
            m.generate(ids, lens, GenParams(max_new_tokens=8))
        except TPCommError as e:
            failed = type(e).__name__
    # count host round trips of the decode loop (.cpu() on device tensors)
    calls = []
    orig = torch.Tensor.cpu

    def counting_cpu(self, *a, **kw):
        if self.is_cuda:
            calls.append(tuple(self.shape))
        return orig(self, *a, **kw)

    torch.Tensor.cpu = counting_cpu
    try:
        out = m.generate(ids, lens, GenParams(max_new_tokens=8))
    finally:
        torch.Tensor.cpu = orig
    # teacher-forced decode: every step feeds the TP=1 greedy token (REF_TOKENS) and records the
    # merged candidates' top-1 id -- compared with TP=1's top-1 wherever its margin is decisive
    tf = []
    ref_tok = json.loads(os.environ.get("REF_TOKENS", "[]"))
    if ref_tok:
        rt = torch.tensor(ref_tok, dtype=torch.int32)
        cur = lens.clone().to(torch.int32).cuda()
        for t in range(rt.shape[1] - 1):
            v, i = m.decode_step(rt[:, t].cuda(), cur, 8, max_ctx=24 + t + 1)
            cv, ci = m.gather_candidates(v, i)
            tf.append(ci.gather(1, cv.argmax(1, keepdim=True)).squeeze(1))
            cur = cur + 1
    info = torch.tensor([int(m.use_graphs), int(m.comm.car is not None), len(m._graphs) + len(m._dev_graphs),
                         len(calls), int(m.ar_fused_calls)])
    if m.comm.car is not None:
        info[1] += 10 * m.comm.car.errors()  # peer-wait timeouts would show here
    torch.save({"tokens": out.cpu(), "vals": allv.cpu(), "idx": alli.cpu(), "info": info, "failed": failed,
                "overlap_diff": overlap_diff, "kv_diff": kv_diff, "kv_rows_same": bool(kv_rows_same and all(kv_nz)),
                "tf_top1": torch.stack(tf, 1) if tf else torch.zeros(0)},
               os.environ["OUT"] + f".{rank}.pt")
    dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
