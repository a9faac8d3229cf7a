"""Chunked prefill on the CPU (reference backend): ``R.attention_ctx``, ``LlamaTP.step(past=...)`` /
``prefill_chunked`` / ``generate(prefill_chunk=...)`` and ``ContinuousLlama(prefill_chunk=...)`` give
what one-shot prefill gives -- per-slot and paged, TP = 1 and TP = 2 over gloo.

Tolerances: the reference backend keeps fp32 K / V rows in its cache, so a chunk attends exactly the
values one-shot prefill attends; the only difference is the fp32 summation order (einsum over the
gathered rows instead of one batched matmul, GEMMs of another row count).  RTOL = 1e-5 relative to the
largest magnitude is ~100 fp32 ulps; observed on the cases below: 1.0e-7 (attention), 5.5e-7 (cache
rows), 2.2e-7 (top-k values)."""
import multiprocessing as mp
import os
import socket

import pytest
import torch

from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
from mlmicroservicetemplate_amd.models.llama_serving import OP_ITER, OP_STOP, ContinuousLlama, _Seq
from mlmicroservicetemplate_amd.ops import reference as R

CFG = dict(vocab=2048, hidden=256, layers=2, heads=8, kv_heads=4, head_dim=32, intermediate=512)
RTOL = 1e-5
MAX_SEQ = 96
PAGES = 8  # 7 data pages of 64 rows + the scratch page


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


@pytest.fixture(scope="module")
def params():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG)
    return cfg, init_llama_shard(cfg, 1, 0, seed=4)


def _prompts():
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, 2000, (3, 70), generator=g)
    return ids, torch.tensor([70, 37, 5])  # ragged; 70 rows cross the 64-row page inside the third 24-chunk


# ------------------------------------------------------------------ the oracle against the one-shot oracle
def _qkv_and_caches(B, S, Hq, Hkv, D, lens, slots, paged):
    """Random fused qkv of B sequences and caches holding exactly its K / V rows: per-slot
    ``[5, 24, Hkv, D]`` or a pool of 4-row pages through a shuffled table."""
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, generator=g)
    _q, k, v = R.split_qkv(qkv, Hq, Hkv, D)
    k, v = k.view(B, S, Hkv, D), v.view(B, S, Hkv, D)
    n_slots, rows = 5, 24
    table = None
    if paged:
        pr = 4
        pps = rows // pr
        table = torch.randperm(n_slots * pps, generator=g).view(n_slots, pps).to(torch.int32)
        kc = torch.full((n_slots * pps, pr, Hkv, D), float("nan"))
        vc = torch.full_like(kc, float("nan"))
        for b in range(B):
            for r in range(int(lens[b])):
                page = int(table[slots[b], r // pr])
                kc[page, r % pr], vc[page, r % pr] = k[b, r], v[b, r]
    else:
        kc = torch.full((n_slots, rows, Hkv, D), float("nan"))  # rows past lens are never read
        vc = torch.full_like(kc, float("nan"))
        for b in range(B):
            kc[slots[b], : lens[b]], vc[slots[b], : lens[b]] = k[b, : lens[b]], v[b, : lens[b]]
    return qkv, kc, vc, table


@pytest.mark.parametrize("paged", [False, True])
def test_attention_ctx_matches_attention(paged):
    B, S, Hq, Hkv, D = 2, 20, 4, 2, 16
    lens = torch.tensor([20, 13], dtype=torch.int32)
    slots = [3, 1]  # a permutation that leaves slots unused
    sid = torch.tensor(slots, dtype=torch.int32)
    qkv, kc, vc, table = _qkv_and_caches(B, S, Hq, Hkv, D, lens, slots, paged)
    want = R.attention(qkv, B, S, Hq, Hkv, D, kv_lens=lens, causal=True).view(B, S, -1)
    # past = 0: the whole sequence as one chunk
    got = R.attention_ctx(qkv, kc, vc, torch.zeros(B, dtype=torch.int32), lens, B, S, Hq, Hkv, D, slot_ids=sid,
                          page_table=table).view(B, S, -1)
    for b in range(B):
        print("attention_ctx rel", _rel(got[b, : lens[b]], want[b, : lens[b]]))
        assert _rel(got[b, : lens[b]], want[b, : lens[b]]) < RTOL
        assert not got[b, lens[b]:].any()  # rows past the valid length: zero
    # past > 0: the chunk [past, lens) against the rows before it, and a chunk that ends mid-sequence
    for past_l, end_l in (([7, 5], [20, 13]), ([3, 12], [11, 13])):
        past, end = torch.tensor(past_l, dtype=torch.int32), torch.tensor(end_l, dtype=torch.int32)
        Sc = int((end - past).max())
        chunk = torch.zeros(B, Sc, qkv.shape[1])
        for b in range(B):
            n = end_l[b] - past_l[b]
            chunk[b, :n] = qkv.view(B, S, -1)[b, past_l[b]: end_l[b]]
        got = R.attention_ctx(chunk.view(B * Sc, -1), kc, vc, past, end, B, Sc, Hq, Hkv, D, slot_ids=sid,
                              page_table=table).view(B, Sc, -1)
        assert torch.isfinite(got).all()  # rows >= lens (NaN in the caches) are never read
        for b in range(B):
            n = end_l[b] - past_l[b]
            assert _rel(got[b, :n], want[b, past_l[b]: end_l[b]]) < RTOL


def test_attention_ctx_head_major_layout():
    B, S, Hq, Hkv, D = 2, 20, 4, 2, 16
    lens = torch.tensor([20, 13], dtype=torch.int32)
    sid = torch.tensor([3, 1], dtype=torch.int32)
    qkv, kc, vc, _ = _qkv_and_caches(B, S, Hq, Hkv, D, lens, [3, 1], False)
    past = torch.tensor([7, 5], dtype=torch.int32)
    chunk = torch.zeros(B, 13, qkv.shape[1])
    for b in range(B):
        chunk[b, : lens[b] - past[b]] = qkv.view(B, S, -1)[b, past[b]: lens[b]]
    a = R.attention_ctx(chunk.view(B * 13, -1), kc, vc, past, lens, B, 13, Hq, Hkv, D, slot_ids=sid)
    b_ = R.attention_ctx(chunk.view(B * 13, -1), kc.transpose(1, 2).contiguous(), vc.transpose(1, 2).contiguous(), past,
                         lens, B, 13, Hq, Hkv, D, slot_ids=sid, head_major=True)
    assert torch.equal(a, b_)


# ------------------------------------------------------------------ LlamaTP
def _model(cfg, p, paged, **kw):
    return LlamaTP(p, cfg, max_batch=3, max_seq=MAX_SEQ, kv_pages=PAGES if paged else 0, **kw)


@pytest.mark.parametrize("paged", [False, True])
def test_step_in_chunks_matches_one_shot(params, paged):
    cfg, p = params
    ids, lens = _prompts()
    B, S = ids.shape
    one, chk = _model(cfg, p, paged), _model(cfg, p, paged)
    if paged:  # the same pages on both models (generate() does this itself)
        for m in (one, chk):
            for b in range(B):
                m.pages.assign(b, MAX_SEQ)
    pos = torch.arange(S, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
    v1, i1 = one.step(ids, pos, lens, decode=False, k=5)
    v2, i2 = chk.prefill_chunked(ids, lens, 24, 5)  # chunks [0, 24) [24, 48) [48, 70); rows drop out as they end
    print("top-k values rel", _rel(v2, v1))
    assert torch.equal(i1, i2)
    assert _rel(v2, v1) < RTOL
    for layer in range(cfg.layers):
        for c1, c2 in ((one.k_cache[layer], chk.k_cache[layer]), (one.v_cache[layer], chk.v_cache[layer])):
            if paged:  # gather each slot's rows through the (identical) tables
                assert torch.equal(one.pages.host, chk.pages.host)
                t = one.pages.host[:B].long()
                c1, c2 = c1[t].reshape(B, -1, *c1.shape[2:]), c2[t].reshape(B, -1, *c2.shape[2:])
            for b in range(B):
                print("cache rows rel", _rel(c2[b, : lens[b]], c1[b, : lens[b]]))
                assert _rel(c2[b, : lens[b]], c1[b, : lens[b]]) < RTOL
                assert not c2[b, lens[b]:].any()  # nothing written past the prompt
    # two explicit chunks through step(past=...), the second splitting the page at row 64
    two = _model(cfg, p, paged)
    if paged:
        for b in range(B):
            two.pages.assign(b, MAX_SEQ)
    cut = 40
    two.step(ids[:, :cut], pos[:, :cut], lens.clamp(max=cut), decode=False, k=5, past=torch.zeros(B, dtype=torch.int32))
    rows = torch.tensor([0])  # only row 0 is longer than 40
    v3, i3 = two.step(ids[rows, cut:], pos[rows, cut:], lens[rows], decode=False, k=5,
                      slot_ids=rows.to(torch.int32), past=torch.full((1,), cut, dtype=torch.int32))
    assert torch.equal(i3[0], i1[0]) and _rel(v3[0], v1[0]) < RTOL


@pytest.mark.parametrize("paged", [False, True])
def test_generate_chunked_same_tokens(params, paged):
    cfg, p = params
    ids, lens = _prompts()
    for gp in (GenParams(max_new_tokens=6), GenParams(6, top_k=20, temperature=0.8, seed=3)):
        want = _model(cfg, p, paged).generate(ids, lens, gp)
        m = _model(cfg, p, paged)
        got = m.generate(ids, lens, gp, prefill_chunk=24)
        assert torch.equal(got, want)
        if paged:
            assert m.pages.free_pages == PAGES - 1


# ------------------------------------------------------------------ serving
def _requests():
    g = torch.Generator().manual_seed(5)
    long_ids = torch.randint(3, 2000, (60,), generator=g).tolist()  # 8 chunks of 8
    shorts = [torch.randint(3, 2000, (n,), generator=g).tolist() for n in (5, 11, 3)]
    return [(long_ids, GenParams(max_new_tokens=5)),
            (shorts[0], GenParams(max_new_tokens=4)),
            (shorts[1], GenParams(6, top_k=5, temperature=0.7, seed=9)),
            (shorts[2], GenParams(max_new_tokens=3))]


def _drive(eng: ContinuousLlama, reqs, trace=None):
    """The scheduler loop run from the test (``ContinuousLlama._loop`` step by step): the long
    request first, the short ones after its second iteration -- while it is mid-prefill when chunked."""
    def it():
        eng.run_iteration(eng._leader_admissions())
        if trace is not None:
            trace.append(dict(eng.stats(), done=[f.done() for f in futs]))

    futs = [eng.submit(*reqs[0])]
    it()
    it()
    futs += [eng.submit(ids, gp) for ids, gp in reqs[1:]]
    for _ in range(200):
        if all(f.done() for f in futs):
            break
        it()
    return [f.result(timeout=0) for f in futs]


@pytest.mark.parametrize("paged", [False, True])
def test_serving_chunked_matches_unchunked(params, paged):
    cfg, p = params
    reqs = _requests()
    want = _drive(ContinuousLlama(_model(cfg, p, paged)), reqs)
    m = _model(cfg, p, paged)
    eng = ContinuousLlama(m, prefill_chunk=8)
    trace = []
    got = _drive(eng, reqs, trace)
    assert got == want  # greedy and seeded top-k alike
    # the long prompt took 8 iterations of 8 positions; short requests were admitted, decoded and
    # one of them finished while it was still prefilling: decode steps ran between its chunks (their
    # dummy row for the prefilling slot must not land on its live rows -- `got == want` above)
    assert [t["prefilling"] for t in trace[:7]] == [1, 1, 2, 1, 1, 1, 1] and trace[7]["prefilling"] == 0
    mid = [t for t in trace if t["prefilling"] >= 1]
    assert any(t["done"][1:] != [False] * len(t["done"][1:]) for t in mid)
    assert max(t["tokens"] for t in mid) >= 6
    st = eng.stats()
    assert st["active"] == 0 and st["prefilling"] == 0
    if paged:
        assert st["kv_pages_free"] == st["kv_pages"] - 1  # every page returned
    # unchunked: the same schedule prefills the long prompt in its first iteration
    assert ContinuousLlama(_model(cfg, p, paged)).stats()["prefilling"] == 0


# ------------------------------------------------------------------ TP = 2 over gloo
class _Chan:
    """The serving control channel (plugins/llm.py implements it with tensors) over object broadcasts."""

    def __init__(self):
        self._adm = None

    def send_header(self, admit):
        import torch.distributed as dist

        if admit is None:
            obj = [(OP_STOP, 0, 0), None]
        else:
            obj = [(OP_ITER, len(admit), max((len(q.ids) for q in admit), default=0)),
                   [(q.ids, q.gp, q.slot) for q in admit]]
        dist.broadcast_object_list(obj, src=0)

    def recv_header(self):
        import torch.distributed as dist

        obj = [None, None]
        dist.broadcast_object_list(obj, src=0)
        self._adm = obj[1]
        return obj[0]

    def recv_admissions(self, n, S):
        assert len(self._adm) == n
        return [_Seq(list(ids), gp, None, slot=slot) for ids, gp, slot in self._adm]


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tp_worker(rank, world, port, paged, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from mlmicroservicetemplate_amd.models.llama import TPComm

    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = tiny_config(**CFG)
        m = LlamaTP(init_llama_shard(cfg, world, rank, seed=4), cfg, tp=world, rank=rank, comm=TPComm(None, world),
                    max_batch=3, max_seq=MAX_SEQ, kv_pages=PAGES if paged else 0)
        eng = ContinuousLlama(m, channel=_Chan(), prefill_chunk=8)
        if rank == 0:
            outs = _drive(eng, _requests())
            eng._stop = True
            assert eng._leader_admissions() is None  # announces the stop
            q.put((rank, outs, eng.iterations, m.pages.free_pages if paged else -1))
        else:
            assert eng.follow() == 0
            q.put((rank, None, eng.iterations, m.pages.free_pages if paged else -1))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.timeout(240)
def test_tp2_chunked_serving_matches_tp1(params, paged):
    cfg, p = params
    want = _drive(ContinuousLlama(_model(cfg, p, paged)), _requests())  # TP = 1, unchunked
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, paged, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=200) for _ in range(2))
    for pr in procs:
        pr.join(30)
        assert pr.exitcode == 0
    assert res[0][1] == want
    assert res[0][2] == res[1][2]  # the follower replayed every iteration
    if paged:
        assert res[0][3] == res[1][3] == PAGES - 1


# ------------------------------------------------------------------ refusals
def test_fp8_kv_refuses_chunked_prefill(params):
    cfg, p = params
    ids, lens = _prompts()
    m = LlamaTP(p, cfg, max_batch=3, max_seq=MAX_SEQ, kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        m.generate(ids, lens, GenParams(2), prefill_chunk=8)
    with pytest.raises(ValueError, match="fp8"):
        m.prefill_chunked(ids, lens, 8, 1)
    with pytest.raises(ValueError, match="fp8"):
        m.step(ids[:, :8], torch.arange(8).expand(3, 8), lens.clamp(max=8), decode=False, k=1,
               past=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="fp8"):
        ContinuousLlama(m, prefill_chunk=8)
    assert m.generate(ids, lens, GenParams(2)).shape == (3, 2)  # unchunked: served as before
    ok = LlamaTP(p, cfg, max_batch=3, max_seq=MAX_SEQ)
    with pytest.raises(ValueError):
        ContinuousLlama(ok, prefill_chunk=-1)
    with pytest.raises(ValueError):
        ok.generate(ids, lens, GenParams(2), prefill_chunk=-4)
    with pytest.raises(ValueError):
        ok.step(ids[:, :1], torch.zeros(3, 1, dtype=torch.int32), torch.ones(3, dtype=torch.int32), decode=True, k=1,
                past=torch.zeros(3, dtype=torch.int32))


def test_plugin_config(tmp_path):
    from mlmicroservicetemplate_amd.config import Settings
    from mlmicroservicetemplate_amd.plugins.base import PluginContext
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    def plugin(text):
        y = tmp_path / "llama.yaml"
        y.write_text(text)
        s = Settings.load(env_file=None, environ={}, overrides={"REGISTER": False, "MODEL": "llama",
                                                                "MODEL_CONFIG": str(y), "MAX_BATCH": 2, "GPUS": 0})
        pl = LlamaPlugin()
        pl.init(PluginContext(settings=s))
        return pl

    base = "config: tiny\nmax_seq: 64\noverrides:\n  layers: 1\n"
    with pytest.raises(ValueError, match="fp8"):
        plugin(base + "kv_dtype: fp8\nprefill_chunk: 16\n")
    pl = plugin(base + "prefill_chunk: 16\n")
    try:
        assert pl.engine.prefill_chunk == 16 and "prefilling" in pl.engine.stats()
    finally:
        pl.close()
    pl = plugin(base)
    try:
        assert pl.engine.prefill_chunk == 0
    finally:
        pl.close()
