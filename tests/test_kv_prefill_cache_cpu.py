"""``kv_prefill="cache"`` on the CPU (reference backend): with the e4m3 KV cache every prefill attention
reads the quantised cache rows, as decode does, so a token's logits do not depend on how its prompt was
chunked, on whether its prefix came from shared pages or on whether a verify step scored it -- chunked
prefill, prefix caching and speculative decoding are served with ``kv_dtype="fp8"`` and emit the very
tokens of the plain run.  Every equality below is exact token equality: the reference cache holds fp32
``kv_dequant_fp8(kv_quant_fp8(row))``, all routes attend those same values, and the only difference left
is the fp32 summation order of GEMMs of another row count (1e-7 relative, tests/test_prefill_chunk_cpu.py),
far below the distance between the first and second candidate of the prompts used here."""
import multiprocessing as mp
import os
import socket

import pytest
import torch

from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, TPComm, init_llama_shard, tiny_config
from mlmicroservicetemplate_amd.models.llama_serving import OP_ITER, OP_STOP, ContinuousLlama, _Seq

CFG = dict(vocab=2048, hidden=256, layers=2, heads=8, kv_heads=4, head_dim=32, intermediate=512)
MAX_SEQ = 192
PAGES = 8  # a request holds at most 3 pages (130-token prefix + suffix + new tokens); 7 data pages + scratch
FP8 = dict(kv_dtype="fp8", kv_prefill="cache")
GPS = (GenParams(max_new_tokens=6), GenParams(6, top_k=20, temperature=0.8, seed=3))


@pytest.fixture(scope="module")
def params():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG)
    return cfg, init_llama_shard(cfg, 1, 0, seed=4)


def _model(cfg, p, paged=True, **kw):
    return LlamaTP(p, cfg, max_batch=3, max_seq=MAX_SEQ, kv_pages=PAGES if paged else 0, **kw)


def _toks(n, seed):
    return torch.randint(3, 2000, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _prompts():
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, 2000, (3, 70), generator=g)
    return ids, torch.tensor([70, 37, 5])  # ragged; 70 rows cross the 64-row page


# ------------------------------------------------------------------ lockstep generate
@pytest.fixture(scope="module")
def plain(params):
    """generate() unchunked under fp8 + cache, per (paged, sampling): computed once, never changed."""
    cfg, p = params
    ids, lens = _prompts()
    return {(paged, gi): _model(cfg, p, paged, **FP8).generate(ids, lens, gp)
            for paged in (False, True) for gi, gp in enumerate(GPS)}


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("chunk", [5, 8, 70, 100])
def test_generate_is_invariant_to_chunking(params, plain, paged, chunk):
    """prefill_chunk 0 (the fixture) against 5, 8, the longest prompt's 70 and 100 above it."""
    cfg, p = params
    ids, lens = _prompts()
    for gi, gp in enumerate(GPS):
        m = _model(cfg, p, paged, **FP8)
        assert torch.equal(m.generate(ids, lens, gp, prefill_chunk=chunk), plain[paged, gi])
        if paged:
            assert m.pages.free_pages == PAGES - 1


def test_cache_mode_is_not_a_noop(params):
    """Prefill logits move from unquantised to e4m3 rows: the first token's candidates differ between
    kv_prefill="rows" and "cache" (values; the 5-token prompt alone would do)."""
    cfg, p = params
    ids, lens = _prompts()
    pos = torch.arange(ids.shape[1], dtype=torch.int32).unsqueeze(0).expand(*ids.shape).contiguous()
    out = {}
    for mode in ("rows", "cache"):
        m = _model(cfg, p, False, kv_dtype="fp8", kv_prefill=mode)
        out[mode] = m.step(ids, pos, lens, decode=False, k=5)
        assert m.kv_prefill == mode
    assert any(not torch.equal(out["rows"][0][b], out["cache"][0][b]) for b in range(ids.shape[0]))
    # ... while the cache rows themselves are the same in layer 0 (same inputs, same quantiser)
    a, b = (_model(cfg, p, False, kv_dtype="fp8", kv_prefill=mode) for mode in ("rows", "cache"))
    a.step(ids, pos, lens, decode=False, k=1)
    b.step(ids, pos, lens, decode=False, k=1)
    assert torch.equal(a.k_cache[0], b.k_cache[0]) and torch.equal(a.v_cache[0], b.v_cache[0])


def test_one_shot_step_equals_explicit_past_zero(params):
    cfg, p = params
    ids, lens = _prompts()
    pos = torch.arange(ids.shape[1], dtype=torch.int32).unsqueeze(0).expand(*ids.shape).contiguous()
    a, b = _model(cfg, p, False, **FP8), _model(cfg, p, False, **FP8)
    va, ia = a.step(ids, pos, lens, decode=False, k=5)
    vb, ib = b.step(ids, pos, lens, decode=False, k=5, past=torch.zeros(3, dtype=torch.int32))
    assert torch.equal(va, vb) and torch.equal(ia, ib)


def test_route_keeps_fp8_verify_steps_on_the_context_kernel():
    """``StepRoute.multi`` (the bf16 verify kernel) is false when the cache is e4m3; the default is unchanged."""
    from mlmicroservicetemplate_amd.models.llama_route import step_route

    kw = dict(B=2, S=4, decode=False, has_past=True, all_rows=True, tp=1, hq=8, hkv=2, head_dim=128, hidden=512,
              have_packed=True, have_w4=False, have_fp8=False, o_packed=True, o_fp8=False, w4_max_rows=0,
              pk_fold=True, prefill_fold=False, fuse_combine=True, fuse_add_norm=True, ar_fuse=True,
              tp_overlap=True, verify_attn="multi", spec_max_tokens=8, dec_chunk=0, ar_fusable=False,
              capturing=False)
    assert step_route(**kw).multi and step_route(**kw, kv_fp8=False).multi
    assert not step_route(**kw, kv_fp8=True).multi


# ------------------------------------------------------------------ continuous engine
PREFIX = _toks(130, 30)  # two full pages + 2 rows


def _requests():
    """Three prompts that share a 130-token prefix (two full pages; one sampled), a long unrelated one,
    and short ones -- greedy and sampled."""
    return [(PREFIX + _toks(7, 31), GenParams(max_new_tokens=8)),
            (_toks(60, 41), GenParams(max_new_tokens=9)),
            (PREFIX + _toks(12, 32), GenParams(8, top_k=5, temperature=0.7, seed=9)),
            (_toks(5, 42), GenParams(max_new_tokens=7)),
            (PREFIX + _toks(3, 33), GenParams(max_new_tokens=6)),
            (_toks(11, 43), GenParams(8, top_k=5, temperature=0.7, seed=9))]


def _it(eng):
    eng.run_iteration(eng._leader_admissions())


def _drive(eng, reqs):
    """The scheduler loop stepped from the test (tests/test_prefix_cache_cpu.py): the first request, two
    iterations, then everything else at once."""
    futs = [eng.submit(*reqs[0])]
    _it(eng)
    _it(eng)
    futs += [eng.submit(ids, gp) for ids, gp in reqs[1:]]
    for _ in range(400):
        if all(f.done() for f in futs):
            break
        _it(eng)
    return [f.result(timeout=0) for f in futs]


def _oracle_drafter(reqs, outs):
    """Right drafts for every sequence of a recorded run (distinct prompts): the tokens that followed
    (tests/test_speculative_cpu.py)."""
    prompts = [list(ids) for ids, _gp in reqs]

    def draft(tokens, n):
        toks = list(tokens)
        for p, c in zip(prompts, outs):
            e = len(toks) - len(p)
            if e > 0 and toks[: len(p)] == p and toks[len(p):] == list(c[:e]):
                return list(c[e: e + n])
        return [toks[-1]] * n

    return draft


@pytest.fixture(scope="module")
def want(params):
    """What the plain engine emits under fp8 + cache: no prefix cache, no speculation, unchunked."""
    cfg, p = params
    return _drive(ContinuousLlama(_model(cfg, p, **FP8)), _requests())


@pytest.mark.parametrize("kw", [dict(prefix_cache=True), dict(speculate=1), dict(speculate=3), dict(prefill_chunk=16),
                                dict(prefix_cache=True, speculate=3, prefill_chunk=16)],
                         ids=["prefix", "spec1", "spec3", "chunk", "all"])
def test_engine_features_keep_the_tokens(params, want, kw):
    cfg, p = params
    reqs = _requests()
    if kw.get("speculate"):
        kw = dict(kw, drafter=_oracle_drafter(reqs, want))
    eng = ContinuousLlama(_model(cfg, p, **FP8), **kw)
    assert _drive(eng, reqs) == want  # greedy and sampled alike
    st = eng.stats()
    if kw.get("prefix_cache"):
        assert st["prefix_hits"] > 0 and st["prefix_hit_tokens"] == 128 * st["prefix_hits"]
    if kw.get("speculate"):
        assert st["spec_accepted"] > 0
    assert st["active"] == 0 and eng.failures == 0


# ------------------------------------------------------------------ TP = 2 over gloo
class _Chan:
    """The serving control channel over object broadcasts (tests/test_prefill_chunk_cpu.py)."""

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


def _tp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = tiny_config(**CFG)
        m = LlamaTP(init_llama_shard(cfg, world, rank, seed=4), cfg, tp=world, rank=rank, comm=TPComm(None, world),
                    max_batch=3, max_seq=MAX_SEQ, kv_pages=PAGES, **FP8)
        eng = ContinuousLlama(m, channel=_Chan(), prefill_chunk=16, prefix_cache=True)
        if rank == 0:
            outs = _drive(eng, _requests())
            eng._stop = True
            assert eng._leader_admissions() is None  # announces the stop
            q.put((rank, outs, eng.iterations, eng.stats()["prefix_hits"]))
        else:
            assert eng.follow() == 0
            q.put((rank, None, eng.iterations, -1))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_tp2_matches_tp1(want):
    """TP = 2, chunked with the prefix cache on, against the plain TP = 1 run."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=200) for _ in range(2))
    for pr in procs:
        pr.join(30)
        assert pr.exitcode == 0
    assert res[0][1] == want
    assert res[0][2] == res[1][2]  # the follower replayed every iteration
    assert res[0][3] > 0


# ------------------------------------------------------------------ refusals
def _plugin(tmp_path, text):
    from mlmicroservicetemplate_amd.config import Settings
    from mlmicroservicetemplate_amd.plugins.base import PluginContext
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    y = tmp_path / "llama.yaml"
    y.write_text(text)
    s = Settings.load(env_file=None, environ={}, overrides={"REGISTER": False, "MODEL": "llama",
                                                            "MODEL_CONFIG": str(y), "MAX_BATCH": 2, "GPUS": 0})
    pl = LlamaPlugin()
    pl.init(PluginContext(settings=s))
    return pl


def test_refusals(params, tmp_path):
    cfg, p = params
    ids, lens = _prompts()
    with pytest.raises(ValueError, match="kv_prefill"):
        _model(cfg, p, kv_prefill="cache")  # bf16: nothing to choose
    with pytest.raises(ValueError, match="kv_prefill"):
        _model(cfg, p, kv_dtype="bf16", kv_prefill="cache")
    with pytest.raises(ValueError, match="kv_prefill"):
        _model(cfg, p, kv_dtype="fp8", kv_prefill="pages")
    # kv_prefill="rows" (the default): the four refusals stand, naming fp8
    for kw in (dict(kv_dtype="fp8"), dict(kv_dtype="fp8", kv_prefill="rows")):
        m = _model(cfg, p, **kw)
        with pytest.raises(ValueError, match="fp8"):
            m.generate(ids, lens, GenParams(2), prefill_chunk=8)
        with pytest.raises(ValueError, match="fp8"):
            m.check_prefill_chunk()
        with pytest.raises(ValueError, match="fp8"):
            m.check_speculate(2)
        with pytest.raises(ValueError, match="fp8"):
            m.check_prefix_cache()
        for ekw in (dict(prefill_chunk=8), dict(speculate=2), dict(prefix_cache=True)):
            with pytest.raises(ValueError, match="fp8"):
                ContinuousLlama(m, **ekw)
        assert m.generate(ids, lens, GenParams(2)).shape == (3, 2)  # unchunked: served as before
    base = "config: tiny\nmax_seq: 128\noverrides:\n  layers: 1\n"
    for extra in ("prefill_chunk: 16\n", "speculate: 2\n", "kv_pages: 5\nprefix_cache: true\n"):
        with pytest.raises(ValueError, match="fp8"):
            _plugin(tmp_path, base + "kv_dtype: fp8\n" + extra)
    with pytest.raises(ValueError, match="kv_prefill"):
        _plugin(tmp_path, base + "kv_prefill: cache\n")
    # with the switch: every check passes
    m = _model(cfg, p, **FP8)
    m.check_prefill_chunk()
    m.check_speculate(2)
    m.check_prefix_cache()
    pl = _plugin(tmp_path, base + "kv_dtype: fp8\nkv_prefill: cache\nprefill_chunk: 16\nkv_pages: 5\n"
                                  "prefix_cache: true\nspeculate: 2\n")
    try:
        d = pl.describe()
        assert (d["kv_dtype"], d["kv_prefill"], d["prefill_chunk"], d["kv_pages"], d["prefix_cache"], d["speculate"]) \
            == ("fp8", "cache", 16, 5, True, 2)
        assert pl.engine.prefill_chunk == 16 and pl.engine.prefix is not None and pl.engine.speculate == 2
    finally:
        pl.close()
