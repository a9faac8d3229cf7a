"""Prefix caching on the CPU (reference backend, tiny config): page reference counts
(models/kv_pages.py), the prefix index (models/prefix_cache.py) and ``ContinuousLlama(prefix_cache=True)``
against ``prefix_cache=False`` -- one-shot and chunked prefill, with and without speculative decoding,
TP = 1 and TP = 2 over gloo.

Token equality is exact, as in ``test_prefill_chunk_cpu.py``: the reference backend keeps fp32 K / V rows,
so a suffix prefilled against adopted pages attends exactly the rows a full prefill attends; only the
fp32 summation order differs (~1e-7 relative on the logits there), far below any top-1 / sampling gap of
these prompts."""
import multiprocessing as mp
import os
import socket

import pytest
import torch

from mlmicroservicetemplate_amd.models import prefix_cache as PC
from mlmicroservicetemplate_amd.models.kv_pages import OutOfPages, PageTable
from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
from mlmicroservicetemplate_amd.models.llama_serving import OP_ITER, OP_STOP, ContinuousLlama, _Seq
from mlmicroservicetemplate_amd.models.prefix_cache import PrefixCache

CFG = dict(vocab=2048, hidden=256, layers=2, heads=8, kv_heads=4, head_dim=32, intermediate=512)
MAX_SEQ = 192
# one request needs at most 3 pages (130-token prefix + suffix + new tokens <= 192 rows); the pool holds
# 1.5x that, rounded up: 5 data pages + the scratch page
PAGES = 6


@pytest.fixture(scope="module")
def params():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG)
    return cfg, init_llama_shard(cfg, 1, 0, seed=4)


def _model(cfg, p, **kw):
    return LlamaTP(p, cfg, max_batch=3, max_seq=MAX_SEQ, kv_pages=PAGES, **kw)


def _toks(n, seed):
    return torch.randint(3, 2000, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


# ------------------------------------------------------------------ PageTable reference counts
def _table(num_pages=8):
    pt = PageTable(num_pages=num_pages, page_rows=64, max_batch=4, pages_per_seq=4)
    return pt, PrefixCache(pt)


def test_adopt_and_release_in_both_orders():
    for first, second in ((0, 1), (1, 0)):
        pt, pc = _table()
        ids = _toks(130, 1)
        pt.assign(0, 192)
        owner = pt.pages_of(0)
        assert pc.insert(ids, owner, stamp=1) == 2
        shared = pc.match(ids + [5])
        assert shared == owner[:2]
        pt.adopt(1, shared)
        pt.assign(1, 192)  # one fresh page behind the two shared ones
        assert pt.pages_of(1)[:2] == shared and pt.host[1, :2].tolist() == shared
        assert [pt.refcount(pg) for pg in owner] == [2, 2, 1]
        assert pt.free_pages == 7 - 4
        pt.release(first)
        # a page adopted by two slots is freed only after both release
        assert [pt.refcount(pg) for pg in shared] == [1, 1] and pt.free_pages == 7 - 3
        assert not set(shared) & set(pt._free)
        pt.release(second)
        assert [pt.refcount(pg) for pg in shared] == [0, 0]
        # indexed pages nobody holds are reclaimable: counted as available, not on the free list
        assert pt.free_pages == 7 and len(pt._free) == 5 and not set(shared) & set(pt._free)
        assert pt.can_fit(64 * 4) and pt.host[first].tolist() == [0, 0, 0, 0]
        with pytest.raises(ValueError):
            pt.adopt(2, [pt._free[0]])  # a free page holds nothing
        pt.assign(2, 64)
        with pytest.raises(ValueError):
            pt.adopt(2, shared)  # shared pages go first


def test_assign_evicts_only_the_shortfall_in_order():
    pt, pc = _table(num_pages=8)  # 7 data pages
    a, b = _toks(192, 1), _toks(128, 2)
    pt.assign(0, 192)
    pa = pt.pages_of(0)
    pc.insert(a, pa, stamp=1)  # 3 entries, depths 1..3
    pt.assign(1, 128)
    pb = pt.pages_of(1)
    pc.insert(b, pb, stamp=2)  # 2 entries, used later
    pt.release(0)
    pt.release(1)
    assert pt.free_pages == 7 and len(pt._free) == 2 and len(pc) == 5
    pt.assign(3, 64 * 4)
    # slot 3 needed 4 with 2 free: exactly 2 evictions -- the oldest stamp, deeper first
    assert pc.evictions == 2 and len(pc) == 3 and pt.free_pages == 3 and pt._free == []
    assert not pc.holds(pa[2]) and not pc.holds(pa[1]) and pc.holds(pa[0])
    with pytest.raises(OutOfPages):
        pt.assign(2, 64 * 4)  # 3 reclaimable, 4 needed
    # OutOfPages still changes nothing: no page handed out, no entry evicted for it
    assert pt.pages_of(2) == [] and pc.evictions == 2 and len(pc) == 3 and pt.free_pages == 3
    assert set(pt.pages_of(3)) >= {pa[2], pa[1]}
    assert pc.match(a) == [pa[0]]  # the chain's head is still served
    pt.release(3)
    # equal stamps, equal depth: the lower page id goes first
    pt2, pc2 = _table(num_pages=4)
    x, y = _toks(64, 3), _toks(64, 4)
    pt2.assign(0, 64)
    pt2.assign(1, 64)
    p0, p1 = pt2.pages_of(0)[0], pt2.pages_of(1)[0]
    pc2.insert(y, [p1], stamp=5)
    pc2.insert(x, [p0], stamp=5)
    pt2.release(0)
    pt2.release(1)
    pt2.assign(2, 128)  # 1 free + 1 eviction
    assert pc2.evictions == 1 and not pc2.holds(min(p0, p1)) and pc2.holds(max(p0, p1))
    # a hit stamps the whole chain: the chain used now outlives one inserted later but not used since
    pt3, pc3 = _table(num_pages=5)
    old, new = _toks(128, 5), _toks(128, 6)
    pt3.assign(0, 128)
    pc3.insert(old, pt3.pages_of(0), stamp=1)
    pt3.assign(1, 128)
    pc3.insert(new, pt3.pages_of(1), stamp=2)
    pt3.release(0)
    pt3.release(1)
    hit = pc3.match(old + [9], stamp=3)
    assert len(hit) == 2
    pt3.adopt(2, hit)
    pt3.release(2)
    pt3.assign(3, 128)  # no free page: two evictions
    assert pc3.match(old + [9]) == hit and pc3.match(new + [9]) == []


def test_clear_frees_reclaimable_pages_and_leaves_held_ones():
    pt, pc = _table()
    ids = _toks(128, 7)
    pt.assign(0, 128)
    pc.insert(ids, pt.pages_of(0), stamp=1)
    pt.adopt(1, pc.match(ids + [1]))
    pt.release(0)
    pc.clear()
    assert len(pc) == 0 and pt.free_pages == len(pt._free) == 5  # slot 1 still holds the two
    pt.release(1)
    assert pt.free_pages == len(pt._free) == 7 and sorted(pt._free) == list(range(1, 8))


def test_two_misses_of_one_prefix_leave_every_reclaimable_page_evictable():
    """Two prompts with a common beginning both miss (a burst): the second must not hang its page under
    the first one's entries, whose pages it does not hold -- else the first one's pages would count as
    available after its release yet be unevictable while the second lives."""
    pt, pc = _table(num_pages=8)  # 7 data pages
    shared = _toks(128, 60)
    a, b = shared + _toks(5, 61), shared + _toks(65, 62)
    assert pc.match(a) == [] and pc.match(b) == []
    pt.assign(0, len(a) + 4)  # 3 pages
    pt.assign(1, len(b) + 4)  # 4 pages: the pool is full
    assert pc.insert(a, pt.pages_of(0), stamp=0) == 2
    assert pc.insert(b, pt.pages_of(1), stamp=0) == 0  # its copies of the shared run stay private, and so
    assert not any(pc.holds(pg) for pg in pt.pages_of(1))  # does its third full page
    pt.release(0)
    assert pt.free_pages == 3 and pt.can_fit(192)
    pt.assign(2, 192)  # what is counted as available is there: 1 free page + 2 evictions
    assert pc.evictions == 2 and len(pc) == 0 and len(pt.pages_of(2)) == 3
    pt.release(1)
    pt.release(2)
    assert pt.free_pages == len(pt._free) == 7
    # a sequence that adopted the shared run does hold it: its next page hangs under it
    pt.assign(0, len(a))
    pc.insert(a, pt.pages_of(0), stamp=1)
    hit = pc.match(b, stamp=2)
    pt.adopt(1, hit)
    pt.assign(1, len(b))
    assert pc.insert(b, pt.pages_of(1), stamp=2) == 1 and len(pc) == 3
    pt.release(0)
    assert pt.free_pages == 7 - 4  # slot 1 holds the shared run: nothing of it is reclaimable
    pt.release(1)
    assert pt.free_pages == 7
    pt.assign(2, 64 * 4)
    pt.assign(3, 64 * 3)  # all three entries evicted, child first
    assert pc.evictions == 5 and len(pc) == 0


# ------------------------------------------------------------------ PrefixCache.match
def test_match_exact_numbers():
    pt, pc = _table(num_pages=16)
    prefix = _toks(130, 10)
    a, b = prefix + _toks(7, 11), prefix + _toks(12, 12)
    pt.assign(0, len(a))
    assert pc.match(a) == []
    assert pc.insert(a, pt.pages_of(0), stamp=0) == 2  # 137 tokens: two full pages
    # two prompts sharing their first 130 tokens hit 2 pages = 128 tokens
    assert pc.match(b) == pt.pages_of(0)[:2]
    # re-submitting a 128-token prompt hits 1 page = 64 tokens: its last token is always computed
    c = _toks(128, 13)
    pt.assign(1, 128)
    assert pc.insert(c, pt.pages_of(1), stamp=0) == 2
    assert pc.match(c) == pt.pages_of(1)[:1]
    assert pc.match(c + [4]) == pt.pages_of(1)
    # a 63-token prompt never hits, nor does a 64-token one
    d = _toks(64, 14)
    pt.assign(2, 64)
    assert pc.insert(d[:63], pt.pages_of(2), stamp=0) == 0
    assert pc.insert(d, pt.pages_of(2), stamp=0) == 1
    assert pc.match(d[:63]) == [] and pc.match(d) == [] and pc.match(d + [1]) == pt.pages_of(2)
    # equal in page 2 but different in page 1: nothing (a page's key includes its parent)
    e = list(a)
    e[5] += 1
    assert e[64:128] == a[64:128] and pc.match(e) == []
    # inserting a chain again adds nothing and keeps the first pages
    pt.assign(3, len(b))
    assert pc.insert(b, pt.pages_of(3), stamp=1) == 0 and pc.match(b) == pt.pages_of(0)[:2]


def test_equal_hashes_do_not_alias(monkeypatch):
    monkeypatch.setattr(PC, "_key_hash", lambda tokens: 7)  # every page's key collides
    pt, pc = _table(num_pages=16)
    x, y = _toks(64, 20), _toks(64, 21)
    assert x != y and hash(PC._Key(x)) == hash(PC._Key(y)) == 7
    pt.assign(0, 64)
    pt.assign(1, 64)
    pc.insert(x, pt.pages_of(0), stamp=0)
    assert pc.match(y + [1]) == []  # the same hash alone is no hit
    pc.insert(y, pt.pages_of(1), stamp=0)
    assert pc.match(x + [1]) == pt.pages_of(0) and pc.match(y + [1]) == pt.pages_of(1)


# ------------------------------------------------------------------ serving
PREFIX = _toks(130, 30)


def _requests():
    """The mix of test_prefill_chunk_cpu.py (a long prompt and three short ones, one of them sampled)
    plus three prompts that share a 130-token prefix (one sampled) and two unrelated 130-token ones."""
    g = torch.Generator().manual_seed(5)
    long_ids = torch.randint(3, 2000, (60,), generator=g).tolist()
    shorts = [torch.randint(3, 2000, (n,), generator=g).tolist() for n in (5, 11, 3)]
    return [(PREFIX + _toks(7, 31), GenParams(max_new_tokens=5)),
            (long_ids, GenParams(max_new_tokens=5)),
            (PREFIX + _toks(12, 32), GenParams(6, top_k=5, temperature=0.7, seed=9)),
            (shorts[0], GenParams(max_new_tokens=4)),
            (shorts[1], GenParams(6, top_k=5, temperature=0.7, seed=9)),
            (PREFIX + _toks(3, 33), GenParams(max_new_tokens=4)),
            (_toks(130, 34), GenParams(max_new_tokens=4)),
            (shorts[2], GenParams(max_new_tokens=3)),
            (_toks(131, 35), GenParams(6, top_k=8, temperature=0.9, seed=2)),
            (PREFIX + _toks(9, 36), GenParams(max_new_tokens=5))]


def _it(eng):
    eng.run_iteration(eng._leader_admissions())


def _drive(eng, reqs):
    """The scheduler loop stepped from the test, as test_prefill_chunk_cpu.py drives it: the first
    request, two iterations, then everything else at once (admitted as slots and pages allow)."""
    futs = [eng.submit(*reqs[0])]
    _it(eng)
    _it(eng)
    futs += [eng.submit(ids, gp) for ids, gp in reqs[1:]]
    for _ in range(400):
        if all(f.done() for f in futs):
            break
        _it(eng)
    return [f.result(timeout=0) for f in futs]


def _serial(eng, reqs):
    """One request at a time: each retires before the next is admitted."""
    outs = []
    for ids, gp in reqs:
        f = eng.submit(ids, gp)
        for _ in range(100):
            if f.done():
                break
            _it(eng)
        outs.append(f.result(timeout=0))
    return outs


@pytest.fixture(scope="module")
def want(params):
    """What prefix_cache=False emits (computed once; the schedule does not change a request's tokens)."""
    cfg, p = params
    eng = ContinuousLlama(_model(cfg, p))
    assert "prefix_hits" not in eng.stats()
    return _drive(eng, _requests())


def _end_state(eng):
    st, pages = eng.stats(), eng.m.pages
    assert st["active"] == 0 and eng.failures == 0
    assert st["kv_pages_free"] == PAGES - 1  # every page is free or reclaimable
    assert len(pages._free) + st["prefix_cached_pages"] == PAGES - 1
    assert all(pages.refcount(pg) == 0 for pg in range(PAGES))
    eng.prefix.clear()
    assert eng.stats()["prefix_cached_pages"] == 0 and pages.free_pages == len(pages._free) == PAGES - 1


@pytest.mark.parametrize("speculate", [0, 2])
@pytest.mark.parametrize("prefill_chunk", [0, 16])
def test_serving_matches_prefix_cache_off(params, want, prefill_chunk, speculate):
    cfg, p = params
    eng = ContinuousLlama(_model(cfg, p), prefix_cache=True, prefill_chunk=prefill_chunk, speculate=speculate)
    got = _drive(eng, _requests())
    assert got == want  # greedy and sampled alike
    st = eng.stats()
    print(prefill_chunk, speculate, {k: v for k, v in st.items() if k.startswith("prefix")})
    assert st["prefix_queries"] == 10 and st["prefix_hits"] >= 1 and st["prefix_hit_tokens"] == 128 * st["prefix_hits"]
    assert st["prefix_evictions"] > 0  # five data pages: the index has to give pages back
    _end_state(eng)


@pytest.mark.parametrize("speculate", [0, 2])
@pytest.mark.parametrize("prefill_chunk", [0, 16])
def test_serial_schedule_exact_hits_and_evictions(params, want, prefill_chunk, speculate):
    """One request at a time over 5 data pages.  By hand: request 0 (137 tokens) indexes the prefix's 2
    pages; requests 2 and 5 hit them (128 tokens each) and add nothing; 1, 3, 4, 7 fill no page.  Request 6
    (130 other tokens, 3 pages) finds 3 free and indexes 2 more: 4 cached, 1 free.  Request 8 (131 other
    tokens) needs 3 with 1 free: 2 evictions, the least recently used -- the prefix's pages, last stamped by
    request 5 -- then indexes its own 2.  Request 9 shares the prefix again but finds it gone: a miss, 3
    pages with 1 free, 2 more evictions (request 6's).  Hits: 2 requests, 256 tokens; evictions: 4."""
    cfg, p = params
    eng = ContinuousLlama(_model(cfg, p), prefix_cache=True, prefill_chunk=prefill_chunk, speculate=speculate)
    assert _serial(eng, _requests()) == want
    st = eng.stats()
    assert (st["prefix_queries"], st["prefix_hits"], st["prefix_hit_tokens"]) == (10, 2, 256)
    assert st["prefix_evictions"] == 4 and st["prefix_cached_pages"] == 4
    _end_state(eng)


@pytest.mark.parametrize("prefill_chunk", [0, 16])
def test_same_batch_burst_in_a_tight_pool(params, prefill_chunk):
    """Two prompts with one 128-token beginning admitted in the same batch both miss; the short one
    retires, and an unrelated request that needs the pages it leaves is admitted while the long one still
    decodes (7 data pages: 4 held, 1 free, 2 to evict).  Nothing fails and the tokens are those of
    prefix_cache off."""
    cfg, p = params
    shared = _toks(128, 70)
    reqs = [(shared + _toks(5, 71), GenParams(max_new_tokens=2)),
            (shared + _toks(65, 72), GenParams(8, top_k=5, temperature=0.7, seed=3)),
            (_toks(130, 73), GenParams(max_new_tokens=3)),
            (shared + _toks(9, 74), GenParams(max_new_tokens=3))]

    def run(on):
        m = LlamaTP(p, cfg, max_batch=3, max_seq=256, kv_pages=8)
        eng = ContinuousLlama(m, prefix_cache=on, prefill_chunk=prefill_chunk)
        futs = [eng.submit(*r) for r in reqs[:2]]
        held_mid = None
        for _ in range(100):
            _it(eng)
            assert not on or m.pages.free_pages == len(m.pages._free) + sum(
                m.pages.refcount(pg) == 0 for pg in range(1, 8) if eng.prefix.holds(pg))
            if futs[0].done() and len(futs) == 2:
                assert not futs[1].done()  # the long one is mid-decode when the others arrive
                futs += [eng.submit(*r) for r in reqs[2:]]
                held_mid = m.pages.pages_of(1)
            if all(f.done() for f in futs) and len(futs) == 4:
                break
        assert eng.failures == 0 and len(held_mid) == 4
        return eng, [f.result(timeout=0) for f in futs]

    _e, want = run(False)
    eng, got = run(True)
    assert got == want
    st = eng.stats()
    assert st["prefix_queries"] == 4 and st["prefix_evictions"] >= 2 and st["active"] == 0
    assert st["kv_pages_free"] == 7


def test_shared_pages_are_never_written(params):
    """The K / V rows of the shared pages, snapshot after the first request's prefill, are bit-identical
    after further hitting requests have prefilled (one-shot and in chunks), decoded, verified with drafts
    that are always rejected, and retired."""
    cfg, p = params
    for prefill_chunk in (0, 16):
        m = _model(cfg, p)
        wrong = lambda tokens, n: [1] * n  # noqa: E731 -- token 1 is never sampled from these prompts' top-k
        eng = ContinuousLlama(m, prefix_cache=True, prefill_chunk=prefill_chunk, speculate=2, drafter=wrong)
        first = eng.submit(PREFIX + _toks(7, 31), GenParams(max_new_tokens=5))
        while not len(eng.prefix):  # until the iteration whose prefill / last chunk indexes the prompt
            _it(eng)
        shared = m.pages.pages_of(0)[:2]
        assert all(eng.prefix.holds(pg) for pg in shared) and len(eng.prefix) == 2
        idx = torch.tensor(shared)
        snap = [(k[idx].clone(), v[idx].clone()) for k, v in zip(m.k_cache, m.v_cache)]
        assert all(k.abs().sum() > 0 for k, _v in snap)
        futs = [first] + [eng.submit(PREFIX + _toks(n, 40 + n), GenParams(max_new_tokens=6)) for n in (1, 12, 30)]
        for _ in range(200):
            if all(f.done() for f in futs):
                break
            _it(eng)
        assert all(f.done() for f in futs)
        st = eng.stats()
        assert st["prefix_hits"] == 3 and st["prefix_hit_tokens"] == 384 and st["prefix_evictions"] == 0
        assert st["spec_steps"] > 0 and st["spec_drafted"] > 0 and st["spec_accepted"] == 0  # all drafts rejected
        for (k0, v0), k, v in zip(snap, m.k_cache, m.v_cache):
            assert torch.equal(k[idx], k0) and torch.equal(v[idx], v0)


def test_failed_iteration_clears_the_index(params):
    cfg, p = params
    m = _model(cfg, p)
    eng = ContinuousLlama(m, prefix_cache=True)
    _serial(eng, _requests()[:1])
    assert len(eng.prefix) == 2
    f = eng.submit(PREFIX + _toks(4, 50), GenParams(max_new_tokens=3))
    boom = RuntimeError("injected")

    def fail(*a, **kw):
        raise boom

    step, m.step = m.step, fail
    _it(eng)
    m.step = step
    assert eng.failures == 1 and f.exception(timeout=0) is boom
    assert len(eng.prefix) == 0 and m.pages.free_pages == len(m.pages._free) == PAGES - 1
    assert _serial(eng, [(PREFIX + _toks(4, 50), GenParams(max_new_tokens=3))])[0]  # serving goes on


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


def _tp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from mlmicroservicetemplate_amd.models.llama import TPComm

    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = tiny_config(**CFG)
        m = LlamaTP(init_llama_shard(cfg, world, rank, seed=4), cfg, tp=world, rank=rank, comm=TPComm(None, world),
                    max_batch=3, max_seq=MAX_SEQ, kv_pages=PAGES)
        eng = ContinuousLlama(m, channel=_Chan(), prefix_cache=True, prefill_chunk=16)
        log = []  # per admission: (iteration, slot, the slot's whole page list)
        admit = eng._admit

        def logged(seqs):
            admit(seqs)
            log.extend((eng.iterations, s.slot, tuple(m.pages.pages_of(s.slot))) for s in seqs)

        eng._admit = logged
        outs = None
        if rank == 0:
            outs = _drive(eng, _requests())
            eng._stop = True
            assert eng._leader_admissions() is None  # announces the stop
        else:
            assert eng.follow() == 0
        st = {k: v for k, v in eng.stats().items() if k.startswith("prefix") or k == "kv_pages_free"}
        q.put((rank, outs, eng.iterations, log, st))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_tp2_same_pages_and_stats_on_both_ranks(want):
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
    assert res[0][1] == want  # the TP = 1 tokens
    assert res[0][2] == res[1][2]  # the follower replayed every iteration
    assert res[0][3] == res[1][3] and len(res[0][3]) == 10  # identical page lists per admission
    assert res[0][4] == res[1][4] and res[0][4]["prefix_hits"] >= 1 and res[0][4]["kv_pages_free"] == PAGES - 1


# ------------------------------------------------------------------ refusals
def test_refusals(params, tmp_path):
    cfg, p = params
    with pytest.raises(ValueError, match="kv_pages"):
        ContinuousLlama(LlamaTP(p, cfg, max_batch=3, max_seq=MAX_SEQ, kv_pages=0), prefix_cache=True)
    with pytest.raises(ValueError, match="prefix caching.*fp8"):
        ContinuousLlama(LlamaTP(p, cfg, max_batch=3, max_seq=MAX_SEQ, kv_pages=PAGES, kv_dtype="fp8"), prefix_cache=True)
    m = _model(cfg, p)
    ContinuousLlama(m, prefix_cache=True)
    with pytest.raises(ValueError, match="already"):
        ContinuousLlama(m, prefix_cache=True)  # one index per page table

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

    base = "config: tiny\nmax_seq: 128\noverrides:\n  layers: 1\n"
    with pytest.raises(ValueError, match="prefix_cache"):
        plugin(base + "kv_pages: 5\nprefix_cache: maybe\n")
    with pytest.raises(ValueError, match="kv_pages"):
        plugin(base + "prefix_cache: true\n")
    with pytest.raises(ValueError, match="fp8"):
        plugin(base + "kv_pages: 5\nkv_dtype: fp8\nprefix_cache: true\n")
    pl = plugin(base + "kv_pages: 5\nprefix_cache: true\n")
    try:
        assert pl.engine.prefix is not None and pl.describe()["prefix_cache"] is True
        assert pl.engine.stats()["prefix_cached_pages"] == 0
    finally:
        pl.close()
    pl = plugin(base + "kv_pages: 5\n")
    try:
        assert pl.engine.prefix is None and "prefix_hits" not in pl.engine.stats()
    finally:
        pl.close()
