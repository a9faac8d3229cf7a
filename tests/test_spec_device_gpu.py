"""Speculation on device through the model: ``ContinuousLlama(speculate=3, spec_device=True)`` and
``LlamaTP.generate(speculate=3, spec_device=True)`` (one captured graph per verify step: drafter, forward,
gather, acceptance) against the host loop of the same build on a second model of the same weights.

The two arms run the same kernels on the same shapes under the same context bounds (the device arm derives
``max(past + n)`` from what the host knows without the drafts), so their token lists are compared for
equality, list for list, as tests/test_decode_pick_gpu.py compares the device and host decode loops.
Independently of the host arm every served token is checked against the reference backend by the rule of
tests/test_decode_verify_gpu.py (teacher-forced, among the reference's top-8, within 3e-2 of the largest
top-1 magnitude, none left out).

That rule is a rule about greedy tokens, and the requests here include seeded top-8 samples at temperature
0.8, which are not the top-1 by design.  Measured with the recipe below, on the plain non-speculative engine
as on both speculative arms (the three emit the same tokens): the sampled request's tokens sit at reference
ranks 1 to 9, up to 0.58 below the reference's top-1 (the rule's bound is 0.0515), and its token 6 is the
reference's 9th candidate, 0.0075 below the 8th -- the fused top-8 and the reference's differ at their last
place within rounding.  So a sampled token is held to the form of the rule that a top-k sample can meet:
teacher-forced, its reference value no more than the same 3e-2 bound below the reference's k-th largest, every
token checked; which of the k it is, is checked exactly by the equality with the host arm, whose picks are
``LlamaTP.pick_token``'s.  Greedy requests are held to the rule as it stands."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
CFG128 = dict(vocab=2048, layers=2, hidden=512, heads=8, kv_heads=2, head_dim=128, intermediate=1024)
K = 3
NEW = 24


@pytest.fixture(scope="module")
def tiny():
    from mlmicroservicetemplate_amd.models.llama import init_llama_shard, tiny_config

    cfg = tiny_config(**CFG128)
    return cfg, init_llama_shard(cfg, 1, 0, seed=5, device=DEV)


def _llama(tiny, backend="fused", kv_pages=0, max_batch=4, **kw):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    return LlamaTP(p, cfg, backend=backend, device=DEV, max_batch=max_batch, max_seq=512, kv_pages=kv_pages, **kw)


@pytest.fixture(scope="module")
def ref_model(tiny):
    """The reference backend every served token is checked against (its cache is rewritten by each use)."""
    return _llama(tiny, "reference")


def _check_sampled_tokens(ref, prompt, out, top_k):
    """A top-k sampled request (module docstring): every emitted token, teacher-forced through the reference
    backend on the run's own prefix, has a reference value no more than 3e-2 of the largest |top-1 value| below
    the reference's ``top_k``-th largest.  Every token is checked, none is left out."""
    full = torch.tensor(list(prompt) + list(out), dtype=torch.int32, device=DEV).unsqueeze(0)
    S = full.shape[1]
    pos = torch.arange(S, dtype=torch.int32, device=DEV).unsqueeze(0)
    v, i = ref.step(full, pos, torch.tensor([S], dtype=torch.int32, device=DEV), decode=False, k=64,
                    past=torch.zeros(1, dtype=torch.int32, device=DEV), all_rows=True)
    L = len(prompt)
    v, i = v[L - 1: S - 1].float().cpu(), i[L - 1: S - 1].cpu()
    bound = 3e-2 * float(v[:, 0].abs().max())
    worst = 0.0
    for t, tok in enumerate(out):
        hit = (i[t] == int(tok)).nonzero()
        assert hit.numel(), f"token {t} ({tok}) is not among the reference's top-64"
        worst = max(worst, float(v[t, top_k - 1] - v[t, int(hit[0, 0])]))
    assert worst <= bound, (worst, bound)
    return worst / bound


def _check_request(ref, prompt, gp, out):
    if gp.top_k > 1:
        return _check_sampled_tokens(ref, prompt, out, gp.top_k)
    return _check_tokens(ref, prompt, out)


def _check_tokens(ref, prompt, out):
    """Every emitted token, teacher-forced through the reference backend on the run's own prefix, is among
    the reference's top-8 with a value within 3e-2 of the largest |value| of the reference's top-1.  Every
    token is checked, none is left out."""
    full = torch.tensor(list(prompt) + list(out), dtype=torch.int32, device=DEV).unsqueeze(0)
    S = full.shape[1]
    pos = torch.arange(S, dtype=torch.int32, device=DEV).unsqueeze(0)
    v, i = ref.step(full, pos, torch.tensor([S], dtype=torch.int32, device=DEV), decode=False, k=8,
                    past=torch.zeros(1, dtype=torch.int32, device=DEV), all_rows=True)
    L = len(prompt)
    v, i = v[L - 1: S - 1].float().cpu(), i[L - 1: S - 1].cpu()  # row p: the candidates of the token at p + 1
    bound = 3e-2 * float(v.abs().max())
    worst = 0.0
    for t, tok in enumerate(out):
        hit = (i[t] == int(tok)).nonzero()
        assert hit.numel(), f"token {t} ({tok}) is not among the reference's top-8"
        worst = max(worst, float(v[t, 0] - v[t, int(hit[0, 0])]))
    assert worst <= bound, (worst, bound)
    return worst / bound


def _requests():
    from mlmicroservicetemplate_amd.models.llama import GenParams

    g = torch.Generator().manual_seed(5)
    mk = lambda n: torch.randint(3, 2000, (n,), generator=g).tolist()  # noqa: E731
    loop = mk(12)
    return [(mk(150), GenParams(max_new_tokens=NEW)), (loop * 4, GenParams(max_new_tokens=NEW)),  # a prompt that repeats
            (mk(70), GenParams(max_new_tokens=NEW, top_k=8, temperature=0.8, seed=9)),
            (mk(3), GenParams(max_new_tokens=NEW))]


def _serve(model, reqs, first=None, **kw):
    """Drive ``ContinuousLlama._loop`` step by step: every request at once, or the first ``first`` of them two
    iterations ahead of the rest.  Returns the engine, the token lists, the ``.cpu()`` calls on device
    tensors the iterations made and the number of iterations that emitted a token (an iteration that only
    advanced prompts by a chunk has nothing to read back)."""
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    eng = ContinuousLlama(model, speculate=K, **kw)
    calls, worked = [], [0]
    orig = torch.Tensor.cpu

    def iterate():
        before = eng.tokens
        eng.run_iteration(eng._leader_admissions())
        worked[0] += eng.tokens != before

    def counting_cpu(self, *a, **k2):
        if self.is_cuda:
            calls.append(tuple(self.shape))
        return orig(self, *a, **k2)

    torch.Tensor.cpu = counting_cpu
    try:
        futs = [eng.submit(ids, gp) for ids, gp in reqs[:first]]
        if first:
            for _ in range(2):
                iterate()
            futs += [eng.submit(ids, gp) for ids, gp in reqs[first:]]
        for _ in range(400):
            if all(f.done() for f in futs):
                break
            iterate()
    finally:
        torch.Tensor.cpu = orig
    outs = [f.result(timeout=0) for f in futs]
    assert eng.failures == 0 and all(s is None for s in eng.slots)
    return eng, outs, calls, worked[0]


def _same_as_host_arm(tiny, ref_model, reqs, model_kw, eng_kw=None, first=None):
    """The equalities every serving case asserts; returns the device arm's engine and model."""
    eng_kw = eng_kw or {}
    host_eng, host_outs, _, _ = _serve(_llama(tiny, **model_kw), reqs, first, **eng_kw)
    assert not host_eng.dev_mode
    model = _llama(tiny, **model_kw)
    eng, outs, calls, worked = _serve(model, reqs, first, spec_device=True, **eng_kw)
    assert eng.dev_mode is True
    hs, ds = host_eng.stats(), eng.stats()
    print(f"{model_kw} {eng_kw}: host {[hs[k] for k in ('iterations', 'spec_steps', 'spec_drafted', 'spec_accepted')]} "
          f"device {[ds[k] for k in ('iterations', 'spec_steps', 'spec_drafted', 'spec_accepted')]}")
    assert outs == host_outs  # list for list
    for key in ("spec_steps", "spec_drafted", "spec_accepted", "tokens", "iterations"):
        assert ds[key] == hs[key], (key, ds, hs)
    assert ds["spec_accepted"] > 0
    # one device -> host copy per iteration that did work, verify steps included, and no other
    assert len(calls) == worked == eng.host_reads, (len(calls), worked, eng.host_reads, eng.iterations)
    if not eng.prefill_chunk:  # every iteration of the drive emits: it stops with the last result
        assert worked == eng.iterations
    for (prompt, gp), out in zip(reqs, outs):
        assert len(out) == gp.max_new_tokens or out[-1] in eng.eos
        _check_request(ref_model, prompt, gp, out)
    if model.pages is not None:
        assert ds["kv_pages_free"] == ds["kv_pages"] - 1
    assert any(key[0] == "serve_spec" for key in model._dev_graphs)  # the verify steps ran as the fused graph
    assert not model._ver_graphs  # ... and never as the host loop's
    return eng, model


@pytest.mark.parametrize("kv_pages", [0, 24])
def test_serving_device_equals_host_loop(tiny, ref_model, kv_pages):
    _same_as_host_arm(tiny, ref_model, _requests(), dict(kv_pages=kv_pages))


def test_serving_switches_between_decode_and_verify_steps(tiny, ref_model):
    """Six sequences in eight slots: plain decode steps while more than four decode (the pick appends to
    ``hist``), verify steps after -- whose drafter needs the tokens the plain steps emitted."""
    from mlmicroservicetemplate_amd.models.llama import GenParams

    g = torch.Generator().manual_seed(5)
    mk = lambda n: torch.randint(3, 2000, (n,), generator=g).tolist()  # noqa: E731
    loop = mk(12)
    prompts = [mk(20), loop * 3, mk(33), mk(9), loop * 2 + mk(5), mk(50)]
    reqs = [(p, GenParams(max_new_tokens=n)) for p, n in zip(prompts, [6, 24, 9, 20, 24, 12])]
    eng, model = _same_as_host_arm(tiny, ref_model, reqs, dict(max_batch=8))
    assert any(key[0] == "serve_hist" for key in model._dev_graphs)  # plain steps ran, in the hist variant
    assert not any(key[0] == "serve" for key in model._dev_graphs)
    assert 1 <= eng.stats()["spec_steps"] < eng.iterations


def test_serving_chunked_prefill_with_prefix_cache(tiny, ref_model):
    reqs = _requests()
    reqs.append((reqs[0][0][:140] + [7, 8, 9], reqs[0][1]))  # shares two full pages with the first request
    eng, _m = _same_as_host_arm(tiny, ref_model, reqs, dict(kv_pages=24), dict(prefill_chunk=64, prefix_cache=True),
                                first=1)
    assert eng.stats()["prefix_hits"] >= 1


def test_serving_fp8_kv_cache(tiny, ref_model):
    _same_as_host_arm(tiny, ref_model, _requests(), dict(kv_dtype="fp8", kv_prefill="cache"))


def _prompts():
    ids = torch.randint(3, 2000, (3, 150), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    ids[1, 40:131] = ids[1, :40].repeat(3)[:91]  # a row that repeats: prompt lookup has something to find
    return ids.to(DEV), torch.tensor([150, 131, 17], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_generate_device_equals_host_loop(tiny, sampled):
    from mlmicroservicetemplate_amd.models.llama import GenParams

    ids, lens = _prompts()
    gp = GenParams(NEW, top_k=8, temperature=0.8, seed=3) if sampled else GenParams(max_new_tokens=NEW)
    host = _llama(tiny)
    want = host.generate(ids, lens, gp, speculate=K).cpu()
    m = _llama(tiny)
    calls = []
    orig = torch.Tensor.cpu

    def counting_cpu(self, *a, **kw):
        if self.is_cuda:
            calls.append(tuple(self.shape))
        return orig(self, *a, **kw)

    torch.Tensor.cpu = counting_cpu
    try:
        got = m.generate(ids, lens, gp, speculate=K, spec_device=True)
    finally:
        torch.Tensor.cpu = orig
    st = dict(m.spec_stats)
    print(f"sampled={sampled}: host {host.spec_stats} device {st}")
    assert torch.equal(got.to(torch.int32).cpu(), want.to(torch.int32))
    assert st == host.spec_stats and st["steps"] >= 1
    # one [B, K + 3] read-back per step, and the result
    assert calls == [(m.max_batch, K + 3)] * st["steps"] + [(3, NEW)], calls
    again = m.generate(ids, lens, gp, speculate=K, spec_device=True)  # over the first run's stale cache rows
    assert torch.equal(again, got) and m.spec_stats == st


def test_refusals_on_the_fused_backend(tiny, monkeypatch):
    from mlmicroservicetemplate_amd.models.llama import GenParams
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    ids, lens = _prompts()
    m = _llama(tiny)
    assert m._spec_device_ok(4, K + 1, 8)
    ContinuousLlama(m, speculate=K, spec_device=True)  # the supported configuration constructs
    with pytest.raises(ValueError, match="<= 16"):  # what check_speculate refuses
        ContinuousLlama(m, speculate=4, spec_device=True)
    with pytest.raises(ValueError, match="drafter"):
        ContinuousLlama(m, speculate=K, spec_device=True, drafter=lambda toks, n: [0] * n)
    monkeypatch.setenv("MLS_SERVE_DEVICE_PICK", "0")
    with pytest.raises(ValueError, match="MLS_SERVE_DEVICE_PICK"):
        ContinuousLlama(m, speculate=K, spec_device=True)
    monkeypatch.delenv("MLS_SERVE_DEVICE_PICK")
    assert not m._spec_device_ok(4, K + 1, 600)  # tp * k > 512: the gather is too large for the pick
    monkeypatch.setattr(m, "top_k_max", 65)
    with pytest.raises(ValueError, match="device-resident"):
        ContinuousLlama(m, speculate=K, spec_device=True)
    monkeypatch.undo()
    monkeypatch.setattr(m, "use_graphs", False)  # graphs off
    with pytest.raises(ValueError, match="device-resident"):
        ContinuousLlama(m, speculate=K, spec_device=True)
    with pytest.raises(ValueError, match="device-resident"):
        m.generate(ids, lens, GenParams(4), speculate=K, spec_device=True)


# ------------------------------------------------------------------ TP = 2 rehearsal
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_tp2_serving_spec_device(tmp_path, ref_model):
    """Two ranks on this GPU over gloo (tests/spec_device_tp_worker.py): rank 0 schedules, rank 1 follows; the
    engine runs ``speculate=3, spec_device=True`` -- 4 positions x 4 query heads per KV head and rank."""
    from mlmicroservicetemplate_amd.models.llama import GenParams

    world = 2
    root = os.path.dirname(HERE)
    port = _port()
    out = str(tmp_path / "spec")
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OUT=out, TP_CFG=json.dumps(CFG128), MLS_CUSTOM_AR="1",
                   PYTHONPATH=os.pathsep.join([root, os.environ.get("PYTHONPATH", "")]))
        # each rank under its own time limit
        procs.append(subprocess.Popen(["timeout", "-k", "10", "150", sys.executable,
                                       os.path.join(HERE, "spec_device_tp_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        o, _ = p.communicate()
        logs.append((p.returncode, o[-3000:]))
        if p.returncode != 0:  # stop at the first non-zero exit
            for q in procs:
                if q.poll() is None:
                    q.kill()
                    q.communicate()
            break
    assert all(rc == 0 for rc, _ in logs) and len(logs) == world, logs
    infos = []
    for r in range(world):
        d = torch.load(out + f".{r}.pt", weights_only=True)
        infos.append(json.loads(d["info"]))
        if r == 0:
            results, reqs = json.loads(d["results"]), json.loads(d["reqs"])
    print(infos)
    for i in infos:
        assert i["dev_mode"] == 1 and i["failures"] == 0, infos
        assert i["host_reads"] <= i["iterations"] and i["cpu_calls"] <= i["iterations"], infos
    assert len({i["iterations"] for i in infos}) == 1, infos
    assert infos[0]["spec"] == infos[1]["spec"] and infos[0]["spec"]["spec_accepted"] > 0, infos
    if all(i["car"] for i in infos):  # the IPC all-reduce is up: the headers ride the spec graph's gather
        f = infos[1]["follower"]
        assert f["carried_headers"] > 0 and f["iters_no_admit_bcast"] == 0, infos
    assert len(results) == len(reqs) == 6
    for (prompt, gpl), got in zip(reqs, results):
        assert isinstance(got, list) and (len(got) == gpl[0] or got[-1] == 2), results  # 2: the tiny config's EOS
        _check_request(ref_model, prompt, GenParams(*gpl), got)
