"""Per-request LoRA adapters on the CPU (reference backend, tiny model): the rule against merged weights, a
mixed continuous batch against each request served alone, the adapter loader and every refusal."""
import json
import os

import pytest
import torch

from mlmicroservicetemplate_amd.models import llama as M
from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama
from mlmicroservicetemplate_amd.ops import reference as R
from mlmicroservicetemplate_amd.utils.checkpoint import CheckpointError, load_lora_adapter, save_state

CFG = M.tiny_config()
A, B_ = 0, 1


def _adapters(zero_b=False):
    ta, ca = M.random_lora_adapter(CFG, 8, seed=21, b_std=0.05)
    tb, cb = M.random_lora_adapter(CFG, 4, seed=22, modules=("q", "v"), alpha=24.0, b_std=0.05)
    cb["use_rslora"] = True
    if zero_b:
        ta = {k: (torch.zeros_like(v) if k.endswith("lora_B") else v) for k, v in ta.items()}
    return [(ta, ca), (tb, cb)]


def _model(params=None, adapters=None, dtype=torch.bfloat16, **kw):
    params = M.init_llama_shard(CFG, seed=5, dtype=dtype) if params is None else params
    m = M.LlamaTP(params, CFG, max_batch=4, max_seq=160, lora={"max_adapters": 3, "max_rank": 8}, **kw)
    for i, (t, c) in enumerate(_adapters() if adapters is None else adapters):
        m.load_adapter(i, t, c)
    return m


def _prompts():
    g = torch.Generator().manual_seed(11)
    return [torch.randint(3, 2000, (n,), generator=g).tolist() for n in (9, 70, 17, 33, 21, 40)]


def _alone(m, ids, gp, **kw):
    return m.generate(torch.tensor([ids]), torch.tensor([len(ids)]), gp, **kw)[0].tolist()


# ------------------------------------------------------------------------------------------ merged weights
@pytest.mark.parametrize("adapter", [A, B_])
def test_all_slots_on_one_adapter_equal_merged_weights(adapter):
    """fp32 weights; the reference model whose qkv is ``W + s B A`` must give the same logits up to fp32
    reassociation -- 1e-4 of max|logit| (sums of 256-512 terms regrouped through 2 layers: a few hundred times
    2^-24) -- and the same greedy token wherever the top-2 margin exceeds twice that."""
    p = M.init_llama_shard(CFG, seed=5, dtype=torch.float32)
    t, c = _adapters()[adapter]
    mods, r, alpha, rs = M.parse_lora_config(c)
    s = R.lora_scale(alpha, r, rs)
    assert s != 1.0
    merged = dict(p)
    D = CFG.head_dim
    rows = {"q": slice(0, CFG.heads * D), "k": slice(CFG.heads * D, (CFG.heads + CFG.kv_heads) * D),
            "v": slice((CFG.heads + CFG.kv_heads) * D, (CFG.heads + 2 * CFG.kv_heads) * D)}
    for i in range(CFG.layers):
        w = p[f"l{i}.qkv"].clone()
        for m_ in mods:
            w[rows[m_]] += s * (t[f"l{i}.{m_}.lora_B"] @ t[f"l{i}.{m_}.lora_A"])
        merged[f"l{i}.qkv"] = w
    lora, ref = _model(p, dtype=torch.float32), M.LlamaTP(merged, CFG, max_batch=4, max_seq=160)
    lora.keep_logits = ref.keep_logits = True
    for ids in _prompts()[:3]:
        out = _alone(ref, ids, M.GenParams(6))
        full = torch.tensor([ids + out], dtype=torch.int32)
        S = full.shape[1]
        pos = torch.arange(S, dtype=torch.int32).unsqueeze(0)
        kw = dict(decode=False, k=2, past=torch.zeros(1, dtype=torch.int32), all_rows=True)
        lora.set_slot_adapter(0, adapter)
        v1, i1 = lora.step(full, pos, torch.tensor([S], dtype=torch.int32), **kw)
        l1 = lora.last_logits
        v0, i0 = ref.step(full, pos, torch.tensor([S], dtype=torch.int32), **kw)
        tol = 1e-4 * float(ref.last_logits.abs().max())
        assert float((l1 - ref.last_logits).abs().max()) <= tol
        clear = (v0[:, 0] - v0[:, 1]) > 2 * tol
        assert clear.sum() >= S // 2 and torch.equal(i1[clear, 0], i0[clear, 0])
        # greedy tokens: equal up to the first generated position whose margin is not clear (none, on these
        # prompts: asserted, so the comparison covers all six tokens)
        gen_clear = clear[len(ids) - 1: S - 1]
        assert bool(gen_clear.all()), gen_clear
        assert _alone(lora, ids, M.GenParams(6, adapter=adapter)) == out


def test_zero_b_adapter_gives_the_base_tokens():
    base = M.LlamaTP(M.init_llama_shard(CFG, seed=5), CFG, max_batch=4, max_seq=160)
    m = _model(adapters=_adapters(zero_b=True))
    for ids in _prompts()[:3]:
        assert _alone(m, ids, M.GenParams(6, adapter=A)) == _alone(base, ids, M.GenParams(6))


def test_no_adapter_loaded_computes_nothing_new(monkeypatch):
    calls = []
    inner = R.lora_qkv
    monkeypatch.setattr(R, "lora_qkv", lambda *a, **kw: calls.append(1) or inner(*a, **kw))
    m = M.LlamaTP(M.init_llama_shard(CFG, seed=5), CFG, max_batch=4, max_seq=160, lora={"max_adapters": 2})
    _alone(m, _prompts()[0], M.GenParams(3))
    assert not calls and m.lora_slot.tolist() == [-1] * 4
    m.load_adapter(0, *_adapters()[0])
    _alone(m, _prompts()[0], M.GenParams(3, adapter=0))
    assert calls


# ------------------------------------------------------------------------------------- continuous batching
def _requests():
    ps = _prompts()
    gp = lambda a, **kw: M.GenParams(max_new_tokens=5, adapter=a, **kw)  # noqa: E731
    return [[(ps[0], gp(A)), (ps[1], gp(-1)), (ps[2], gp(B_))],
            [(ps[3], gp(B_, top_k=4, temperature=0.8, seed=3)), (ps[4], gp(-1)), (ps[5], gp(A, top_k=3, seed=9))]]


def _drive(eng):
    waves = _requests()
    reqs, futs = list(waves[0]), [eng.submit(*r) for r in waves[0]]
    for _ in range(3):
        eng.run_iteration(eng._leader_admissions())
    reqs += waves[1]
    futs += [eng.submit(*r) for r in waves[1]]
    for _ in range(80):
        if all(f.done() for f in futs):
            break
        eng.run_iteration(eng._leader_admissions())
    assert eng.failures == 0
    return reqs, [f.result(timeout=0) for f in futs]


@pytest.fixture(scope="module")
def alone():
    """Every request served alone (greedy and sampled), and the proof that adapters matter on every prompt: the
    base model's tokens fail the top-8 / 3e-2 rule of test_prefix_cache_gpu.py against a's reference, a's against b's."""
    m = _model()
    outs = {}
    for w in _requests():
        for ids, gp in w:
            outs[tuple(ids)] = _alone(m, ids, gp)
    for ids in _prompts():
        gen = {a: _alone(m, ids, M.GenParams(5, adapter=a)) for a in (-1, A, B_)}
        assert not _passes(m, A, ids, gen[-1]) and not _passes(m, B_, ids, gen[A])
        assert _passes(m, A, ids, gen[A]) and _passes(m, -1, ids, gen[-1])
    return outs


def _passes(ref, adapter, prompt, out) -> bool:
    ref.set_slot_adapter(0, adapter)
    full = torch.tensor([list(prompt) + list(out)], dtype=torch.int32)
    S = full.shape[1]
    v, i = ref.step(full, torch.arange(S, dtype=torch.int32).unsqueeze(0), torch.tensor([S], dtype=torch.int32),
                    decode=False, k=8, past=torch.zeros(1, dtype=torch.int32), all_rows=True)
    L = len(prompt)
    v, i = v[L - 1: S - 1].float(), i[L - 1: S - 1]
    bound = 3e-2 * float(v.abs().max())
    for t, tok in enumerate(out):
        hit = (i[t] == int(tok)).nonzero()
        if not hit.numel() or float(v[t, 0] - v[t, int(hit[0, 0])]) > bound:
            return False
    return True


@pytest.mark.parametrize("kv_pages,prefill_chunk,speculate", [(0, 0, 0), (12, 0, 0), (12, 32, 0), (0, 32, 0), (0, 0, 3),
                                                              (12, 32, 3)])
def test_mixed_batch_equals_each_request_alone(alone, kv_pages, prefill_chunk, speculate):
    m = _model(kv_pages=kv_pages)
    eng = ContinuousLlama(m, prefill_chunk=prefill_chunk, speculate=speculate)
    reqs, outs = _drive(eng)
    for (ids, gp), out in zip(reqs, outs):
        assert out == alone[tuple(ids)], (gp.adapter, gp.top_k)
    assert m.lora_slot.tolist() == [-1] * 4


# --------------------------------------------------------------------------------------- loader, refusals
def _peft_dir(path, tensors, config, native=False):
    os.makedirs(path, exist_ok=True)
    def name(k):
        i, p, ab = k[1:].split(".")[0], k.split(".")[1], k[-1]
        return k if native else f"base_model.model.model.layers.{i}.self_attn.{p}_proj.lora_{ab}.weight"
    save_state(os.path.join(path, "adapter_model.safetensors"), {name(k): v for k, v in tensors.items()})
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(dict(config, peft_type="LORA", bias="none"), f)
    return str(path)


@pytest.mark.parametrize("native", [False, True])
def test_loader_round_trip(tmp_path, native):
    t, c = _adapters()[1]
    got, cfg = load_lora_adapter(_peft_dir(tmp_path / "b", t, c, native), CFG.layers)
    assert set(got) == set(t) and all(torch.equal(got[k], t[k].float()) for k in t)
    m = _model(adapters=[])
    m.load_adapter(0, got, cfg)
    ids = _prompts()[0]
    assert _alone(m, ids, M.GenParams(5, adapter=0)) == _alone(_model(), ids, M.GenParams(5, adapter=B_))


def test_loader_refusals(tmp_path):
    t, c = _adapters()[0]
    with pytest.raises(CheckpointError, match="adapter_config"):
        load_lora_adapter(str(tmp_path / "nothing"), CFG.layers)
    d = _peft_dir(tmp_path / "bin", t, c)
    os.rename(os.path.join(d, "adapter_model.safetensors"), os.path.join(d, "adapter_model.bin"))
    with pytest.raises(CheckpointError, match="adapter_model.bin"):
        load_lora_adapter(d, CFG.layers)
    o = dict(t, **{"l0.o.lora_A": t["l0.q.lora_A"].clone(), "l0.o.lora_B": t["l0.q.lora_B"].clone()})
    os.makedirs(tmp_path / "o")
    save_state(str(tmp_path / "o" / "adapter_model.safetensors"),
               {f"model.layers.{k[1:].split('.')[0]}.self_attn.{k.split('.')[1]}_proj.lora_{k[-1]}.weight": v
                for k, v in o.items()})
    with open(tmp_path / "o" / "adapter_config.json", "w") as f:
        json.dump(c, f)
    with pytest.raises(CheckpointError, match="o_proj"):
        load_lora_adapter(str(tmp_path / "o"), CFG.layers)
    with pytest.raises(CheckpointError, match="rank"):
        load_lora_adapter(_peft_dir(tmp_path / "r", t, dict(c, r=4)), CFG.layers)
    with pytest.raises(CheckpointError, match="layer 1"):
        load_lora_adapter(_peft_dir(tmp_path / "l", t, c), 1)
    with pytest.raises(CheckpointError, match="missing"):
        load_lora_adapter(_peft_dir(tmp_path / "m", {k: v for k, v in t.items() if not k.startswith("l1.v")}, c),
                          CFG.layers)


@pytest.mark.parametrize("change,match", [
    ({"target_modules": ["q_proj", "o_proj"]}, "o_proj"),
    ({"target_modules": ["gate_proj"]}, "gate_proj"),
    ({"modules_to_save": ["lm_head"]}, "modules_to_save"),
    ({"bias": "all"}, "bias"),
    ({"use_dora": True}, "DoRA"),
    ({"rank_pattern": {"layers.0.self_attn.q_proj": 4}}, "rank_pattern"),
    ({"r": 65}, "rank"),
    ({"r": 0}, "rank"),
])
def test_config_refusals(change, match):
    t, c = _adapters()[0]
    m = _model(adapters=[])
    with pytest.raises(ValueError, match=match):
        m.load_adapter(0, t, dict(c, **change))
    assert not m.lora_loaded


def test_model_refusals():
    t, c = _adapters()[0]
    m = _model(adapters=[])
    with pytest.raises(ValueError, match="max_adapters"):
        m.load_adapter(3, t, c)
    t16, c16 = M.random_lora_adapter(CFG, 16, seed=1)
    with pytest.raises(ValueError, match="max_rank"):
        m.load_adapter(0, t16, c16)
    with pytest.raises(ValueError, match="do not match"):
        m.load_adapter(0, dict(t, **{"l1.k.lora_B": t["l1.q.lora_B"]}), c)
    with pytest.raises(ValueError, match="no tensor"):
        m.load_adapter(0, {k: v for k, v in t.items() if k != "l0.v.lora_A"}, c)
    with pytest.raises(ValueError, match="without lora"):
        M.LlamaTP(M.init_llama_shard(CFG, seed=5), CFG).load_adapter(0, t, c)
    m.load_adapter(0, t, c)
    for slot, idx, match in ((4, 0, "slot"), (-1, 0, "slot"), (0, 1, "not loaded"), (0, -2, "not loaded")):
        with pytest.raises(ValueError, match=match):
            m.set_slot_adapter(slot, idx)
    with pytest.raises(ValueError, match="not loaded"):
        _alone(m, [5, 6, 7], M.GenParams(2, adapter=2))
    with pytest.raises(ValueError, match="not loaded"):
        ContinuousLlama(m).submit([5, 6, 7], M.GenParams(2, adapter=1))
    with pytest.raises(ValueError, match="prefix_cache"):
        ContinuousLlama(_model(kv_pages=12), prefix_cache=True)
    assert m.lora_slot.tolist() == [-1] * 4


def test_a_failed_iteration_leaves_every_slot_on_the_base_model(monkeypatch):
    m = _model()
    eng = ContinuousLlama(m)
    futs = [eng.submit(ids, gp) for ids, gp in _requests()[0]]
    monkeypatch.setattr(m, "step", lambda *a, **kw: (_ for _ in ()).throw(RuntimeError("boom")))
    eng.run_iteration(eng._leader_admissions())
    assert eng.failures == 1 and all(f.exception() is not None for f in futs)
    assert m.lora_slot.tolist() == [-1] * 4 and all(s is None for s in eng.slots)
