"""LoRA on all seven linear projections (``lora={"targets": "all"}``) on the CPU, reference backend, the tiny
config of tests/test_lora_cpu.py: the rule against host-merged weights, a mixed batch against each row alone
and against TP = 2 over gloo, the refusals and the loader's four new PEFT names."""
import json
import os

import pytest
import torch
import torch.multiprocessing as mp

from mlmicroservicetemplate_amd.models import llama as M
from mlmicroservicetemplate_amd.ops import reference as R
from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin
from mlmicroservicetemplate_amd.utils.checkpoint import load_lora_adapter, save_state
from test_lora_tp_cpu import _port

CFG = M.tiny_config()
LORA = {"max_adapters": 3, "max_rank": 8, "targets": "all"}
GP = M.GenParams(6, adapter=[-1, 0, 1])  # a mixed batch: base, adapter 0, adapter 1
TP_CFG = dict(vocab=2048, hidden=256, layers=2, heads=8, kv_heads=4, head_dim=32, intermediate=512)


def _adapters(cfg=CFG):
    return [M.random_lora_adapter(cfg, 8, seed=21, modules=R.LORA_ALL_MODULES, b_std=0.05),
            M.random_lora_adapter(cfg, 4, seed=22, modules=("v", "o", "up", "down"), alpha=24.0, b_std=0.05)]


def _model(params, cfg=CFG, lora=LORA, **kw):
    m = M.LlamaTP(params, cfg, max_batch=4, max_seq=160, lora=lora, **kw)
    for i, (t, c) in enumerate(_adapters(cfg)):
        m.load_adapter(i, t, c)
    return m


def _prompts():
    return torch.randint(3, 2000, (3, 12), generator=torch.Generator().manual_seed(7)), torch.tensor([12, 7, 3])


def _merged(p, t, c):
    """fp32 ``W + s B A`` for every target module."""
    mods, r, alpha, rs = M.parse_lora_config(c, targets="all")
    s, D, out = R.lora_scale(alpha, r, rs), CFG.head_dim, dict(p)
    q0 = {"q": 0, "k": CFG.heads * D, "v": (CFG.heads + CFG.kv_heads) * D}
    for i in range(CFG.layers):
        for m_ in mods:
            d = s * (t[f"l{i}.{m_}.lora_B"] @ t[f"l{i}.{m_}.lora_A"])
            name = f"l{i}.qkv" if m_ in q0 else f"l{i}.{m_}"
            w = out[name].clone()
            w[q0.get(m_, 0): q0.get(m_, 0) + d.shape[0]] += d
            out[name] = w
    return out


@pytest.mark.parametrize("adapter", [0, 1])
def test_tokens_equal_merged_weights(adapter):
    p = M.init_llama_shard(CFG, seed=5, dtype=torch.float32)
    lora = _model(p)
    ref = M.LlamaTP(_merged(p, *_adapters()[adapter]), CFG, max_batch=4, max_seq=160)
    base = M.LlamaTP(p, CFG, max_batch=4, max_seq=160)
    ids, lens = _prompts()
    for kw in ({}, dict(top_k=20, temperature=0.8, seed=3)):
        want = ref.generate(ids, lens, M.GenParams(6, **kw)).tolist()
        assert lora.generate(ids, lens, M.GenParams(6, adapter=adapter, **kw)).tolist() == want
        assert want != base.generate(ids, lens, M.GenParams(6, **kw)).tolist()  # the adapter matters


def _tp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    torch.set_num_threads(1)  # fixed summation order: exact token equality across runs
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = M.tiny_config(**TP_CFG)
        m = _model(M.init_llama_shard(cfg, world, rank, seed=1), cfg, tp=world, rank=rank, comm=M.TPComm(None, world))
        q.put(m.generate(*_prompts(), GP).tolist())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_mixed_batch_rows_get_their_own_tokens_and_tp2_matches_tp1():
    torch.set_num_threads(1)
    cfg = M.tiny_config(**TP_CFG)
    one, (ids, lens) = _model(M.init_llama_shard(cfg, 1, 0, seed=1), cfg), _prompts()
    want = one.generate(ids, lens, GP).tolist()
    for b, a in enumerate(GP.adapter):  # each row of the mixed batch gets the tokens it gets alone
        assert one.generate(ids[b: b + 1], lens[b: b + 1], M.GenParams(6, adapter=a)).tolist()[0] == want[b]
    ctx, port = mp.get_context("spawn"), _port()
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=200) for _ in range(2)]
    for pr in procs:
        pr.join(30)
        assert pr.exitcode == 0
    assert res == [want, want]


def test_refusals():
    p = M.init_llama_shard(CFG, seed=5)
    t, c = _adapters()[0]
    qkv = M.LlamaTP(p, CFG, max_batch=4, max_seq=160, lora={"max_adapters": 2, "max_rank": 8})
    with pytest.raises(ValueError, match="o_proj"):
        qkv.load_adapter(0, t, c)
    with pytest.raises(ValueError, match="targets"):
        M.LlamaTP(p, CFG, max_batch=4, max_seq=160, lora=dict(LORA, targets="mlp"))
    with pytest.raises(ValueError, match="lora_targets"):
        LlamaPlugin.parse_lora({"lora": {"a": "/x"}, "lora_targets": "mlp"})
    with pytest.raises(ValueError, match="prefix_cache"):
        LlamaPlugin.parse_lora({"lora": {"a": "/x"}, "lora_targets": "all"}, prefix_cache=True)
    assert LlamaPlugin.parse_lora({"lora": {"a": "/x"}, "lora_targets": "all"})[1]["targets"] == "all"


def test_loader_round_trips_the_peft_names(tmp_path):
    t, c = _adapters()[1]
    block = {"v": "self_attn", "o": "self_attn", "up": "mlp", "down": "mlp"}
    names = {k: "base_model.model.model.layers.{}.{}.{}_proj.lora_{}.weight".format(
        k[1:].split(".")[0], block[k.split(".")[1]], k.split(".")[1], k[-1]) for k in t}
    save_state(str(tmp_path / "adapter_model.safetensors"), {names[k]: v for k, v in t.items()})
    with open(tmp_path / "adapter_config.json", "w") as f:
        json.dump(dict(c, peft_type="LORA", bias="none"), f)
    got, cfg = load_lora_adapter(str(tmp_path), CFG.layers, targets="all")
    assert set(got) == set(t) and all(torch.equal(got[k], t[k].float()) for k in t)
    with pytest.raises(ValueError, match="o_proj"):  # the default still refuses, as the q / k / v model does
        load_lora_adapter(str(tmp_path), CFG.layers)
    M.LlamaTP(M.init_llama_shard(CFG, seed=5), CFG, max_batch=4, max_seq=160, lora=LORA).load_adapter(0, got, cfg)
