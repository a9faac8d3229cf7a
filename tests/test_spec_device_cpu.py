"""Speculation on device (``spec_device``), the part that needs no GPU: the option exists, refuses what it
cannot serve with a ``ValueError`` at construction (nothing falls back to the host loop), leaves
``speculate`` without it exactly as it was (host path, ``tp > 1`` refused with the same message), and
MODEL_CONFIG ``speculate_device`` is parsed and reported.  On this backend (reference, CPU) the device
loop does not exist, so a well-formed request is itself one of the refusals."""
import multiprocessing as mp
import os
import socket

import pytest
import torch

from mlmicroservicetemplate_amd.models import speculative as SP
from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

CFG128 = dict(vocab=2048, layers=2, hidden=512, heads=8, kv_heads=2, head_dim=128, intermediate=1024)
K = 3


@pytest.fixture(scope="module")
def params():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG128)
    return cfg, init_llama_shard(cfg, 1, 0, seed=5)


@pytest.fixture(scope="module")
def model(params):
    cfg, p = params
    return LlamaTP(p, cfg, max_batch=4, max_seq=128)


def _prompts():
    ids = torch.randint(3, 2000, (2, 9), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    return ids, torch.tensor([9, 4], dtype=torch.int32)


def test_engine_refusals(params, model, monkeypatch):
    with pytest.raises(ValueError, match="speculate >= 1"):
        ContinuousLlama(model, spec_device=True)  # speculate == 0
    with pytest.raises(ValueError, match="drafter"):  # a host hook cannot run inside the graph
        ContinuousLlama(model, speculate=K, spec_device=True, drafter=SP.make_prompt_lookup(2))
    with pytest.raises(ValueError, match="device-resident"):  # reference backend on the CPU: no device loop
        ContinuousLlama(model, speculate=K, spec_device=True)
    with pytest.raises(ValueError, match=r"speculate must be in \[1, 7\]"):  # what check_speculate refuses
        ContinuousLlama(model, speculate=8, spec_device=True)
    cfg, p = params
    m8 = LlamaTP(p, cfg, max_batch=2, max_seq=64, kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        ContinuousLlama(m8, speculate=K, spec_device=True)
    monkeypatch.setenv("MLS_SERVE_DEVICE_PICK", "0")
    with pytest.raises(ValueError, match="MLS_SERVE_DEVICE_PICK"):
        ContinuousLlama(model, speculate=K, spec_device=True)


def test_generate_refusals(model):
    ids, lens = _prompts()
    gp = GenParams(max_new_tokens=4)
    with pytest.raises(ValueError, match="speculate >= 1"):
        model.generate(ids, lens, gp, spec_device=True)
    with pytest.raises(ValueError, match="drafter"):
        model.generate(ids, lens, gp, speculate=K, spec_device=True, drafter=SP.prompt_lookup_draft)
    with pytest.raises(ValueError, match="device-resident"):
        model.generate(ids, lens, gp, speculate=K, spec_device=True)
    with pytest.raises(ValueError, match="device-resident"):
        model.check_spec_device(K)
    assert not model._spec_device_ok(4, K + 1, 8)


def test_without_the_option_nothing_changes(model):
    """``speculate`` alone: the host path (``dev_mode`` stays False), the default drafter, the same tokens
    as plain decoding; ``generate`` likewise."""
    ids, lens = _prompts()
    gp = GenParams(max_new_tokens=6)
    eng = ContinuousLlama(model, speculate=K)
    assert eng.spec_device is False
    fut = eng.submit(ids[0].tolist(), gp)
    for _ in range(20):
        if fut.done():
            break
        eng.run_iteration(eng._leader_admissions())
    assert not eng.dev_mode and eng.failures == 0
    plain = model.generate(ids[:1], lens[:1], gp)
    assert fut.result(timeout=0) == plain[0].tolist()
    assert torch.equal(model.generate(ids[:1], lens[:1], gp, speculate=K), plain)


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
        cfg = tiny_config(**CFG128)
        m = LlamaTP(init_llama_shard(cfg, world, rank, seed=5), cfg, tp=world, rank=rank, comm=TPComm(None, world),
                    max_batch=4, max_seq=128)
        msgs = []
        for kw in (dict(speculate=K), dict(speculate=K, spec_device=True)):
            try:
                ContinuousLlama(m, **kw)
                msgs.append("")
            except ValueError as e:
                msgs.append(str(e))
        q.put((rank, msgs))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_tp2_without_the_option_is_still_refused():
    """A TP = 2 model over gloo: ``speculate`` alone is refused with the message it always had; with
    ``spec_device`` the constructor no longer stops at ``tp > 1`` (here it stops at the missing device loop)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=100) for _ in range(2))
    for pr in procs:
        pr.join(30)
        assert pr.exitcode == 0
    for _rank, (host, dev) in res:
        assert "speculate is not available with tp > 1 in the continuous engine" in host
        assert "tp > 1" not in dev and "device-resident" in dev


def test_model_config(tmp_path):
    from mlmicroservicetemplate_amd.config import Settings
    from mlmicroservicetemplate_amd.plugins.base import PluginContext
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    assert LlamaPlugin.parse_speculate_device({}, 0) is False
    assert LlamaPlugin.parse_speculate_device({"speculate_device": False}, 3) is False
    assert LlamaPlugin.parse_speculate_device({"speculate_device": True}, 3) is True
    for bad in (1, "yes", 0, None):
        with pytest.raises(ValueError, match="speculate_device"):
            LlamaPlugin.parse_speculate_device({"speculate_device": bad}, 3)
    with pytest.raises(ValueError, match="speculate >= 1"):
        LlamaPlugin.parse_speculate_device({"speculate_device": True}, 0)

    def plugin(text, **over):
        y = tmp_path / "llama.yaml"
        y.write_text(text)
        s = Settings.load(env_file=None, environ={}, overrides=dict({"REGISTER": False, "MODEL": "llama",
                                                                      "MODEL_CONFIG": str(y), "MAX_BATCH": 2,
                                                                      "GPUS": 0}, **over))
        pl = LlamaPlugin()
        pl.init(PluginContext(settings=s))
        return pl

    base = "config: tiny\nmax_seq: 64\noverrides:\n  layers: 1\n"
    with pytest.raises(ValueError, match="speculate_device"):
        plugin(base + "speculate: 2\nspeculate_device: 1\n")
    with pytest.raises(ValueError, match="speculate >= 1"):
        plugin(base + "speculate_device: true\n")
    for cb in (True, False):  # the CPU has no device loop: refused at start-up on both serving paths
        with pytest.raises(ValueError, match="device-resident"):
            plugin(base + "speculate: 2\nspeculate_device: true\n", CONTINUOUS_BATCHING=cb)
    pl = plugin(base + "speculate: 2\nspeculate_ngram: 2\nspeculate_device: false\n")
    try:
        d = pl.describe()
        assert d["speculate"] == 2 and d["speculate_ngram"] == 2 and d["speculate_device"] is False
        assert pl.engine.spec_device is False and pl.engine.drafter is not None
        assert pl._spec_device_kw() == {}
    finally:
        pl.close()
    pl = plugin(base)
    try:
        assert pl.describe()["speculate_device"] is False
        # what the engine and generate() get when the option is on: the n-gram bound feeds the kernel
        pl.speculate, pl.speculate_ngram, pl.speculate_device = 3, 5, True
        assert pl._spec_device_kw() == dict(spec_device=True, spec_ngram=(5, 1)) and pl._drafter() is None
        assert pl.describe()["speculate_device"] is True
    finally:
        pl.close()
