"""int4 (W4A16) weights on CPU: the quantisation rule in ops.reference, the granule packing, the
reference backend as the oracle of the fused path, TP sharding and the plugin's ``weight_dtype`` key."""
import multiprocessing as mp
import os
import socket

import pytest
import torch

from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
from mlmicroservicetemplate_amd.ops import reference as R
from test_kv_fp8_cpu import CFG, CFG128, decode_top5_deviation

# Relative max deviation of the decode step's top-5 logit values, reference backend with int4 layer
# projections vs the bf16 model (CFG128, seed 5, two 20-token prompts).  Measured on the CPU: 0.049853.
D_W4 = 0.0499


def w4_test_rows(n: int = 64, k: int = 1024, seed: int = 0) -> torch.Tensor:
    """bf16-valued rows with per-group magnitudes over three decades, an all-zero group and one 1e4 outlier."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.logspace(-2, 1, n * (k // 128)).view(n, k // 128, 1)
    w = (torch.randn(n, k // 128, 128, generator=g) * mag).reshape(n, k)
    w[3, k - 128:] = 0.0
    w[5, k - 60] = 1e4
    return w.to(torch.bfloat16).float()


def test_roundtrip_bound_and_scales():
    w = w4_test_rows()
    q, scale = R.w4_quant(w)
    assert q.dtype == torch.int8 and q.shape == w.shape
    assert scale.dtype == torch.bfloat16 and scale.shape == (64, 8)
    assert int(q.min()) >= -8 and int(q.max()) <= 7
    dq = R.w4_dequant(q, scale)
    assert dq.dtype == torch.float32
    step = scale.float().repeat_interleave(128, dim=1)
    err = (dq - w).abs()
    print("worst |dq - w| / scale:", (err / step).max().item())
    assert (err <= 0.5 * step * (1 + 1e-3)).all()
    amax = w.view(64, 8, 128).abs().amax(-1)
    want = torch.clamp((amax / torch.full_like(amax, 7.0)).to(torch.bfloat16).float(), min=2.0 ** -40)
    assert torch.equal(scale.float(), want)
    assert not q[3, 896:].any() and (dq[3, 896:] == 0).all()
    assert scale[3, 7].float().item() == 2.0 ** -40
    assert q[5, 964].item() == 7  # the outlier sets its group's scale
    with pytest.raises(ValueError):
        R.w4_quant(torch.zeros(16, 192))


@pytest.mark.parametrize("N,K", [(16, 128), (48, 384), (32, 1024)])
def test_pack_unpack_is_bit_exact(N, K):
    from mlmicroservicetemplate_amd import ops

    w = w4_test_rows(N, K, seed=N + K)
    wq, scales = ops.pack_skinny_w4(w.to(torch.bfloat16))
    assert wq.dtype == torch.uint8 and wq.shape == (N * K // 2,)
    assert scales.dtype == torch.bfloat16 and scales.shape == (N * K // 128,)
    q, scale = ops.unpack_skinny_w4_reference(wq, scales, N, K)
    want_q, want_s = R.w4_quant(w)
    assert torch.equal(q, want_q) and torch.equal(scale, want_s)
    # the documented nibble order: word 0 of granule 0 = row 0, k 0..7; weight e at bits 4 (e // 2) + 16 (e % 2)
    word = int.from_bytes(bytes(wq[:4].tolist()), "little")
    for e in range(8):
        assert (word >> (4 * (e // 2) + 16 * (e % 2))) & 15 == int(want_q[0, e]) + 8
    # lane (g, nr)'s 16 bytes follow at (g * 16 + nr) * 16: its word `ks` starts at k = 32 ks + 8 g
    g, nr, ks = 2, 5, 3
    off = (g * 16 + nr) * 16 + ks * 4
    assert (int(wq[off]) & 15) == int(want_q[nr, 32 * ks + 8 * g]) + 8
    x = torch.randn(3, K)
    assert torch.equal(ops.w4_reference(x, w), x @ R.w4_dequant(want_q, want_s).T)
    with pytest.raises(ValueError):
        ops.pack_skinny_w4(torch.zeros(24, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.pack_skinny_w4(torch.zeros(16, 192, dtype=torch.bfloat16))


def _fold(w, gain):
    return (w.float() * gain.float().view(1, -1)).to(w.dtype)


def test_reference_model_weights_are_the_fold_quantise_dequantise():
    cfg = tiny_config(**CFG)
    p = init_llama_shard(cfg, 1, 0, seed=4)
    m = LlamaTP(p, cfg, max_batch=2, max_seq=64, weight_dtype="int4")
    assert m.weight_dtype == "int4" and not m.w4
    for i in range(cfg.layers):
        for n, gain in (("qkv", "attn_norm"), ("gate", "mlp_norm"), ("up", "mlp_norm"), ("o", None), ("down", None)):
            w = p[f"l{i}.{n}"] if gain is None else _fold(p[f"l{i}.{n}"], p[f"l{i}.{gain}"])
            assert torch.equal(m.p[f"l{i}.{n}"], R.w4_dequant(*R.w4_quant(w))), (i, n)
        for gain in ("attn_norm", "mlp_norm"):
            assert (m.p[f"l{i}.{gain}"] == 1).all()
        # quantising gate and up separately == quantising the fused backend's interleaved matrix
        from mlmicroservicetemplate_amd.ops import interleave_gate_up

        gu = interleave_gate_up(_fold(p[f"l{i}.gate"], p[f"l{i}.mlp_norm"]), _fold(p[f"l{i}.up"], p[f"l{i}.mlp_norm"]))
        assert torch.equal(R.w4_dequant(*R.w4_quant(gu)), interleave_gate_up(m.p[f"l{i}.gate"], m.p[f"l{i}.up"]))
    for n in ("embed", "lm_head", "final_norm"):
        assert torch.equal(m.p[n], p[n])  # not quantised
    assert any((p[f"l0.{n}"].float() != m.p[f"l0.{n}"]).any() for n in ("o", "down"))


def test_weight_dtype_is_validated_and_default_is_unchanged():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG)
    p = init_llama_shard(cfg, 1, 0, seed=4)
    with pytest.raises(ValueError):
        LlamaTP(p, cfg, max_batch=2, max_seq=64, weight_dtype="int8")
    with pytest.raises(ValueError):
        LlamaTP(p, cfg, max_batch=2, max_seq=64, weight_dtype="fp8")
    plain = LlamaTP(p, cfg, max_batch=2, max_seq=64)
    named = LlamaTP(p, cfg, max_batch=2, max_seq=64, weight_dtype="bf16")
    assert plain.weight_dtype == named.weight_dtype == "bf16" and not named.w4
    assert plain.p.keys() == named.p.keys() == p.keys()
    for k in p:
        assert torch.equal(plain.p[k], p[k]) and torch.equal(named.p[k], p[k]) and named.p[k].dtype == p[k].dtype
    ids = torch.randint(3, 2000, (2, 12), generator=torch.Generator().manual_seed(1))
    lens = torch.tensor([12, 7])
    gp = GenParams(max_new_tokens=5)
    assert torch.equal(plain.generate(ids, lens, gp), named.generate(ids, lens, gp))
    assert plain.layer_weight_bytes() == sum(v.numel() * 2 for k, v in p.items()
                                             if k.split(".")[-1] in ("qkv", "o", "gate", "up", "down"))


def test_tp_shards_hold_slices_of_the_tp1_weights_and_tp4_is_refused():
    """Row-parallel K slices are multiples of 128, so a rank's quantised shard is the slice of the
    quantised whole; hidden 256 over 4 ranks would cut the o-projection's K to 64."""
    from mlmicroservicetemplate_amd.models.llama import ShardEmulationComm

    cfg = tiny_config(**CFG)
    full = LlamaTP(init_llama_shard(cfg, 1, 0, seed=1), cfg, max_batch=4, max_seq=64, weight_dtype="int4")
    D = cfg.head_dim
    for rank in range(2):
        m = LlamaTP(init_llama_shard(cfg, 2, rank, seed=1), cfg, tp=2, rank=rank, comm=ShardEmulationComm(2),
                    max_batch=4, max_seq=64, weight_dtype="int4")
        hq, inter = m.sd.hq, m.sd.inter
        for i in range(cfg.layers):
            assert torch.equal(m.p[f"l{i}.o"], full.p[f"l{i}.o"][:, rank * hq * D:(rank + 1) * hq * D])
            assert torch.equal(m.p[f"l{i}.down"], full.p[f"l{i}.down"][:, rank * inter:(rank + 1) * inter])
            assert torch.equal(m.p[f"l{i}.gate"], full.p[f"l{i}.gate"][rank * inter:(rank + 1) * inter])
            assert torch.equal(m.p[f"l{i}.qkv"][: hq * D], full.p[f"l{i}.qkv"][rank * hq * D:(rank + 1) * hq * D])
    ids = torch.randint(3, 2000, (3, 12), generator=torch.Generator().manual_seed(7))
    out = m.generate(ids, torch.tensor([12, 7, 3]), GenParams(max_new_tokens=4))  # one shard runs end to end
    assert out.shape == (3, 4)
    with pytest.raises(ValueError, match="128"):
        LlamaTP(init_llama_shard(cfg, 4, 0, seed=1), cfg, tp=4, rank=0, comm=ShardEmulationComm(4), max_batch=4,
                max_seq=64, weight_dtype="int4")


def _tp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from mlmicroservicetemplate_amd.models.llama import TPComm

    torch.set_num_threads(1)  # fixed summation order
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = tiny_config(**CFG)
        m = LlamaTP(init_llama_shard(cfg, world, rank, seed=1), cfg, tp=world, rank=rank, comm=TPComm(None, world),
                    max_batch=4, max_seq=64, weight_dtype="int4")
        ids = torch.randint(3, 2000, (3, 12), generator=torch.Generator().manual_seed(7))
        q.put((rank, m.generate(ids, torch.tensor([12, 7, 3]), GenParams(max_new_tokens=6)).tolist()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_tp2_generates_the_tokens_of_tp1():
    """Two ranks with summed partial products (ShardEmulationComm drops the sum, so its tokens are
    not the model's: the ranks run as processes, as tests/test_llama_cpu.py's TP test)."""
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG)
    ids = torch.randint(3, 2000, (3, 12), generator=torch.Generator().manual_seed(7))
    want = LlamaTP(init_llama_shard(cfg, 1, 0, seed=1), cfg, max_batch=4, max_seq=64,
                   weight_dtype="int4").generate(ids, torch.tensor([12, 7, 3]), GenParams(max_new_tokens=6))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=200) for _ in range(2)]
    for pr in procs:
        pr.join(30)
        assert pr.exitcode == 0
    for _rank, got in res:
        assert got == want.tolist()


def test_quantisation_deviation_of_the_oracle():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG128)
    p = init_llama_shard(cfg, 1, 0, seed=5)
    ids = torch.randint(3, 2000, (2, 20), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    lens = torch.tensor([20, 20], dtype=torch.int32)
    q4 = LlamaTP(p, cfg, max_batch=2, max_seq=64, weight_dtype="int4")
    full = LlamaTP(p, cfg, max_batch=2, max_seq=64)
    dev = decode_top5_deviation(q4, full, ids, lens)
    print("int4 vs bf16 weights, top-5 logit deviation:", dev)
    assert 0 < dev <= 1.05 * D_W4


def test_plugin_weight_dtype(tmp_path):
    import time

    from fastapi.testclient import TestClient

    from mlmicroservicetemplate_amd.api.app import create_app
    from mlmicroservicetemplate_amd.config import Settings
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    assert LlamaPlugin.parse_weight_dtype({}) == "bf16"
    assert LlamaPlugin.parse_weight_dtype({"weight_dtype": "int4"}) == "int4"
    with pytest.raises(ValueError):
        LlamaPlugin.parse_weight_dtype({"weight_dtype": "int8"})

    y = tmp_path / "llama.yaml"
    y.write_text("config: tiny\nmax_seq: 128\nweight_dtype: int4\noverrides:\n  layers: 2\n")
    s = Settings.load(env_file=None, environ={}, overrides={"REGISTER": False, "MODEL": "llama", "MODEL_CONFIG": str(y),
                                                          "MAX_BATCH": 8, "GPUS": 0})
    cfg = tiny_config(layers=2)
    m = LlamaTP(init_llama_shard(cfg, 1, 0, seed=0), cfg, max_batch=8, max_seq=128, weight_dtype="int4")
    ids = [1, 55, 99, 1000]
    want = m.generate(torch.tensor([ids]), torch.tensor([len(ids)]), GenParams(5))[0].tolist()
    with TestClient(create_app(s), raise_server_exceptions=False) as c:
        t0 = time.time()
        while c.get("/status").status_code != 200 and time.time() - t0 < 60:
            time.sleep(0.05)
        assert c.app.state.runtime.plugin.model.weight_dtype == "int4"
        r = c.post("/generate", json={"input_ids": ids, "max_new_tokens": 5})
        assert r.status_code == 200, r.text
        res = r.json()["result"]
        assert res["num_tokens"] >= 1 and res["token_ids"] == want[: res["num_tokens"]]


def test_plugin_rejects_a_bad_weight_dtype_before_building(tmp_path, monkeypatch):
    from mlmicroservicetemplate_amd.config import Settings
    from mlmicroservicetemplate_amd.models import llama
    from mlmicroservicetemplate_amd.plugins.base import PluginContext
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    def no_alloc(*a, **k):
        raise AssertionError("weights were initialised before weight_dtype was validated")

    monkeypatch.setattr(llama, "init_llama_shard", no_alloc)
    y = tmp_path / "llama.yaml"
    y.write_text("config: tiny\nweight_dtype: int3\n")
    s = Settings.load(env_file=None, environ={}, overrides={"REGISTER": False, "MODEL": "llama", "MODEL_CONFIG": str(y),
                                                          "MAX_BATCH": 8, "GPUS": 0})
    with pytest.raises(ValueError, match="weight_dtype"):
        LlamaPlugin().init(PluginContext(settings=s))
