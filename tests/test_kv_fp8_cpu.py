"""FP8 (e4m3) KV cache on CPU: the quantisation rule in ops.reference, the reference backend as the
oracle of the fused path (per-slot and paged), page accounting and the plugin's ``kv_dtype`` key."""
import time

import pytest
import torch

from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
from mlmicroservicetemplate_amd.ops import reference as R

CFG = dict(vocab=2048, hidden=256, layers=2, heads=8, kv_heads=4, head_dim=32, intermediate=512)  # test_kv_pages.py
CFG128 = dict(layers=2, hidden=512, heads=8, kv_heads=2, head_dim=128, intermediate=1024)  # the fused path's head size

# Relative max deviation of the decode step's top-5 logit values, reference backend with the fp8
# cache vs with the fp32 cache (CFG128, seed 5, two 20-token prompts).  Measured on the CPU: 0.011078.
D_REF = 0.0111


def kv_fp8_test_rows(n: int = 4096, d: int = 128, seed: int = 0) -> torch.Tensor:
    """bf16-valued rows with per-row magnitudes over ~3 decades, an all-zero row and a row with one
    1e4 outlier."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g) * torch.logspace(-2, 1, n).unsqueeze(1)
    x[7] = 0.0
    x[11, 5] = 1e4
    return x.to(torch.bfloat16).float()


def roundtrip_bound(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """|x|/16 is e4m3's half-ulp for normals, scale * 2^-10 half its subnormal step."""
    return 1.01 * (x.abs() / 16 + scale.unsqueeze(-1) * 2.0 ** -10)


def test_roundtrip_bound_and_scales():
    x = kv_fp8_test_rows()
    q, scale = R.kv_quant_fp8(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    deq = R.kv_dequant_fp8(q, scale)
    err = (deq - x).abs()
    bound = roundtrip_bound(x, scale)
    print("worst ratio", (err / bound.clamp_min(1e-30)).max().item() * 1.01)
    assert (err <= bound).all()
    assert torch.isfinite(scale).all() and torch.isfinite(deq).all()
    want = torch.clamp(x.abs().amax(-1), min=2.0 ** -40) / 448
    assert torch.allclose(scale, want, rtol=1e-6, atol=0)
    assert not q[7].any() and (deq[7] == 0).all()
    assert deq[11, 5] == 1e4 or abs(deq[11, 5].item() - x[11, 5].item()) <= x[11, 5].item() / 16


def _prefill(model, ids, lens):
    B, S = ids.shape
    pos = torch.arange(S, dtype=torch.int32, device=ids.device).unsqueeze(0).expand(B, S).contiguous()
    return model.step(ids, pos, lens, decode=False, k=5)


def test_reference_model_cache_is_the_roundtrip():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG)
    p = init_llama_shard(cfg, 1, 0, seed=4)
    ids = torch.randint(3, 2000, (2, 20), generator=torch.Generator().manual_seed(1)).to(torch.int32)
    lens = torch.tensor([20, 9], dtype=torch.int32)
    ref = LlamaTP(p, cfg, max_batch=2, max_seq=64)
    q8 = LlamaTP(p, cfg, max_batch=2, max_seq=64, kv_dtype="fp8")
    assert ref.kv_dtype == "bf16" and q8.kv_dtype == "fp8"
    _prefill(ref, ids, lens)
    _prefill(q8, ids, lens)
    # layer 0 sees identical inputs in both runs (prefill attention is unquantised, so later layers do too)
    for i in range(cfg.layers):
        for full, quant in ((ref.k_cache[i], q8.k_cache[i]), (ref.v_cache[i], q8.v_cache[i])):
            for b, n in enumerate(lens.tolist()):
                assert torch.equal(quant[b, :n], R.kv_dequant_fp8(*R.kv_quant_fp8(full[b, :n])))
                assert full[b, :n].abs().sum() > 0
                assert not quant[b, n:].any()
    with pytest.raises(ValueError):
        LlamaTP(p, cfg, max_batch=2, max_seq=64, kv_dtype="int4")


def test_reference_model_paged_matches_per_slot():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG)
    p = init_llama_shard(cfg, 1, 0, seed=4)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 2000, (3, 70), generator=g)
    lens = torch.tensor([70, 41, 5])
    for gp in (GenParams(max_new_tokens=9), GenParams(9, top_k=8, temperature=0.7, seed=2)):
        want = LlamaTP(p, cfg, max_batch=3, max_seq=192, kv_dtype="fp8").generate(ids, lens, gp)
        paged = LlamaTP(p, cfg, max_batch=3, max_seq=192, kv_pages=7, kv_dtype="fp8")
        got = paged.generate(ids, lens, gp)
        assert torch.equal(got, want)
        assert paged.pages.free_pages == 6


def decode_top5_deviation(model_a, model_b, ids, lens):
    """Prefill both, one decode step of the same token; relative max deviation of a's top-5 logit
    values from b's (the measure of tests/test_models_gpu.py's fused-vs-reference comparison)."""
    B = ids.shape[0]
    for m in (model_a, model_b):
        _prefill(m, ids, lens)
    tok = torch.full((B, 1), 7, dtype=torch.int32, device=ids.device)
    cur = lens.view(B, 1).clone()
    vb, _ = model_b.step(tok, cur, lens + 1, decode=True, k=5)
    va, _ = model_a.step(tok, cur, lens + 1, decode=True, k=5)
    return ((va.float() - vb.float()).abs().max() / (vb.float().abs().max() + 1e-6)).item()


def test_quantisation_deviation_of_the_oracle():
    torch.set_num_threads(1)
    cfg = tiny_config(**CFG128)
    p = init_llama_shard(cfg, 1, 0, seed=5)
    ids = torch.randint(3, 2000, (2, 20), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    lens = torch.tensor([20, 20], dtype=torch.int32)
    q8 = LlamaTP(p, cfg, max_batch=2, max_seq=64, kv_dtype="fp8")
    full = LlamaTP(p, cfg, max_batch=2, max_seq=64)
    dev = decode_top5_deviation(q8, full, ids, lens)
    print("fp8 vs fp32 cache, top-5 logit deviation:", dev)
    assert 0 < dev <= 1.5 * D_REF


def test_page_accounting():
    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    cfg = LLAMA3_8B
    assert cfg.head_dim == 128
    for tp in (1, 8):
        hkv = cfg.kv_heads // tp
        base = cfg.layers * 2 * 64 * hkv
        assert LlamaPlugin.kv_page_bytes(cfg, tp, "fused", "fp8") == base * (128 + 4)
        assert LlamaPlugin.kv_page_bytes(cfg, tp, "fused", "bf16") == base * 128 * 2
        assert LlamaPlugin.kv_page_bytes(cfg, tp, "fused") == base * 128 * 2
        assert LlamaPlugin.kv_page_bytes(cfg, tp, "reference", "bf16") == base * 128 * 4
        assert LlamaPlugin.kv_page_bytes(cfg, tp, "reference", "fp8") == base * 128 * 4  # fp32 round-tripped rows
    free = 200 << 30
    full = 10 ** 9  # the full-coverage cap does not bind
    n16 = LlamaPlugin.kv_pages_for(free, LlamaPlugin.kv_page_bytes(cfg, 1, "fused", "bf16"), full)
    n8 = LlamaPlugin.kv_pages_for(free, LlamaPlugin.kv_page_bytes(cfg, 1, "fused", "fp8"), full)
    assert n16 == (free // 2) // (32 * 2 * 64 * 8 * 256)
    assert n8 >= 1.9 * n16
    assert LlamaPlugin.kv_pages_for(free, LlamaPlugin.kv_page_bytes(cfg, 1, "fused", "fp8"), 100) == 100
    # the existing entry point takes the dtype too (CPU: the full-coverage cap)
    assert LlamaPlugin._kv_pages("auto", tiny_config(**CFG), 1, 2, 128, "cpu", "reference", "fp8") == 2 * 2 + 1


def test_plugin_kv_dtype(tmp_path):
    from fastapi.testclient import TestClient

    from mlmicroservicetemplate_amd.api.app import create_app
    from mlmicroservicetemplate_amd.config import Settings

    y = tmp_path / "llama.yaml"
    y.write_text("config: tiny\nmax_seq: 128\nkv_dtype: fp8\noverrides:\n  layers: 2\n")
    s = Settings.load(env_file=None, environ={}, overrides={"REGISTER": False, "MODEL": "llama", "MODEL_CONFIG": str(y),
                                                          "MAX_BATCH": 8, "GPUS": 0})
    cfg = tiny_config(layers=2)
    m = LlamaTP(init_llama_shard(cfg, 1, 0, seed=0), cfg, max_batch=8, max_seq=128, kv_dtype="fp8")
    ids = [1, 55, 99, 1000]
    want = m.generate(torch.tensor([ids]), torch.tensor([len(ids)]), GenParams(5))[0].tolist()
    with TestClient(create_app(s), raise_server_exceptions=False) as c:
        t0 = time.time()
        while c.get("/status").status_code != 200 and time.time() - t0 < 60:
            time.sleep(0.05)
        assert c.app.state.runtime.plugin.model.kv_dtype == "fp8"
        r = c.post("/generate", json={"input_ids": ids, "max_new_tokens": 5})
        assert r.status_code == 200, r.text
        res = r.json()["result"]
        assert res["num_tokens"] >= 1 and res["token_ids"] == want[: res["num_tokens"]]
