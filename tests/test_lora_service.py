"""/generate with ``"adapter"`` end to end on the CPU: MODEL_CONFIG ``lora: {name: PEFT directory}``, single
process and TP = 2 (adapters ride the admissions broadcast), same tokens as the in-process model."""
import json
import os
import signal
import socket
import subprocess
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

import pytest
import requests
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore", category=DeprecationWarning)
IDS = [1, 55, 99, 1000]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _adapters():
    from mlmicroservicetemplate_amd.models.llama import random_lora_adapter, tiny_config

    cfg = tiny_config(layers=2)
    return cfg, {"a": random_lora_adapter(cfg, 8, seed=21, b_std=0.05),
                 "b": random_lora_adapter(cfg, 4, seed=22, modules=("q", "v"), alpha=24.0, b_std=0.05)}


def _yaml(tmp_path, extra=""):
    from mlmicroservicetemplate_amd.utils.checkpoint import save_state

    _, ads = _adapters()
    lines = ["config: tiny", "max_seq: 128", "overrides:", "  layers: 2", "lora_max_rank: 8", "lora:"]
    for name, (t, c) in ads.items():
        d = tmp_path / f"adapter_{name}"
        d.mkdir()
        save_state(str(d / "adapter_model.safetensors"),
                   {f"base_model.model.model.layers.{k[1:].split('.')[0]}.self_attn.{k.split('.')[1]}_proj."
                    f"lora_{k[-1]}.weight": v for k, v in t.items()})
        (d / "adapter_config.json").write_text(json.dumps(dict(c, peft_type="LORA", bias="none")))
        lines.append(f"  {name}: {d}")
    y = tmp_path / "llama.yaml"
    y.write_text("\n".join(lines) + "\n" + extra)
    return str(y)


def _expected(n):
    from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard

    cfg, ads = _adapters()
    m = LlamaTP(init_llama_shard(cfg, 1, 0, seed=0), cfg, max_batch=8, max_seq=128,
                lora={"max_adapters": 2, "max_rank": 8})
    for i, name in enumerate(ads):
        m.load_adapter(i, *ads[name])
    out = {name: m.generate(torch.tensor([IDS]), torch.tensor([len(IDS)]), GenParams(n, adapter=a))[0].tolist()
           for name, a in ((None, -1), ("a", 0), ("b", 1))}
    assert out[None] != out["a"] != out["b"] != out[None]
    return out


def _post(c, adapter, n):
    body = {"input_ids": IDS, "max_new_tokens": n}
    if adapter is not None:
        body["adapter"] = adapter
    return c.post("/generate", json=body)


def test_generate_with_adapters_in_process(tmp_path):
    from fastapi.testclient import TestClient

    from mlmicroservicetemplate_amd.api.app import create_app
    from mlmicroservicetemplate_amd.config import Settings

    s = Settings.load(env_file=None, environ={}, overrides={"REGISTER": False, "MODEL": "llama",
                                                          "MODEL_CONFIG": _yaml(tmp_path), "MAX_BATCH": 8, "GPUS": 0})
    exp = _expected(5)
    with TestClient(create_app(s), raise_server_exceptions=False) as c:
        t0 = time.time()
        while c.get("/status").status_code != 200 and time.time() - t0 < 60:
            time.sleep(0.05)
        for name in (None, "a", "b", "a", None):
            r = _post(c, name, 5)
            assert r.status_code == 200, r.text
            res = r.json()["result"]
            assert res["token_ids"] == exp[name][: res["num_tokens"]], name
            assert set(res) == {"token_ids", "text", "num_tokens", "prompt_tokens"}  # the response format is unchanged
        empty = c.post("/generate", json={"input_ids": [], "max_new_tokens": 3}).status_code
        assert _post(c, "nobody", 3).status_code == empty == 400
        assert c.post("/generate", json={"input_ids": IDS, "adapter": 0}).status_code == 400
        assert c.get("/info").json()["model"]["adapters"] == ["a", "b"]


def test_prefix_cache_with_adapters_is_refused(tmp_path):
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    with pytest.raises(ValueError, match="prefix_cache"):
        LlamaPlugin.parse_lora({"lora": {"a": "/x"}}, prefix_cache=True)
    with pytest.raises(ValueError, match="names to directories"):
        LlamaPlugin.parse_lora({"lora": ["a"]})
    assert LlamaPlugin.parse_lora({}) == ({}, None)
    assert LlamaPlugin.parse_lora({"lora": {"a": "/x", "b": "/y"}, "lora_max_rank": 8}) == (
        {"a": "/x", "b": "/y"}, {"max_adapters": 2, "max_rank": 8})


@pytest.mark.timeout(180)
def test_generate_tp2_service_with_adapters(tmp_path):
    port = _port()
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="",
               MODEL_CONFIG=_yaml(tmp_path), LOG_LEVEL="warning")
    proc = subprocess.Popen([sys.executable, "-m", "mlmicroservicetemplate_amd", "serve", "--model", "llama", "--tp", "2",
                             "--port", str(port), "--host", "127.0.0.1", "--no-register", "--env-file", "/nonexistent"],
                            cwd=ROOT, env=env, start_new_session=True)
    try:
        url = f"http://127.0.0.1:{port}"
        deadline = time.time() + 120
        while time.time() < deadline:
            try:
                if requests.get(url + "/status", timeout=1).status_code == 200:
                    break
            except requests.RequestException:
                pass
            time.sleep(0.3)
        exp = _expected(6)

        def one(name):
            body = {"input_ids": IDS, "max_new_tokens": 6}
            if name is not None:
                body["adapter"] = name
            return name, requests.post(url + "/generate", json=body, timeout=60)

        with ThreadPoolExecutor(6) as ex:  # a, b and base in flight together: one continuous batch
            for name, r in ex.map(one, ["a", None, "b", "b", "a", None]):
                assert r.status_code == 200, r.text
                res = r.json()["result"]
                assert res["token_ids"] == exp[name][: res["num_tokens"]], name
        assert one("nobody")[1].status_code == 400
        assert requests.get(url + "/info", timeout=5).json()["model"]["tp"] == 2
    finally:
        os.killpg(proc.pid, signal.SIGTERM)
        try:
            proc.wait(30)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
