"""Prompt scoring on the CPU: the oracle pair ``ops.reference.linear_logprob`` / ``logprob_merge``, the reference
backend's ``LlamaTP.score`` and the ``"score": true`` request of ``/generate``."""
import time

import pytest
import torch

from mlmicroservicetemplate_amd.ops import reference as R

VOCAB, K, M = 100, 32, 9


@pytest.mark.parametrize("shards", [(100,), (64, 36), (40, 40, 20)])
def test_sharded_oracle_equals_log_softmax(shards):
    """Uneven shards, each zero-padded by 4 rows past its ``valid``: folded, they are the full log-softmax."""
    g = torch.Generator().manual_seed(len(shards))
    x = torch.randn(M, K, generator=g, dtype=torch.float64) * 2
    w = torch.randn(VOCAB, K, generator=g, dtype=torch.float64)
    targets = torch.randint(0, VOCAB, (M,), generator=g, dtype=torch.int32)
    targets[3] = -1
    parts, lo = [], 0
    for n in shards:
        padded = torch.cat([w[lo: lo + n], torch.zeros(4, K, dtype=torch.float64)])
        parts.append(R.linear_logprob(x, padded, targets, lo, n))
        lo += n
    got = R.logprob_merge(torch.stack(parts))
    want = torch.log_softmax(x @ w.T, dim=1).gather(1, targets.clamp(min=0).long().unsqueeze(1)).squeeze(1)
    keep = targets >= 0
    assert torch.allclose(got[keep], want[keep], rtol=0, atol=1e-12)
    assert got[3] == float("-inf")
    # a shard that is all padding adds nothing
    empty = R.linear_logprob(x, torch.zeros(8, K, dtype=torch.float64), targets, VOCAB, 0)
    assert torch.equal(R.logprob_merge(torch.stack(parts + [empty])), got)


def _tiny(**kw):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP, init_llama_shard, tiny_config

    cfg = tiny_config(layers=2)
    return LlamaTP(init_llama_shard(cfg, 1, 0, seed=0), cfg, max_batch=4, max_seq=32, **kw), cfg


def test_reference_score_is_the_gather_of_its_logits():
    m, cfg = _tiny()
    g = torch.Generator().manual_seed(1)
    B, S = 3, 12
    ids = torch.randint(3, cfg.vocab, (B, S), generator=g, dtype=torch.int32)
    lens = torch.tensor([12, 7, 1], dtype=torch.int32)
    got = m.score(ids, lens)
    assert got.shape == (B, S) and got.dtype == torch.float32
    # the model's own full logits of every row: a chunk at past 0 with every row kept
    m.keep_logits = True
    pos = torch.arange(S, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
    m.step(ids, pos, lens, decode=False, k=1, past=torch.zeros(B, dtype=torch.int32), all_rows=True)
    lsm = torch.log_softmax(m.last_logits.double()[:, : cfg.vocab], dim=1).view(B, S, -1)
    for b in range(B):
        n = int(lens[b])
        want = lsm[b, : n - 1].gather(1, ids[b, 1:n].long().unsqueeze(1)).squeeze(1)
        assert torch.allclose(got[b, 1:n].double(), want, rtol=0, atol=1e-4)
        assert got[b, 0] == 0 and (got[b, n:] == 0).all()
    with pytest.raises(ValueError):
        m.score(torch.zeros(1, 33, dtype=torch.int32), torch.tensor([33]))


@pytest.mark.parametrize("continuous", [False, True])
def test_score_request(tmp_path, continuous):
    from fastapi.testclient import TestClient

    from mlmicroservicetemplate_amd.api.app import create_app
    from mlmicroservicetemplate_amd.config import Settings

    y = tmp_path / "llama.yaml"
    y.write_text("config: tiny\nmax_seq: 32\noverrides:\n  layers: 2\n")
    s = Settings.load(env_file=None, environ={}, overrides={
        "REGISTER": False, "MODEL": "llama", "MODEL_CONFIG": str(y), "MAX_BATCH": 4, "GPUS": 0,
        "CONTINUOUS_BATCHING": continuous})
    ids = [1, 55, 99, 1000, 7]
    with TestClient(create_app(s), raise_server_exceptions=False) as c:
        t0 = time.time()
        while c.get("/status").status_code != 200 and time.time() - t0 < 60:
            time.sleep(0.05)
        r = c.post("/generate", json={"input_ids": ids, "score": True, "max_new_tokens": 0})
        if continuous:
            assert r.status_code == 400 and "CONTINUOUS_BATCHING" in r.json()["detail"]
            return
        assert r.status_code == 200, r.text
        res = r.json()["result"]
        want = _tiny()[0].score(torch.tensor([ids]), torch.tensor([len(ids)]))[0]
        assert res["input_ids"] == ids and res["tokens"] == 4
        assert torch.allclose(torch.tensor(res["logprobs"], dtype=torch.float64), want.double(), rtol=0, atol=1e-5)
        assert res["nll"] == pytest.approx(-float(want.sum()), abs=1e-4)
        assert c.post("/generate", json={"input_ids": ids, "score": "yes"}).status_code == 400
