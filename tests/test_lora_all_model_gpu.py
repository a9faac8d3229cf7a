"""LoRA on all seven projections through the fused Llama (``lora={"targets": "all"}``, csrc/lora_linear.hip in
the layer tail) against the reference backend: every emitted token under test_lora_model_gpu.py's rule
(``_check_tokens``, imported), bf16 and int4 weights, decode batches of 3 mixed and 18 on one adapter, a 2 x 17
prefill, each captured decode step replayed on other adapters, and the routes with only q / k / v adapters."""
import pytest
import torch

from mlmicroservicetemplate_amd.models.llama import (GenParams, LlamaTP, init_llama_shard, random_lora_adapter,
                                                     tiny_config)
from mlmicroservicetemplate_amd.ops.reference import LORA_ALL_MODULES
from test_lora_model_gpu import CFG128, DEV, _check_tokens

pytestmark = pytest.mark.gpu
A, B_ = 0, 1  # rank 8 on all seven modules; rank 4 on q, o, gate, down
LORA = {"max_adapters": 3, "max_rank": 16, "targets": "all"}


@pytest.fixture(scope="module")
def tiny():
    cfg = tiny_config(**CFG128)
    ads = [random_lora_adapter(cfg, 8, seed=21, modules=LORA_ALL_MODULES, b_std=0.05),
           random_lora_adapter(cfg, 4, seed=22, modules=("q", "o", "gate", "down"), alpha=24.0, b_std=0.05)]
    return cfg, init_llama_shard(cfg, 1, 0, seed=5), ads


def _llama(tiny, backend, weight_dtype="bf16", lora=LORA, adapters=None):
    cfg, p, ads = tiny
    m = LlamaTP(p, cfg, backend=backend, device=DEV, max_batch=20, max_seq=128, weight_dtype=weight_dtype, lora=lora)
    for i, (t, c) in enumerate(ads if adapters is None else adapters):
        m.load_adapter(i, t, c)
    return m


@pytest.fixture(scope="module", params=["bf16", "int4"])
def models(tiny, request):
    return _llama(tiny, "fused", request.param), _llama(tiny, "reference", request.param)


def _generate(m, lens, adapters, new=4):
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, 2000, (len(lens), max(lens)), generator=g)
    out = m.generate(ids, torch.tensor(lens), GenParams(new, adapter=adapters)).tolist()
    return [ids[b, :n].tolist() for b, n in enumerate(lens)], out


@pytest.mark.parametrize("lens,adapters", [([9, 30, 12], [A, -1, B_]), ([5 + b for b in range(18)], [A] * 18),
                                           ([17, 17], [B_, A])], ids=["3_mixed", "18_one_adapter", "2x17_prefill"])
def test_tokens_against_the_reference_backend(models, lens, adapters):
    m, ref = models
    prompts, out = _generate(m, lens, adapters)
    worst = max(_check_tokens(ref, a, q, o) for a, q, o in zip(adapters, prompts, out))
    print(f"{m.weight_dtype} {lens[:3]}..: worst token gap {worst:.3f} of the bound")
    # the captured decode step replayed after set_slot_adapter: other adapters, no re-capture
    captured = {k: id(v) for k, v in {**m._graphs, **m._dev_graphs}.items()}
    other = adapters[1:] + adapters[:1]
    for a, q, o in zip(other, *_generate(m, lens, other)):
        _check_tokens(ref, a, q, o)
    base = _generate(m, lens, [-1] * len(lens))[1]
    assert captured and {k: id(v) for k, v in {**m._graphs, **m._dev_graphs}.items()} == captured
    assert all(o == b for a, o, b in zip(adapters, out, base) if a < 0), "a base row changed"
    assert any(o != b for a, o, b in zip(adapters, out, base) if a >= 0), "the adapters change nothing"


def test_qkv_only_adapters_keep_the_routes(tiny):
    """``targets: "all"`` with only q / k / v adapters loaded routes every step as the default model does."""
    qkv = [random_lora_adapter(tiny[0], 8, seed=21, b_std=0.05)]
    m, old = _llama(tiny, "fused", adapters=qkv), _llama(tiny, "fused", lora={"max_adapters": 3}, adapters=qkv)
    shapes = [(1, 1, True), (3, 1, True), (18, 1, True), (20, 1, True), (2, 17, False), (2, 64, False)]
    before = [m._route(B, S, dec, False, False) for B, S, dec in shapes]
    assert before == [old._route(B, S, dec, False, False) for B, S, dec in shapes]
    assert any(r.fuse_combine for r in before) and any(r.fuse_rn for r in before)
    m.load_adapter(1, *tiny[2][0])  # an o / gate / up / down adapter: the fusions a delta cannot pass are off
    assert not any(r.fuse_combine or r.fuse_rn for r in (m._route(B, S, dec, False, False) for B, S, dec in shapes))
