"""``w4_rows="all"`` on CPU: the route rules of the new tier, the refusals, the reference backend (which ignores
it) and the plugin's ``w4_rows`` key."""
import pytest
import torch

from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
from mlmicroservicetemplate_amd.models.llama_route import ProjTiers, proj_tiers, step_route
from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin
from test_kv_fp8_cpu import CFG128

STEP = dict(S=1, decode=True, has_past=True, all_rows=False, tp=1, hq=8, hkv=2, head_dim=128, hidden=1024,
            have_packed=False, have_w4=True, have_fp8=False, o_packed=False, o_fp8=False, w4_max_rows=32, pk_fold=True,
            prefill_fold=False, fuse_combine=True, fuse_add_norm=True, ar_fuse=True, tp_overlap=True,
            verify_attn="multi", spec_max_tokens=8, dec_chunk=0, ar_fusable=False, capturing=False)
CFG_P = (tiny_config(**CFG128), init_llama_shard(tiny_config(**CFG128), 1, 0, seed=5))


@pytest.mark.parametrize("rows", [1, 16, 24, 32, 33, 64, 257, 4096])
def test_route_rules(rows):
    tr = proj_tiers(rows, False, True, False, 32, w4_all=True)
    assert tr.w4 == (rows <= 32) and tr.w4g == (rows > 32)  # skinny up to the kernel's limit, tiled above
    rt = step_route(B=rows, w4_all=True, **STEP)
    assert rt.fold and not rt.fuse_rn and not rt.ar_fuse and not rt.fuse_combine  # fold as for w4, fuse_rn off
    assert not step_route(B=rows, w4_all=True, **dict(STEP, tp=2)).fold
    assert not step_route(B=rows, w4_all=True, **dict(STEP, pk_fold=False)).fuse_rn  # ... at every row count, as w8
    assert not step_route(B=rows, w4_all=True, **dict(STEP, tp=2, decode=False, has_past=False, S=4)).overlap
    assert not proj_tiers(rows, True, False, False, 0, w4_all=True).w4g  # no int4 codes: the switch routes nothing
    old = proj_tiers(rows, True, True, False, 32)
    assert old == ProjTiers(rows=rows, w4=rows <= 32, fp8=False, packed=rows <= 24, fuse=rows <= 16) and not old.w4g
    rt = step_route(B=rows, **STEP)
    assert not rt.proj.w4g and rt.fold == (rows <= 32) and rt.fuse_rn == (rows > 32)


def test_refusals_and_plugin_key():
    cfg, p = CFG_P
    for kw in (dict(w4_rows="all"), dict(weight_dtype="w8a8", w4_rows="all"), dict(weight_dtype="int4", w4_rows="prefill")):
        with pytest.raises(ValueError, match="w4_rows"):
            LlamaTP(p, cfg, max_batch=2, max_seq=64, **kw)
    assert LlamaPlugin.parse_w4_rows({}, "bf16") == LlamaPlugin.parse_w4_rows({}, "int4") == "decode"
    assert LlamaPlugin.parse_w4_rows({"w4_rows": "all"}, "int4") == "all"
    for extra, wd in (({"w4_rows": "all"}, "bf16"), ({"w4_rows": "all"}, "w8a8"), ({"w4_rows": "prefill"}, "int4")):
        with pytest.raises(ValueError, match="w4_rows"):
            LlamaPlugin.parse_w4_rows(extra, wd)


def test_reference_backend_ignores_it():
    cfg, p = CFG_P
    ids = torch.randint(3, 2000, (2, 20), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    lens = torch.tensor([20, 13], dtype=torch.int32)
    plain = LlamaTP(p, cfg, max_batch=2, max_seq=64, weight_dtype="int4")
    every = LlamaTP(p, cfg, max_batch=2, max_seq=64, weight_dtype="int4", w4_rows="all")
    assert every.w4_rows == "all" and plain.w4_rows == "decode" and not every.w4
    assert all(torch.equal(every.p[n], w) for n, w in plain.p.items())
    assert every.layer_weight_bytes() == plain.layer_weight_bytes()
    gp = GenParams(max_new_tokens=4)
    assert torch.equal(every.generate(ids, lens, gp), plain.generate(ids, lens, gp))
