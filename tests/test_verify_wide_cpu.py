"""``verify_cols`` without a GPU: the route table, ``check_speculate``'s bound, the construction refusals, the
reference backend (which accepts the option and computes the same) and the plugin's parsing."""
import pytest
import torch

from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP
from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin
from test_llama_route_cpu import route
from test_speculative_cpu import MAX_SEQ, _prompts, params  # noqa: F401 (fixture)


@pytest.mark.parametrize("G,S,cols,multi,wide", [
    (4, 4, 16, True, False), (4, 5, 16, False, False), (4, 4, 64, True, False), (4, 5, 64, True, True),
    (4, 8, 64, True, True), (8, 8, 64, True, True), (8, 2, 64, True, False), (8, 3, 64, True, True),
    (2, 8, 64, True, False), (1, 8, 64, True, False)])
def test_route_table(G, S, cols, multi, wide):
    rt = route(B=2, S=S, decode=False, has_past=True, all_rows=True, hq=8, hkv=8 // G, verify_cols=cols)
    assert (rt.multi, rt.wide) == (multi, wide)


    for off in (dict(all_rows=False), dict(verify_attn="ctx"), dict(kv_fp8=True), dict(S=9)):  # never a multi step
        assert not route(**dict(dict(B=2, S=S, decode=False, has_past=True, all_rows=True, verify_cols=cols), **off)).multi


def test_check_speculate_bound_and_construction_refusals(params):  # noqa: F811
    cfg, p = params  # heads 8, kv_heads 2: G = 4
    for bad in (32, 0, "64", True):
        with pytest.raises(ValueError, match="verify_cols must be 16 or 64"):
            LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, verify_cols=bad)
    with pytest.raises(ValueError, match="bf16"):
        LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, verify_cols=64, kv_dtype="fp8", kv_prefill="cache")
    for cols in (16, 64):
        m = LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, verify_cols=cols)
        assert m.verify_cols == cols
        m.backend, m.kv_hm = "fused", True  # check_speculate's fused rule reads only these and the head counts
        m.check_speculate(3)
        for K in (5, 7):
            if cols == 64:
                m.check_speculate(K)
            else:
                with pytest.raises(ValueError, match="<= 16"):
                    m.check_speculate(K)
        with pytest.raises(ValueError, match="speculate must be in"):
            m.check_speculate(8)


def test_reference_backend_speculates_five_drafts(params):  # noqa: F811
    cfg, p = params
    ids, lens = _prompts()
    gp = GenParams(max_new_tokens=12)
    want = LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ).generate(ids, lens, gp)
    m = LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, verify_cols=64)
    assert torch.equal(m.generate(ids, lens, gp, speculate=5), want)


def test_plugin_parses_verify_cols():
    assert LlamaPlugin.parse_verify_cols({}, "bf16") == 16 and LlamaPlugin.parse_verify_cols({}, "fp8") == 16
    assert LlamaPlugin.parse_verify_cols({"verify_cols": 64}, "bf16") == 64
    for bad in (32, "wide", None, True):
        with pytest.raises(ValueError, match="verify_cols must be 16 or 64"):
            LlamaPlugin.parse_verify_cols({"verify_cols": bad}, "bf16")
    with pytest.raises(ValueError, match="bf16 only"):
        LlamaPlugin.parse_verify_cols({"verify_cols": 64}, "fp8")
