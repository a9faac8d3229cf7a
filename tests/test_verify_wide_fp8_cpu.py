"""``verify_fp8="wide"`` without a GPU: route table, refusals, ``check_speculate``'s bound, the reference backend."""
import dataclasses

import pytest
import torch

from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP
from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin
from test_llama_route_cpu import route
from test_speculative_cpu import MAX_SEQ, _prompts, params  # noqa: F401 (fixture)

FP8 = dict(kv_dtype="fp8", kv_prefill="cache")


@pytest.mark.parametrize("G,S", [(4, 4), (4, 5), (4, 8), (8, 2), (8, 3), (8, 8), (2, 8), (1, 8), (8, 9)])
@pytest.mark.parametrize("kv_fp8", [True, False])
@pytest.mark.parametrize("opt_in", [True, False])
def test_route_table(opt_in, kv_fp8, G, S):
    kw = dict(B=2, S=S, decode=False, has_past=True, all_rows=True, hq=8, hkv=8 // G, kv_fp8=kv_fp8)
    base, got = route(**kw), route(verify_fp8_wide=opt_in, **kw)
    fits = S <= 8 and S * G <= 64  # spec_max_tokens = 8
    assert got.wide == (kv_fp8 and opt_in and fits and S * G > 16)
    assert got.multi == (fits and (kv_fp8 and opt_in or not kv_fp8 and S * G <= 16))
    assert dataclasses.replace(got, multi=base.multi, wide=base.wide) == base  # no other decision reads the keyword
    if not (kv_fp8 and opt_in):
        assert got == base  # the default, and a bf16 cache: identical to today
    for off in (dict(verify_attn="ctx"), dict(all_rows=False), dict(has_past=False)):
        rt = route(verify_fp8_wide=opt_in, **dict(kw, **off))
        assert not rt.multi and not rt.wide


def test_refusals_and_check_speculate(params):  # noqa: F811
    cfg, p = params  # heads 8, kv_heads 2: G = 4
    for kv in (("bf16", "rows"), ("fp8", "rows")):
        with pytest.raises(ValueError, match="verify_fp8"):
            LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, verify_fp8="wide", kv_dtype=kv[0], kv_prefill=kv[1])
        with pytest.raises(ValueError, match="verify_fp8"):
            LlamaPlugin.parse_verify_fp8({"verify_fp8": "wide"}, *kv)
    with pytest.raises(ValueError, match="bf16"):  # verify_cols stays the bf16 cache's option
        LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, verify_fp8="wide", verify_cols=64, **FP8)
    assert LlamaPlugin.parse_verify_fp8({"verify_fp8": "wide"}, "fp8", "cache") == "wide"
    m = LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, verify_fp8="wide", **FP8)
    assert m.verify_fp8 == "wide" and m.verify_cols == 16
    m.backend, m.kv_hm, m.spec_max_tokens = "fused", True, 17  # what check_speculate's fused rule reads, + the heads
    m.check_speculate(15)  # G = 4: 64 columns
    with pytest.raises(ValueError, match="<= 64"):
        m.check_speculate(16)
    m.verify_fp8 = "multi"
    with pytest.raises(ValueError, match="<= 16"):
        m.check_speculate(5)


def test_reference_backend_speculates_five_drafts(params):  # noqa: F811
    cfg, p = params
    (ids, lens), gp = _prompts(), GenParams(max_new_tokens=12)
    want = LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, **FP8).generate(ids, lens, gp)
    m = LlamaTP(p, cfg, max_batch=4, max_seq=MAX_SEQ, verify_fp8="wide", **FP8)
    assert torch.equal(m.generate(ids, lens, gp, speculate=5), want)
