"""``verify_fp8="multi"`` without a GPU: the route rule, its default, and the constructor / MODEL_CONFIG refusals."""
import dataclasses

import pytest

from test_llama_route_cpu import TP1, route


@pytest.mark.parametrize("arm", ["multi", "ctx"])  # MLS_VERIFY_ATTN
@pytest.mark.parametrize("S,G", [(4, 4), (5, 4), (2, 8), (3, 8), (8, 2), (9, 2), (16, 1)])  # 9 > spec_max_tokens
@pytest.mark.parametrize("opt_in", [True, False])
@pytest.mark.parametrize("kv_fp8", [True, False])
def test_route_rule(kv_fp8, opt_in, S, G, arm):
    kw = dict(dims=dict(TP1, hq=8 * G, hkv=8), B=2, S=S, decode=False, has_past=True, all_rows=True, verify_attn=arm,
              spec_max_tokens=16 if G == 1 else 8, kv_fp8=kv_fp8)
    base, got = route(**kw), route(verify_fp8_multi=opt_in, **kw)
    fits = arm != "ctx" and S <= kw["spec_max_tokens"] and S * G <= 16
    assert got.multi == (fits and (not kv_fp8 or opt_in))
    assert base.multi == (fits and not kv_fp8)  # the default: an e4m3 cache stays on the context kernel
    assert dataclasses.replace(got, multi=base.multi) == base  # no other decision reads the keyword
    for off in (dict(has_past=False), dict(all_rows=False)):  # a first prefill, a prefill chunk
        assert not route(verify_fp8_multi=opt_in, **dict(kw, **off)).multi


def test_refusals():
    from mlmicroservicetemplate_amd.models.llama import LlamaTP, init_llama_shard, tiny_config
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    cfg = tiny_config()
    ref = LlamaTP(init_llama_shard(cfg, 1, 0, seed=1), cfg, max_batch=1, max_seq=16, kv_dtype="fp8", kv_prefill="cache",
                  verify_fp8="multi")  # the reference backend accepts and ignores it
    assert ref.verify_fp8 == "multi" and not ref.kv_fp8
    for kw in (dict(verify_fp8="multi"), dict(verify_fp8="multi", kv_dtype="fp8"),
               dict(verify_fp8="split", kv_dtype="fp8", kv_prefill="cache")):
        with pytest.raises(ValueError, match="verify_fp8"):
            LlamaTP({}, cfg, **kw)
    assert LlamaPlugin.parse_verify_fp8({}, "bf16", "rows") == "ctx"
    assert LlamaPlugin.parse_verify_fp8({"verify_fp8": "multi"}, "fp8", "cache") == "multi"
    for extra, kv in (({"verify_fp8": "multi"}, ("bf16", "rows")), ({"verify_fp8": "multi"}, ("fp8", "rows")),
                      ({"verify_fp8": "split"}, ("fp8", "cache"))):
        with pytest.raises(ValueError, match="verify_fp8"):
            LlamaPlugin.parse_verify_fp8(extra, *kv)
