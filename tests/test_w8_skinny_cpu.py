"""``w8_decode="skinny"`` without a GPU: the route's new tier, the fused form's host limit and the refusals."""
import dataclasses

import pytest

from mlmicroservicetemplate_amd.models.llama_route import proj_tiers
from test_llama_route_cpu import route


@pytest.mark.parametrize("rows", [1, 8, 16, 17, 26, 512])
@pytest.mark.parametrize("have_w8", [True, False])
@pytest.mark.parametrize("skinny", [True, False])
@pytest.mark.parametrize("bound", [16, 8])
def test_tier_is_on_exactly_below_the_bound_and_changes_nothing_else(rows, have_w8, skinny, bound):
    base = proj_tiers(rows, False, False, False, 0, have_w8)
    got = proj_tiers(rows, False, False, False, 0, have_w8, w8_skinny=skinny, w8_skinny_rows=bound)
    assert got.w8s == (have_w8 and skinny and rows <= bound) and not base.w8s
    assert dataclasses.replace(got, w8s=False) == base
    kw = dict(B=rows, have_packed=False, have_w8=have_w8)
    step, step0 = route(w8_skinny=skinny, w8_skinny_rows=bound, **kw), route(**kw)
    assert step.proj == got and dataclasses.replace(step, proj=base) == step0


def test_fused_fits_on_the_llama3_8b_corners():
    from mlmicroservicetemplate_amd import ops

    assert ops.skinny_w8_fused_fits(8, 4096) and not ops.skinny_w8_fused_fits(9, 4096)
    assert ops.skinny_w8_fused_fits(2, 14336) and not ops.skinny_w8_fused_fits(3, 14336)
    assert not ops.skinny_w8_fused_fits(17, 128) and not ops.skinny_w8_fused_fits(1, 192)


def test_refusals():
    from mlmicroservicetemplate_amd.models.llama import LlamaTP, tiny_config
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin

    cfg = tiny_config()
    for kw in (dict(w8_decode="skinny"), dict(w8_decode="skinny", weight_dtype="int4"),
               dict(w8_decode="ring", weight_dtype="w8a8")):
        with pytest.raises(ValueError, match="w8_decode"):
            LlamaTP({}, cfg, **kw)
    assert LlamaPlugin.parse_w8_decode({}, "bf16") == "tile"
    assert LlamaPlugin.parse_w8_decode({"w8_decode": "skinny"}, "w8a8") == "skinny"
    for extra, wd in (({"w8_decode": "skinny"}, "bf16"), ({"w8_decode": "ring"}, "w8a8")):
        with pytest.raises(ValueError, match="w8_decode"):
            LlamaPlugin.parse_w8_decode(extra, wd)
