"""models/llama_route.py: the per-step kernel routing of the fused Llama forward as a pure function.
The expected values are the rules as models/llama.py held them inline (each with its measurement, now
quoted next to the rule): row-count thresholds 4 (e4m3) / 16 (fused-norm GEMM) / 24 (packed) /
w4_max_rows (int4), the TP = 1 residual fold, the o-prologue combine up to 32 head rows, the fused
all-reduce, the verify attention's 16 lane columns, the overlapped TP prefill, the decode split."""
import sys

import pytest

from mlmicroservicetemplate_amd.models.llama_route import proj_tiers, step_route

# Llama-3-8B on one GPU, and one rank of TP = 8
TP1 = dict(tp=1, hq=32, hkv=8, head_dim=128, hidden=4096)
TP8 = dict(tp=8, hq=4, hkv=1, head_dim=128, hidden=4096)


def route(dims=TP1, **kw):
    """A decode step of B rows on a bf16 model with packed copies and every switch at its default."""
    a = dict(B=1, S=1, decode=True, has_past=False, all_rows=False, have_packed=True, have_w4=False,
             have_fp8=False, o_packed=True, o_fp8=False, w4_max_rows=0, pk_fold=True, prefill_fold=False,
             fuse_combine=True, fuse_add_norm=True, ar_fuse=True, tp_overlap=True, verify_attn="multi",
             spec_max_tokens=8, dec_chunk=0, ar_fusable=dims["tp"] > 1, capturing=False)
    a.update(dims)
    a.update(kw)
    return step_route(**a)


def test_module_needs_no_torch():
    mod = sys.modules[step_route.__module__]
    src = open(mod.__file__).read()
    assert "import torch" not in src and "from torch" not in src and "torch" not in vars(mod)


def test_packed_boundary():
    assert route(B=24).packed and not route(B=25).packed
    assert not route(B=24, have_packed=False, o_packed=False).packed


def test_fused_norm_boundary():
    assert route(B=16).fuse and not route(B=17).fuse
    assert route(B=4, S=4, decode=False).fuse and not route(B=1, S=17, decode=False).fuse  # rows, not batch


def test_int4_boundary():
    # an int4 model packs no bf16 copy of the layer projections, only of the lm_head
    w4 = dict(have_w4=True, w4_max_rows=32, o_packed=False)
    r = route(B=32, **w4)
    assert r.w4 and not r.packed and r.fold and not r.fuse_rn
    r = route(B=33, **w4)
    assert not r.w4 and not r.packed and not r.fold and r.fuse_rn
    assert not route(TP8, B=33, **w4).fuse_rn
    assert not route(B=32, have_w4=True, w4_max_rows=16, o_packed=False).w4  # MLS_W4_MAX_ROWS


def test_fp8_tier():
    assert route(B=4, have_fp8=True).fp8 and not route(B=5, have_fp8=True).fp8
    assert not route(B=4).fp8
    tr = route(B=4, have_fp8=True).proj
    assert tr.fp8_for(4096) and not tr.fp8_for(14336)  # 4 * K * 2 <= 65536
    assert tr.fp8_for(8192) and not tr.fp8_for(8193)
    assert not route(B=5, have_fp8=True).proj.fp8_for(64)


def test_fold():
    assert route(B=1).fold
    assert not route(B=1, pk_fold=False).fold
    assert not route(B=1, have_packed=False, o_packed=False).fold
    assert not route(dict(TP1, tp=2, hq=16, hkv=4), B=1).fold
    prefill = dict(B=2, S=20, decode=False)
    assert not route(**prefill).fold and route(**prefill, prefill_fold=True).fold
    assert not route(B=40, prefill_fold=True).fold  # a decode step above the packed rows
    assert not route(dict(TP1, tp=2, hq=16, hkv=4), **prefill, prefill_fold=True).fold


def test_fuse_combine():
    assert route(B=1).fuse_combine
    assert not route(B=2).fuse_combine  # 64 head rows
    assert route(TP8, B=4).fuse_combine and not route(TP8, B=5).fuse_combine
    assert not route(B=1, fuse_combine=False).fuse_combine
    assert not route(B=1, S=1, decode=False).fuse_combine
    assert not route(B=1, o_fp8=True, have_fp8=True).fuse_combine
    assert not route(B=1, o_packed=False).fuse_combine


def test_ar_fuse():
    assert route(TP8, B=8).ar_fuse
    assert not route(B=8, ar_fusable=True).ar_fuse  # TP = 1
    assert not route(TP8, B=8, ar_fusable=False).ar_fuse
    assert not route(TP8, B=8, ar_fuse=False).ar_fuse
    assert not route(TP8, B=8, have_packed=False, o_packed=False).ar_fuse
    assert route(TP8, B=24).ar_fuse and not route(TP8, B=25).ar_fuse  # packed copies not in use


def test_multi():
    verify = dict(decode=False, has_past=True, all_rows=True)
    assert route(B=2, S=4, **verify).multi
    assert not route(B=2, S=5, **verify).multi  # 5 positions x 4 heads per KV head = 20 lane columns > 16
    assert not route(B=2, S=4, **verify, verify_attn="ctx").multi
    assert not route(B=2, S=4, decode=False, has_past=True, all_rows=False).multi
    assert not route(B=2, S=4, decode=False).multi
    assert route(dict(TP1, hq=8, hkv=8), B=1, S=8, **verify).multi
    assert not route(dict(TP1, hq=8, hkv=8), B=1, S=9, **verify).multi  # spec_max_tokens


def test_overlap():
    on = dict(B=2, S=32, decode=False)
    assert route(TP8, **on).overlap
    assert not route(**on).overlap  # TP = 1
    assert not route(TP8, **on, has_past=True).overlap
    assert not route(TP8, B=1, S=64, decode=False).overlap
    assert not route(TP8, B=2, S=31, decode=False).overlap  # 62 rows
    assert not route(TP8, **on, tp_overlap=False).overlap
    assert not route(TP8, **on, capturing=True).overlap
    assert not route(TP8, B=64).overlap  # a decode step


def test_dec_chunk():
    assert route(B=1).dec_chunk == 64 and route(B=31).dec_chunk == 64
    assert route(B=32).dec_chunk == 128 and route(B=128).dec_chunk == 128
    assert route(B=1, dec_chunk=128).dec_chunk == 128 and route(B=64, dec_chunk=256).dec_chunk == 256


def test_fuse_rn():
    assert route(B=25).fuse_rn and not route(B=24).fuse_rn
    assert route(B=17, have_packed=False, o_packed=False).fuse_rn
    assert not route(B=16, have_packed=False, o_packed=False).fuse_rn
    assert not route(B=25, fuse_add_norm=False).fuse_rn
    assert not route(B=2, S=20, decode=False, prefill_fold=True).fuse_rn
    assert not route(TP8, B=25).fuse_rn


@pytest.mark.parametrize("nb,packed,fuse", [(2, True, True), (16, True, True), (17, True, False), (24, True, False),
                                            (25, False, False)])
def test_lm_head_tiers(nb, packed, fuse):
    """The lm_head walks the same ladder at its own row count, never through int4 codes."""
    tr = proj_tiers(nb, True, False, False, 0)
    assert (tr.packed, tr.fuse, tr.w4, tr.fp8) == (packed, fuse, False, False)
