"""``ops.decode_attention_wide_fp8`` (ops/csrc/decode_verify_wide_fp8.hip, 16 < T * Hq / Hkv <= 64) on
``attn_cases.ctx_case(fp8=True)`` with everything a launch must not read poisoned (bytes 0x7F, NaN scales and K / V
columns), against ``R.attention_ctx`` on ``R.kv_dequant_fp8`` of the same bytes under test_decode_verify_fp8_gpu.py's
bounds; ``LlamaTP(verify_fp8="wide")`` against the reference backend by ``_check_tokens``."""
import pytest
import torch

import attn_cases as A
from mlmicroservicetemplate_amd import ops
from mlmicroservicetemplate_amd.ops import reference as R
from test_kv_prefill_cache_gpu import FP8, _check_tokens, _llama, _prompts, ref_model, tiny  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
DEV, D = "cuda:0", 128
UNSUPPORTED, BAD_ARG = 1002, 1001
PASTS = [0, 63, 60, 128, 125, 200]  # one key; a full split; steps across rows 64 and 128; an empty step; 4 splits
_CASES = {}


def _case(Hq, Hkv, T):
    if (Hq, Hkv, T) not in _CASES:
        c = A.ctx_case(PASTS, [T, 1, T, 1, T, max(1, T // 2)], T, Hq, Hkv, D, fp8=True, seed=41, device=DEV)
        # ctx_case builds no empty step: row 3 gives its one query back, and the cache row it had is poisoned
        c["n"][3], c["lens"][3] = 0, c["past"][3]
        for cache, fill in ((c["kc"], A.NAN8), (c["vc"], A.NAN8), (c["ks"], float("nan")), (c["vs"], float("nan"))):
            cache[int(c["slot_ids"][3]), :, PASTS[3]:] = fill
        c.update(A.paged_views(c, 64, c["table"]))
        c["args"] = (c["past"], c["lens"], c["B"], T, Hq, Hkv, D)
        c["slot"], c["pages"] = (c["kc"], c["vc"], c["ks"], c["vs"]), (c["kp"], c["vp"], c["ksp"], c["vsp"])
        deq = R.kv_dequant_fp8(c["kc"], c["ks"]), R.kv_dequant_fp8(c["vc"], c["vs"])
        c["want"] = A.valid_rows(R.attention_ctx(c["qkv"], *deq, *c["args"], slot_ids=c["slot_ids"], head_major=True),
                                 c["B"], T, c["n"])
        c["tol"] = A.tolerance(A.rows_ctx(c["qkv"], *deq, *c["args"], slot_ids=c["slot_ids"]), D)
        _CASES[(Hq, Hkv, T)] = c
    return _CASES[(Hq, Hkv, T)]


def _run(c, op=None, paged=False, **kw):
    kw.update(page_table=c["table"]) if paged else None
    return (op or ops.decode_attention_wide_fp8)(c["qkv"], *c["pages" if paged else "slot"], *c["args"],
                                                 slot_ids=c["slot_ids"], **kw)


@pytest.mark.parametrize("Hq,Hkv,T", [(8, 2, 5), (8, 2, 8), (8, 1, 5), (8, 1, 8), (4, 2, 16)])
def test_kernel_vs_oracle_per_slot_and_paged(Hq, Hkv, T):
    c = _case(Hq, Hkv, T)
    outs = {64: _run(c, chunk=64), 128: _run(c, chunk=128), "paged": _run(c, paged=True),
            "bound": _run(c, max_len=c["max_ctx"])}  # a tight host bound changes the grid, not the result
    assert torch.isfinite(c["want"]).all()
    valid = {name: A.valid_rows(out, c["B"], T, c["n"]) for name, out in outs.items()}
    for name, got in valid.items():
        assert torch.isfinite(got.float()).all(), name  # no poisoned byte, scale or column was read
        err, herr = A.rel(got, c["want"]), A.head_err(got, c["want"], D).max().item()
        print(f"Hq={Hq} Hkv={Hkv} T={T} {name}: rel {err:.5f}, per-head {herr:.5f} (bound {c['tol']:.5f})")
        assert err < 2e-2 and herr < c["tol"], name
    assert torch.equal(valid["paged"], valid[64]) and torch.equal(valid["bound"], valid[64])  # the same splits and order


def test_narrow_shapes_forward_bit_identical():
    c = _case(8, 2, 4)  # T * G = 16: the narrow kernel's own shape
    for kw in (dict(chunk=64), dict(paged=True)):
        assert torch.equal(_run(c, **kw), _run(c, ops.decode_attention_multi_fp8, **kw))


def test_empty_rows_graph_replay_and_workspace():
    c = _case(8, 2, 5)
    B, T, Hq = c["B"], 5, 8
    past, lens = c["past"].clone(), c["past"].clone()
    args, kw = (c["qkv"], *c["slot"], past, lens, B, T, Hq, 2, D), dict(slot_ids=c["slot_ids"])
    out = ops.decode_attention_wide_fp8(*args, **kw)  # lens == past: every row is empty
    assert torch.isfinite(out.float()).all() and not out.any()
    lens.copy_(c["lens"])
    ws = torch.empty(B * T * Hq * 6 * (D + 2), device=DEV)  # 6 splits of 64 hold the slot's 333 rows
    out = torch.empty(B * T, Hq * D, device=DEV, dtype=torch.bfloat16)
    ops.decode_attention_wide_fp8(*args, workspace=ws, out=out, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.decode_attention_wide_fp8(*args, workspace=ws, out=out, **kw)
    for shift in (0, 3, 0, 2):  # lens 65 -> 62 and 130 -> 127: a split fewer, the 65-row sequence on the direct path
        past.copy_((c["past"] - shift).clamp_min(0))
        lens.copy_(past + c["n"])
        g.replay()
        eager = ops.decode_attention_wide_fp8(*args, **kw)
        assert torch.equal(A.valid_rows(out, B, T, c["n"]), A.valid_rows(eager, B, T, c["n"])), shift
    assert torch.equal(ops.decode_attention_wide_fp8(*args, workspace=ws[:1], **kw), eager)  # too short: replaced


@pytest.mark.parametrize("Hq,Hkv,T,d,chunk,match,code", [
    (8, 8, 17, 128, 64, "<= 64", UNSUPPORTED), (8, 2, 17, 128, 64, "<= 64", UNSUPPORTED),  # T = 17; T * G = 68
    (6, 2, 5, 128, 64, "1, 2, 4, 8", UNSUPPORTED), (8, 2, 5, 64, 64, "head_dim", UNSUPPORTED),
    (8, 2, 5, 128, 32, "64 or 128", BAD_ARG)])
def test_refusals(Hq, Hkv, T, d, chunk, match, code):
    zeros = lambda *s, dt=torch.uint8: torch.zeros(*s, device=DEV, dtype=dt)  # noqa: E731
    q, cache, sc = zeros(T, (Hq + 2 * Hkv) * d, dt=torch.bfloat16), zeros(2, Hkv, 64, d), zeros(2, Hkv, 64, dt=torch.float32)
    past, lens = zeros(1, dt=torch.int32), torch.full((1,), T, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match=match):
        ops.decode_attention_wide_fp8(q, cache, cache, sc, sc, past, lens, 1, T, Hq, Hkv, d, chunk=chunk)
    out, ws = torch.full((T, Hq * d), float("nan"), device=DEV, dtype=torch.bfloat16), zeros(1 << 16, dt=torch.float32)
    rc = ops.lib().mls_decode_attention_wide_fp8(
        q.data_ptr(), cache.data_ptr(), cache.data_ptr(), sc.data_ptr(), sc.data_ptr(), out.data_ptr(), ws.data_ptr(),
        ws[1 << 15:].data_ptr(), q.shape[1], Hq * d, past.data_ptr(), lens.data_ptr(), None, None, 0, 2, 1, T, Hq, Hkv, d,
        2, 64, 64, chunk, 1.0, ops.stream_ptr(torch.device(DEV)))
    assert rc == code and torch.isnan(out.float()).all()  # nothing was launched


# ------------------------------------------------------------------ the fused model (heads 8, kv_heads 2, head_dim 128)
@pytest.mark.parametrize("speculate,kv_pages,spec_device", [(5, 0, False), (7, 24, False), (7, 0, True), (5, 24, True),
                                                            (3, 0, False)])  # 16 columns: the narrow op only
def test_fused_generate_speculates(tiny, ref_model, monkeypatch, speculate, kv_pages, spec_device):  # noqa: F811
    from mlmicroservicetemplate_amd.models.llama import GenParams

    calls = {}  # seq of every call of the three ops an e4m3 verify step can take (a captured step calls as it records)
    for name in ("decode_attention_wide_fp8", "decode_attention_multi_fp8", "flash_attention_ctx_fp8"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=getattr(ops, name), **kw: (
            calls.setdefault(_n, []).append(a[8]) or _f(*a, **kw)))
    ids, lens = _prompts()
    m = _llama(tiny, "fused", kv_pages, verify_fp8="wide", **FP8)
    got = m.generate(ids, lens, GenParams(max_new_tokens=24), speculate=speculate, spec_device=spec_device).cpu()
    assert got.shape == (3, 24) and m.spec_stats["steps"] >= 1
    for b in range(3):  # never against another fused route's tokens: the reference, on the run's own prefix
        _check_tokens(ref_model, ids[b, : int(lens[b])].tolist(), got[b].tolist())
    ran, idle = ("decode_attention_wide_fp8", "decode_attention_multi_fp8")[::1 if speculate > 3 else -1]
    assert set(calls[ran]) == {speculate + 1} and idle not in calls  # every verify step ran that op
    assert speculate + 1 not in calls["flash_attention_ctx_fp8"]  # and none the context kernel
