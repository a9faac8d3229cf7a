"""The wide verify attention (ops/csrc/decode_verify_wide.hip, ``ops.decode_attention_wide``: 16 < T * Hq / Hkv <=
64) against the fp32 oracle of tests/attn_cases.py on the same bf16 cache rows, and ``LlamaTP(verify_cols=64)``
against the reference backend.  Bound: attn_cases' per-(row, head) ``tolerance`` (4 x the rounding model)."""
import pytest
import torch

import attn_cases as A
from mlmicroservicetemplate_amd import ops
from test_decode_verify_gpu import _check_tokens, _oracle_drafter, _prompts, ref_model, tiny  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
UNSUPPORTED = 1002
PASTS = [0, 63, 60, 128, 125, 200]  # one key; a full split; steps across rows 64 and 128; an empty step; 4 splits
_CASES = {}


def _case(Hq, Hkv, T):
    """Ragged counts 0 .. T in one batch; unused slots, rows >= lens, page tails and qkv's K / V columns are NaN."""
    if (Hq, Hkv, T) not in _CASES:
        c = A.ctx_case(PASTS, [T, 1, T, 1, T, max(1, T // 2)], T, Hq, Hkv, D, seed=31, device=DEV)
        # ctx_case builds no empty step: row 3 gives its one query back, and the cache row it had goes NaN
        c["n"][3], c["lens"][3] = 0, c["past"][3]
        for cache in (c["kc"], c["vc"]):
            cache[int(c["slot_ids"][3]), :, PASTS[3]:] = float("nan")
        c.update(A.paged_views(c, 64, c["table"]))
        c["args"] = (c["past"], c["lens"], c["B"], T, Hq, Hkv, D)
        c["oracle_rows"] = A.rows_ctx(c["qkv"], c["kc"], c["vc"], *c["args"], slot_ids=c["slot_ids"])
        _CASES[(Hq, Hkv, T)] = c
    return _CASES[(Hq, Hkv, T)]


def _run(c, op=None, paged=False, **kw):
    kc, vc = (c["kp"], c["vp"]) if paged else (c["kc"], c["vc"])
    kw.update(page_table=c["table"]) if paged else None
    return (op or ops.decode_attention_wide)(c["qkv"], kc, vc, *c["args"], slot_ids=c["slot_ids"], **kw)


@pytest.mark.parametrize("Hq,Hkv,T", [(8, 2, 5), (8, 2, 8), (8, 1, 5), (8, 1, 8), (4, 2, 16)])
def test_kernel_vs_oracle_per_slot_and_paged(Hq, Hkv, T):
    c = _case(Hq, Hkv, T)
    want, tol = A.attend(c["oracle_rows"]), A.tolerance(c["oracle_rows"], D)
    outs = {64: _run(c, chunk=64), 128: _run(c, chunk=128), "paged": _run(c, paged=True)}
    torch.cuda.synchronize()
    valid = {name: A.valid_rows(out, c["B"], T, c["n"]) for name, out in outs.items()}
    for name, got in valid.items():
        assert torch.isfinite(got.float()).all(), name  # no poisoned row, page or column was read
        err = A.head_err(got, want, D).max().item()
        print(f"Hq={Hq} Hkv={Hkv} T={T} {name}: per-head {err:.5f} (bound {tol:.5f})")
        assert err < tol, name
    assert torch.equal(valid["paged"], valid[64])  # the same splits in the same order, only the addressing differs


def test_narrow_shapes_forward_bit_identical():
    c = _case(8, 2, 4)  # T * G = 16: the narrow kernel's own shape
    for kw in (dict(chunk=64), dict(chunk=128), dict(paged=True)):
        assert torch.equal(_run(c, **kw), _run(c, ops.decode_attention_multi, **kw))


def test_empty_rows_are_finite_and_zero():
    Hq, Hkv, T, B = 8, 2, 5, 3
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    kc = torch.full((B, Hkv, 256, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    kc[1, :, :100] = 1.0
    past = torch.tensor([0, 100, 0], dtype=torch.int32, device=DEV)
    out = ops.decode_attention_wide(qkv, kc, kc, past, past.clone(), B, T, Hq, Hkv, D)
    assert torch.isfinite(out.float()).all() and not out.any()


def test_graph_replay_equals_eager_across_a_split_boundary():
    c = _case(8, 2, 5)
    B, T, Hq = c["B"], 5, 8
    past, lens = c["past"].clone(), c["lens"].clone()
    ws = torch.empty(B * T * Hq * 6 * (D + 2), device=DEV)  # 6 splits of 64 hold the slot's 333 rows
    out = torch.empty(B * T, Hq * D, device=DEV, dtype=torch.bfloat16)
    args = (c["qkv"], c["kc"], c["vc"], past, lens, B, T, Hq, 2, D)
    ops.decode_attention_wide(*args, slot_ids=c["slot_ids"], workspace=ws, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.decode_attention_wide(*args, slot_ids=c["slot_ids"], workspace=ws, out=out)
    for shift in (0, 3, 0, 2):  # lens 65 -> 62 and 130 -> 127: a split fewer, the 65-row sequence on the direct path
        past.copy_((c["past"] - shift).clamp_min(0))
        lens.copy_(past + c["n"])
        g.replay()
        eager = ops.decode_attention_wide(*args, slot_ids=c["slot_ids"])
        assert torch.equal(A.valid_rows(out, B, T, c["n"]), A.valid_rows(eager, B, T, c["n"])), shift
    # the workspace rule of the narrow op: one that is too short is replaced, never overrun
    short = ops.decode_attention_wide(*args, slot_ids=c["slot_ids"], workspace=ws[:1])
    assert torch.equal(short, eager)


@pytest.mark.parametrize("Hq,Hkv,T,d,row_major,match", [(8, 1, 9, 128, False, "<= 64"), (8, 2, 5, 64, False, "head_dim"),
                                                       (6, 2, 5, 128, False, "1, 2, 4, 8"),
                                                       (8, 2, 5, 128, True, "head-major")])
def test_refusals(Hq, Hkv, T, d, row_major, match):
    zeros = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device=DEV, dtype=dt)  # noqa: E731
    q, cache = zeros(T, (Hq + 2 * Hkv) * d), zeros(2, 64, Hkv, d) if row_major else zeros(2, Hkv, 64, d)
    past, lens = zeros(1, dt=torch.int32), torch.full((1,), T, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match=match):
        ops.decode_attention_wide(q, cache, cache, past, lens, 1, T, Hq, Hkv, d)
    out, ws = torch.full((T, Hq * d), float("nan"), device=DEV, dtype=torch.bfloat16), zeros(1 << 16, dt=torch.float32)
    rc = ops.lib().mls_decode_attention_wide(q.data_ptr(), cache.data_ptr(), cache.data_ptr(), out.data_ptr(),
                                             ws.data_ptr(), ws[1 << 15:].data_ptr(), q.shape[1], Hq * d, past.data_ptr(),
                                             lens.data_ptr(), None, None, 0, 2, 1, T, Hq, Hkv, d, 2,
                                             0 if row_major else 64, 64, 64, 1.0, ops.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and torch.isnan(out.float()).all()  # nothing was launched


# ------------------------------------------------------------------ the fused model (heads 8, kv_heads 2, head_dim 128)
NEW = 24


def _llama(tiny, backend="fused", kv_pages=0, **kw):  # noqa: F811
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    return LlamaTP(tiny[1], tiny[0], backend=backend, device=DEV, max_batch=4, max_seq=512, kv_pages=kv_pages, **kw)


@pytest.fixture(scope="module")
def plain(tiny):  # noqa: F811
    """The plain fused run's continuation: what an oracle drafter proposes."""
    from mlmicroservicetemplate_amd.models.llama import GenParams

    ids, lens = _prompts()
    return _llama(tiny).generate(ids, lens, GenParams(max_new_tokens=NEW)).tolist()


@pytest.mark.parametrize("speculate,kv_pages,loop", [(5, 0, "oracle"), (7, 24, "oracle"), (7, 0, "wrong"),
                                                     (5, 24, "wrong"), (5, 24, "device"), (7, 0, "device")])
def test_fused_generate_speculates_past_three_drafts(tiny, ref_model, plain, monkeypatch, speculate, kv_pages, loop):  # noqa: F811
    from mlmicroservicetemplate_amd.models.llama import GenParams

    calls, inner = [], ops.decode_attention_wide
    monkeypatch.setattr(ops, "decode_attention_wide", lambda *a, **kw: calls.append(a[6]) or inner(*a, **kw))
    ids, lens = _prompts()
    prompts = [ids[b, : int(lens[b])].tolist() for b in range(3)]
    gp = GenParams(max_new_tokens=NEW)
    m = _llama(tiny, kv_pages=kv_pages, verify_cols=64)
    kw = dict(spec_device=True) if loop == "device" else dict(
        drafter=_oracle_drafter(prompts, plain) if loop == "oracle" else (lambda toks, n: [1] * n))
    got = m.generate(ids, lens, gp, speculate=speculate, **kw).cpu()
    assert got.shape == (3, NEW) and calls and set(calls) == {speculate + 1}  # every verify step ran the wide op
    for b in range(3):  # never against another fused route's tokens: the reference, on the run's own prefix
        _check_tokens(ref_model, prompts[b], got[b].tolist())
    print(f"speculate={speculate} kv_pages={kv_pages} {loop}: {m.spec_stats}")
    if loop == "oracle":
        assert m.spec_stats["accepted"] > 0 and m.spec_stats["steps"] < NEW - 1
    if kv_pages:
        assert m.pages.free_pages == kv_pages - 1


def test_default_verify_cols_never_takes_the_wide_op(tiny, monkeypatch):  # noqa: F811
    from mlmicroservicetemplate_amd.models.llama import GenParams

    monkeypatch.setattr(ops, "decode_attention_wide", lambda *a, **kw: pytest.fail("the wide verify kernel"))
    assert _llama(tiny).generate(*_prompts(), GenParams(max_new_tokens=8), speculate=3).shape == (3, 8)
    with pytest.raises(ValueError, match="<= 16"):
        _llama(tiny).generate(*_prompts(), GenParams(max_new_tokens=8), speculate=5)
