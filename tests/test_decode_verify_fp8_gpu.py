"""The verify step's attention on the e4m3 KV cache (ops/csrc/decode_verify_fp8.hip,
``ops.decode_attention_multi_fp8``) and ``LlamaTP(verify_fp8="multi")``.

Cases: ``attn_cases.ctx_case(fp8=True)`` with the verify tests' ``past`` and ragged counts (everything a launch must
not read is poisoned: bytes 0x7F, NaN scales, NaN K / V columns of qkv).  Oracle: ``R.attention_ctx`` on
``R.kv_dequant_fp8`` of the same bytes.  Bounds: 2e-2 of the largest output magnitude (P is rounded to bf16 before
the PV product: ``flash_attention_ctx_fp8``'s and ``decode_attention_multi``'s bound), the per-head bound of
tests/attn_cases.py on the dequantised rows, and 3e-2 for the model against the reference backend
(tests/test_e2e_gpu.py, test_kv_prefill_cache_gpu.py)."""
import pytest
import torch

import attn_cases as A
from mlmicroservicetemplate_amd import ops
from mlmicroservicetemplate_amd.ops import reference as R
from test_kv_prefill_cache_gpu import FP8, _check_tokens, _llama, _prompts, ref_model, tiny  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
UNSUPPORTED, BAD_ARG = 1002, 1001
K = 3


@pytest.mark.parametrize("Hq,Hkv,T", [(4, 1, 4), (8, 2, 4), (8, 1, 2), (4, 2, 8), (2, 2, 16)])
def test_kernel_vs_oracle_per_slot_and_paged(Hq, Hkv, T):
    c = A.ctx_case(A.VERIFY_PASTS, A.verify_counts(T), T, Hq, Hkv, D, fp8=True, seed=21, device=DEV)
    args = (c["past"], c["lens"], c["B"], T, Hq, Hkv, D)
    ref = R.attention_ctx(c["qkv"], R.kv_dequant_fp8(c["kc"], c["ks"]), R.kv_dequant_fp8(c["vc"], c["vs"]), *args,
                          slot_ids=c["slot_ids"], head_major=True)
    valid = lambda o: A.valid_rows(o, c["B"], T, c["n"])  # noqa: E731
    want, tol = valid(ref), A.tolerance(c["rows"], D)  # the rows hold the dequantised K / V
    slot = (c["kc"], c["vc"], c["ks"], c["vs"])
    run = lambda caches, **kw: ops.decode_attention_multi_fp8(c["qkv"], *caches, *args, slot_ids=c["slot_ids"], **kw)  # noqa: E731
    outs = {64: run(slot, chunk=64), 128: run(slot, chunk=128),
            "paged": run((c["kp"], c["vp"], c["ksp"], c["vsp"]), page_table=c["table"]),
            "bound": run(slot, max_len=c["max_ctx"])}  # a tight host bound changes the grid, not the result
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    for name, out in outs.items():
        got = valid(out)
        assert torch.isfinite(got.float()).all(), name  # no poisoned byte, scale or column was read
        err, herr = A.rel(got, want), A.head_err(got, want, D).max().item()
        print(f"Hq={Hq} Hkv={Hkv} T={T} {name}: rel {err:.5f}, per-head {herr:.5f} (bound {tol:.5f})")
        assert err < 2e-2 and herr < tol, name
    # the same splits in the same order, only the addressing / the grid differs
    assert torch.equal(valid(outs["paged"]), valid(outs[64])) and torch.equal(valid(outs["bound"]), valid(outs[64]))


@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (8, 2), (8, 8)])
def test_one_query_matches_decode_attention_fp8(Hq, Hkv):
    """T = 1 is single-token decode attention on the same poisoned cache (lens 1, 64, 65, 200, 333; slot b = row b,
    336 rows: the decode op's layout).  The merges may contract differently: not bitwise."""
    B = 5
    c = A.ctx_case([0, 63, 64, 199, 332], [1] * B, 1, Hq, Hkv, D, max_seq=336, slot_ids=range(B), fp8=True, seed=3,
                   device=DEV)
    caches = (c["kc"], c["vc"], c["ks"], c["vs"])
    one = ops.decode_attention_fp8(c["qkv"], *caches, c["lens"], Hq, Hkv, D, chunk=64)
    out = torch.full((B, Hq * D), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.decode_attention_multi_fp8(c["qkv"], *caches, c["past"], c["lens"], B, 1, Hq, Hkv, D, out=out)
    err = A.rel(out, one)
    print(f"Hq={Hq} Hkv={Hkv}: T=1 vs decode_attention_fp8 rel {err:.5f}")
    assert torch.isfinite(out.float()).all() and torch.isfinite(one.float()).all() and err < 2e-2


def test_bad_geometry_is_refused():
    Hq, Hkv, T, B, W = 4, 2, 4, 1, 4 + 2 * 2
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, device=DEV, dtype=dt)  # noqa: E731
    one = lambda *s: torch.ones(*s, device=DEV)  # noqa: E731
    qkv, q64, q16 = (z(B * t, W * d, dt=torch.bfloat16) for t, d in ((T, D), (T, 64), (16, D)))
    past, lens = z(B, dt=torch.int32), torch.full((B,), T, dtype=torch.int32, device=DEV)
    table = torch.tensor([[1, 2]], dtype=torch.int32, device=DEV)
    hm, sc = z(2, Hkv, 64, D), one(2, Hkv, 64)
    out = torch.full((16 * B, Hq * D), float("nan"), device=DEV, dtype=torch.bfloat16)
    ws = torch.zeros(1 << 16, device=DEV, dtype=torch.float32)
    op = lambda q, c, s, t, d, pa=past, pt=None, hq=Hq, hkv=Hkv: ops.decode_attention_multi_fp8(  # noqa: E731
        q, c, c, s, s, pa, lens, B, t, hq, hkv, d, page_table=pt)

    def entry(q, cache, scale, t, d, rows, pt=None, hq=Hq, hkv=Hkv, q_stride=None, chunk=64, off=0):  # the C entry
        return ops.lib().mls_decode_attention_multi_fp8(  # max_len = rows
            q.data_ptr(), cache.data_ptr(), cache.data_ptr(), scale.data_ptr() + off, scale.data_ptr(), out.data_ptr(),
            ws.data_ptr(), ws[1 << 15:].data_ptr(), q_stride or q.shape[1], hq * d, past.data_ptr(), lens.data_ptr(),
            None, None if pt is None else pt.data_ptr(), 0 if pt is None else 2, 1 if pt is not None else cache.shape[0],
            B, t, hq, hkv, d, cache.shape[0], rows, rows or 64, chunk, 1.0, ops.stream_ptr(torch.device(DEV)))

    op(qkv, hm, sc, T, D)  # the supported layout launches
    # the wrapper's message; q, cache, scales, T, D; the rows per block the entry is told; the page table; Hq, Hkv
    for match, q, cache, scale, t, d, rows, pt, *heads in (
            ("head-major", qkv, z(2, 64, Hkv, D), sc, T, D, 0, None),                  # row-major [slots, rows, Hkv, D]
            ("head_dim", q64, z(2, Hkv, 64, 64), sc, T, 64, 64, None),                 # D = 64
            ("<= 16", q16, hm, sc, 16, D, 64, None),                                   # T * G = 32
            # T * G <= 16 passes: only the G check keeps these from the G = 8 instantiation
            ("1, 2, 4, 8", z(B, 18 * D, dt=torch.bfloat16), z(2, 1, 64, D), one(2, 1, 64), 1, D, 64, None, 16, 1),
            ("1, 2, 4, 8", z(B, 5 * D, dt=torch.bfloat16), z(2, 1, 64, D), one(2, 1, 64), 1, D, 64, None, 3, 1),
            ("64 rows", qkv, z(4, Hkv, 32, D), one(4, Hkv, 32), T, D, 32, table),      # pages of 32 rows
            ("1024 splits", qkv, z(1, Hkv, 65600, D), one(1, Hkv, 65600), T, D, 65600, None)):  # 1025 splits of 64
        with pytest.raises(ValueError, match=match):
            op(q, cache, scale, t, d, past, pt, *heads)
        assert entry(q, cache, scale, t, d, rows, pt, *heads) == UNSUPPORTED, match
    with pytest.raises(TypeError, match="k_cache"):  # bf16 caches are the other op's
        op(qkv, hm.to(torch.bfloat16), sc, T, D)
    with pytest.raises(TypeError, match="past"):
        op(qkv, hm, sc, T, D, pa=past.long())
    assert entry(qkv, hm, sc, T, D, 64, q_stride=qkv.shape[1] + 4) == BAD_ARG  # misaligned stride
    assert entry(qkv, hm, sc, T, D, 64, off=4) == BAD_ARG                      # misaligned scale pointer
    assert entry(qkv, hm, sc, T, D, 64, chunk=32) == BAD_ARG                   # splits of 64 or 128 rows
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()  # nothing was launched
    assert entry(qkv, hm, sc, T, D, 64) == 0  # and the supported call goes through the entry
    torch.cuda.synchronize()
    assert torch.isfinite(out[:T].float()).all()


@pytest.fixture
def counted(monkeypatch):
    """Calls of the new op (a captured step calls it while it warms up and records)."""
    calls, inner = [], ops.decode_attention_multi_fp8
    monkeypatch.setattr(ops, "decode_attention_multi_fp8", lambda *a, **kw: calls.append(a[8]) or inner(*a, **kw))
    monkeypatch.setattr(ops, "decode_attention_multi", lambda *a, **kw: pytest.fail("the bf16 verify kernel"))
    return calls


@pytest.mark.parametrize("kv_pages", [0, 24])
def test_fused_verify_step_vs_reference_backend(tiny, ref_model, counted, kv_pages):  # noqa: F811
    from mlmicroservicetemplate_amd.models.llama import GenParams

    ids, lens = _prompts()
    B, S = ids.shape
    T, STEPS = K + 1, 4
    cont = ref_model.generate(ids, lens, GenParams(max_new_tokens=T * STEPS)).to(DEV)  # the reference's own greedy run
    pos = torch.arange(S, device=DEV, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
    n = torch.full((B,), T, dtype=torch.int32, device=DEV)
    vals = []
    for m in (_llama(tiny, "reference", kv_pages, **FP8), _llama(tiny, "fused", kv_pages, verify_fp8="multi", **FP8)):
        for b in range(B if kv_pages else 0):
            m.pages.assign(b, 256)
        m.step(ids, pos, lens, decode=False, k=8)
        vals.append([m.verify_step(cont[:, T * s: T * s + T].to(torch.int32), lens + T * s, n, 8,  # teacher-forced
                                   max_ctx=S + T * s + T)[0].reshape(B * T, -1).float().clone() for s in range(STEPS)])
    err = A.rel(torch.cat(vals[1]), torch.cat(vals[0]))
    print(f"kv_pages={kv_pages}: fused verify (verify_fp8=multi) vs reference top-k values rel {err:.4f}")
    assert err <= 3e-2 and counted and set(counted) == {T}


@pytest.mark.parametrize("kv_pages,spec_device", [(0, False), (24, False), (0, True)])
def test_fused_generate_speculative(tiny, ref_model, counted, kv_pages, spec_device):  # noqa: F811
    from mlmicroservicetemplate_amd.models.llama import GenParams

    ids, lens = _prompts()
    m = _llama(tiny, "fused", kv_pages, verify_fp8="multi", **FP8)
    got = m.generate(ids, lens, GenParams(max_new_tokens=24), speculate=K, spec_device=spec_device).cpu()
    assert got.shape == (3, 24) and m.spec_stats["steps"] >= 1
    for b in range(3):  # never against another fused route's tokens: the reference, on the run's own prefix
        _check_tokens(ref_model, ids[b, : int(lens[b])].tolist(), got[b].tolist())
    assert counted and set(counted) == {K + 1}
