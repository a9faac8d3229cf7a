"""Every attention kernel at its edges, against the fp32 oracle, in the per-head metric of
tests/attn_cases.py: ``flash_fwd_kernel`` / ``flash_fwd2_kernel`` (``ops.flash_attention``, ``_rows``),
``decode_attn_kernel`` / ``decode_attn_mfma_kernel`` (``ops.decode_attention``), ``decode_attn_fp8_kernel``
(``ops.decode_attention_fp8``), ``decode_verify_kernel`` (``ops.decode_attention_multi``) and
``flash_ctx_kernel<FP8, SPLIT>`` with its combine (``ops.flash_attention_ctx``, ``_fp8``).

The inputs are ``attn_cases.SPECS``: the smallest shapes at which each path still runs its edges (lens /
past either side of the 64- and 128-row boundaries, a one-key row, ragged valid counts, more splits than
combine lanes), everything a launch must not read poisoned with NaN (0x7F bytes and NaN scales for e4m3).
tests/test_attn_cases_cpu.py proves on the CPU that on these inputs every mutant oracle -- a lost last key,
one key too many inside the row, a lost first / last key of a tile, a lost split, the next KV head, a merge
without rescale, an un-rotated appended K row -- is at least 3 x ``tol`` away from the oracle; each test here
asserts ``head_err(kernel, oracle).max() < tol`` with ``tol = FACTOR x`` the rounding model's error on the
same inputs (computed on the device, never from a kernel), finite valid rows, and the bit-for-bit relations
the older tests hold: paged == per-slot at 64-row splits, row-major == head-major, repeat launches equal.

Measured on an MI355X, largest per-head error of a family's launches next to the rounding model's on the
same inputs (every factor is 4; each test prints its own figures with ``-s``):

    family                                   kernel          model           kernel / model, worst launch
    decode valu (plain / rope)               0.0036 / 0.0036 0.0040-0.0061   0.85
    decode mfma (plain / rope)               0.0043 / 0.0042 0.0040-0.0059   1.00
    decode e4m3 (plain / rope)               0.0054 / 0.0058 0.0071-0.0110   0.73
    verify (decode_attention_multi)          0.0056          0.0050-0.0056   1.00
    ctx bf16, splits 1 / 2 / 4               0.0072          0.0049-0.0072   1.04
    ctx e4m3, splits 1 / 2 / 4               0.0161          0.0055-0.0161   1.09
    prefill v1 and v2, rows                  0.0087          0.0046-0.0087   1.00"""
import pytest
import torch

import attn_cases as A
from mlmicroservicetemplate_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0  # tol = FACTOR x model error; test_attn_cases_cpu.py holds every mutant to >= 3 x tol at this factor


@pytest.fixture(scope="module")
def ops():
    from mlmicroservicetemplate_amd import ops as o

    o.lib()
    return o


_PAGED = {}


def _paged(name, page_rows):
    """The case's caches as page pools of ``page_rows`` rows (shared; rope-mode launches clone them)."""
    key = (name, page_rows)
    if key not in _PAGED:
        _PAGED[key] = A.paged_views(A.case(name, DEV), page_rows, seed=page_rows)
    return _PAGED[key]


def _check(label, got, want, rows, D, factor=FACTOR):
    assert torch.isfinite(got.float()).all(), label  # no poisoned row, byte, scale or column was read
    model = A.head_err(A.attention_model(rows), A.attend(rows), D).max().item()
    err = A.head_err(got, want, D).max().item()
    print(f"ATTN-EDGE {label}: kernel {err:.4f} model {model:.4f} tol {factor * model:.4f}")
    assert err < factor * model, label
    return err


# ------------------------------------------------------------------ decode, bf16 cache
DECODE = [(s, impl) for s in ((4, 1, 128), (8, 2, 128), (16, 2, 128), (12, 12, 64)) for impl in ("valu", "mfma")
          if impl == "valu" or s[2] == 128]  # the matrix-core kernel: D = 128


def _decode_layouts(name, c, chunk):
    """(label, k, v, keywords) of the four cache images: row- / head-major, per-slot / paged."""
    p = _paged(name, chunk)
    rm = lambda t: t.permute(0, 2, 1, 3).contiguous()  # noqa: E731
    return [("rows", rm(c["kc"]), rm(c["vc"]), {}),
            ("heads", c["kc"], c["vc"], dict(head_major=True)),
            ("rows paged", rm(p["kp"]), rm(p["vp"]), dict(page_table=p["table"])),
            ("heads paged", p["kp"], p["vp"], dict(page_table=p["table"], head_major=True))]


@pytest.mark.parametrize("shape,impl", DECODE)
def test_decode_attention(ops, shape, impl):
    Hq, Hkv, D = shape
    name = f"decode-{Hq}-{Hkv}-{D}"
    c = A.case(name, DEV)
    want = R.decode_attention(c["q"], c["kc"].permute(0, 2, 1, 3), c["vc"].permute(0, 2, 1, 3), c["lens"], Hq, Hkv, D)
    cnt = torch.zeros(c["B"] * Hkv, device=DEV, dtype=torch.int32)
    for chunk in ((64, 128, 256) if impl == "valu" else (64, 128)):
        outs = {}
        for label, k, v, kw in _decode_layouts(name, c, chunk):
            for max_len in (None, max(A.DECODE_LENS)):  # loose: what the cache holds; tight: the longest row
                out = ops.decode_attention(c["q"], k, v, c["lens"], Hq, Hkv, D, chunk=chunk, counters=cnt, impl=impl,
                                           max_len=max_len, **kw)
                again = ops.decode_attention(c["q"], k, v, c["lens"], Hq, Hkv, D, chunk=chunk, counters=cnt,
                                             impl=impl, max_len=max_len, **kw)
                _check(f"decode {impl} {shape} chunk {chunk} {label} max_len {max_len}", out, want, c["rows"], D)
                assert torch.equal(again, out)
                assert not cnt.any()  # the ticket counters are back at zero
                outs[(label, max_len)] = out
        if chunk == 64:  # the same splits in the same order, only the addressing differs
            first = outs[("rows", None)]
            assert all(torch.equal(o, first) for (label, ml), o in outs.items() if ml is None)


@pytest.mark.parametrize("shape,impl", DECODE)
def test_decode_attention_rope_append(ops, shape, impl):
    """Rope mode: q is the raw fused row, RoPE on q and the new K, the new K / V appended at lens - 1 (poisoned
    before the launch) and attended.  Oracle on the rows the case says the launch leaves in the cache."""
    Hq, Hkv, D = shape
    name = f"decode-{Hq}-{Hkv}-{D}-rope"
    c = A.case(name, DEV)
    want = A.attend(c["rows"])
    for chunk in ((64, 128, 256) if impl == "valu" else (64, 128)):
        for label, k, v, kw in _decode_layouts(name, c, chunk):
            k, v = k.clone(), v.clone()
            out = ops.decode_attention(c["q"], k, v, c["lens"], Hq, Hkv, D, chunk=chunk, impl=impl,
                                       positions=c["positions"], cos=c["cos"], sin=c["sin"], **kw)
            _check(f"decode rope {impl} {shape} chunk {chunk} {label}", out, want, c["rows"], D)
            if label == "heads":  # the appended row, and nothing else, was written
                for b, r in enumerate(c["rows"]):
                    L = r.k.shape[0]
                    assert torch.equal(k[b, :, : L - 1], c["kc"][b, :, : L - 1])
                    assert torch.isnan(k[b, :, L:].float()).all() and torch.isnan(v[b, :, L:].float()).all()
                    assert torch.equal(v[b, :, L - 1].float(), r.v[L - 1])
                    new = k[b, :, L - 1].float()
                    assert ((new - r.k[L - 1]).abs() <= 2.0 ** -7 * r.k[L - 1].abs() + 1e-6).all()  # a bf16 ulp


@pytest.mark.parametrize("impl", ["valu", "mfma"])
def test_decode_attention_more_splits_than_lanes(ops, impl):
    """130 splits of 64 against the combine's D = 128 lanes (both of its passes in their strided form), B = 1."""
    c = A.case("decode-130-splits", DEV)
    want = R.decode_attention(c["q"], c["kc"].permute(0, 2, 1, 3), c["vc"].permute(0, 2, 1, 3), c["lens"], 4, 1, 128)
    out = ops.decode_attention(c["q"], c["kc"], c["vc"], c["lens"], 4, 1, 128, chunk=64, impl=impl, head_major=True)
    _check(f"decode {impl} 130 splits", out, want, c["rows"], 128)
    assert torch.equal(ops.decode_attention(c["q"], c["kc"], c["vc"], c["lens"], 4, 1, 128, chunk=64, impl=impl,
                                            head_major=True), out)


# ------------------------------------------------------------------ decode, e4m3 cache
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (8, 2), (16, 2)])
def test_decode_attention_fp8(ops, Hq, Hkv):
    D = 128
    name = f"decode8-{Hq}-{Hkv}-{D}"
    c = A.case(name, DEV)
    deq = lambda q8, s: R.kv_dequant_fp8(q8, s).permute(0, 2, 1, 3)  # noqa: E731
    want = R.decode_attention(c["q"], deq(c["kc"], c["ks"]), deq(c["vc"], c["vs"]), c["lens"], Hq, Hkv, D)
    cnt = torch.zeros(c["B"] * Hkv, device=DEV, dtype=torch.int32)
    for chunk in (64, 128):
        p = _paged(name, chunk)
        outs = []
        for label, caches, kw in (("per-slot", (c["kc"], c["vc"], c["ks"], c["vs"]), {}),
                                  ("paged", (p["kp"], p["vp"], p["ksp"], p["vsp"]), dict(page_table=p["table"]))):
            out = ops.decode_attention_fp8(c["q"], *caches, c["lens"], Hq, Hkv, D, chunk=chunk, counters=cnt, **kw)
            again = ops.decode_attention_fp8(c["q"], *caches, c["lens"], Hq, Hkv, D, chunk=chunk, counters=cnt, **kw)
            _check(f"decode fp8 ({Hq}, {Hkv}) chunk {chunk} {label}", out, want, c["rows"], D)
            assert torch.equal(again, out) and not cnt.any()
            outs.append(out)
        if chunk == 64:
            assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (8, 2), (16, 2)])
def test_decode_attention_fp8_rope_append(ops, Hq, Hkv):
    D = 128
    name = f"decode8-{Hq}-{Hkv}-{D}-rope"
    c = A.case(name, DEV)
    want = A.attend(c["rows"])
    for chunk in (64, 128):
        p = _paged(name, chunk)
        for label, caches, kw in (("per-slot", (c["kc"], c["vc"], c["ks"], c["vs"]), {}),
                                  ("paged", (p["kp"], p["vp"], p["ksp"], p["vsp"]), dict(page_table=p["table"]))):
            k8, v8, ks, vs = (t.clone() for t in caches)
            out = ops.decode_attention_fp8(c["q"], k8, v8, ks, vs, c["lens"], Hq, Hkv, D, chunk=chunk,
                                           positions=c["positions"], cos=c["cos"], sin=c["sin"], **kw)
            _check(f"decode fp8 rope ({Hq}, {Hkv}) chunk {chunk} {label}", out, want, c["rows"], D)
            if label == "per-slot":
                for b, r in enumerate(c["rows"]):
                    L = r.k.shape[0]
                    assert torch.equal(k8[b, :, : L - 1], c["kc"][b, :, : L - 1]) and (k8[b, :, L:] == A.NAN8).all()
                    assert torch.isnan(ks[b, :, L:]).all() and torch.isnan(vs[b, :, L:]).all()
                    assert torch.equal(R.kv_dequant_fp8(v8[b, :, L - 1], vs[b, :, L - 1]), r.v[L - 1])  # the writer's bytes
                    new = R.kv_dequant_fp8(k8[b, :, L - 1], ks[b, :, L - 1])
                    # a bf16 ulp of the rotated row may move an e4m3 code: one step, 2^-3 of the element
                    assert ((new - r.k[L - 1]).abs() <= 2.0 ** -3 * r.k[L - 1].abs() + ks[b, :, L - 1].unsqueeze(-1)).all()


# ------------------------------------------------------------------ verify
@pytest.mark.parametrize("Hq,Hkv,T", [(4, 1, 4), (8, 2, 4), (8, 1, 2), (4, 2, 8), (2, 2, 16)])
def test_decode_attention_multi(ops, Hq, Hkv, T):
    D = 128
    c = A.case(f"verify-{Hq}-{Hkv}-{T}", DEV)
    args = (c["past"], c["lens"], c["B"], T, Hq, Hkv, D)
    ref = R.attention_ctx(c["qkv"], c["kc"], c["vc"], *args, slot_ids=c["slot_ids"], head_major=True)
    want = A.valid_rows(ref, c["B"], T, c["n"])
    runs = {64: dict(chunk=64), 128: dict(chunk=128), "paged": dict(page_table=c["table"]),
            "bound": dict(max_len=int(c["lens"].max()))}
    outs = {}
    for label, kw in runs.items():
        k, v = (c["kp"], c["vp"]) if label == "paged" else (c["kc"], c["vc"])
        out = ops.decode_attention_multi(c["qkv"], k, v, *args, slot_ids=c["slot_ids"], **kw)
        again = ops.decode_attention_multi(c["qkv"], k, v, *args, slot_ids=c["slot_ids"], **kw)
        outs[label] = A.valid_rows(out, c["B"], T, c["n"])
        _check(f"verify ({Hq}, {Hkv}, T = {T}) {label}", outs[label], want, c["rows"], D)
        assert torch.equal(A.valid_rows(again, c["B"], T, c["n"]), outs[label])
    assert torch.equal(outs["paged"], outs[64]) and torch.equal(outs["bound"], outs[64])


# ------------------------------------------------------------------ ctx
@pytest.mark.parametrize("S", [1, 4, 64, 65, 130])
@pytest.mark.parametrize("fp8", [False, True])
def test_flash_attention_ctx(ops, S, fp8):
    Hq, Hkv, D = 8, 2, 128
    c = A.case(f"ctx{'8' if fp8 else ''}-{Hq}-{Hkv}-{S}", DEV)
    B = c["B"]
    args = (c["past"], c["lens"], B, S, Hq, Hkv, D)
    if fp8:
        ref = R.attention_ctx(c["qkv"], R.kv_dequant_fp8(c["kc"], c["ks"]), R.kv_dequant_fp8(c["vc"], c["vs"]), *args,
                              slot_ids=c["slot_ids"], head_major=True)
        op = ops.flash_attention_ctx_fp8
        images = {False: (c["kc"], c["vc"], c["ks"], c["vs"]), True: (c["kp"], c["vp"], c["ksp"], c["vsp"])}
    else:
        ref = R.attention_ctx(c["qkv"], c["kc"], c["vc"], *args, slot_ids=c["slot_ids"], head_major=True)
        op = ops.flash_attention_ctx
        images = {False: (c["kc"], c["vc"]), True: (c["kp"], c["vp"])}
    want = A.valid_rows(ref, B, S, c["n"])
    for splits in (1, 2, 4):  # the one-key row's later splits are empty
        kw = {}
        if splits > 1:
            ws = torch.full((ops.flash_ctx_workspace_elems(B, S, Hq, D, splits),), float("nan"), device=DEV)
            kw = dict(splits=splits, max_ctx=c["max_ctx"], workspace=ws)
        outs = []
        for paged in (False, True):
            out = torch.full((B * S, Hq * D), float("nan"), device=DEV, dtype=torch.bfloat16)
            run = lambda o: op(c["qkv"], *images[paged], *args, slot_ids=c["slot_ids"],  # noqa: E731
                               page_table=c["table"] if paged else None, out=o, **kw)
            run(out)
            again = run(torch.full_like(out, float("nan")))
            assert torch.isfinite(out.float()).all()  # padding rows included: zeros
            pad = torch.cat([out.view(B, S, -1)[b, int(c["n"][b]):] for b in range(B)])
            assert not pad.any()
            _check(f"ctx{' fp8' if fp8 else ''} S = {S} splits {splits} paged {paged}", A.valid_rows(out, B, S, c["n"]),
                   want, c["rows"], D)
            assert torch.equal(again, out)
            outs.append(out)
        assert torch.equal(outs[0], outs[1])  # the paged launch cuts the same tiles at the same boundaries


# ------------------------------------------------------------------ prefill
PREFILL = [f"prefill-causal-{S}" for S in (63, 64, 65, 130, 200)] + ["prefill-lens-130", "prefill64-lens-128",
                                                                     "prefill64-causal-100"]


@pytest.mark.parametrize("name", PREFILL)
@pytest.mark.parametrize("version", [1, 2])
def test_flash_attention(ops, name, version):
    c = A.case(name, DEV)
    B, S, Hq, Hkv, D = c["B"], c["S"], c["Hq"], c["Hkv"], c["D"]
    want = R.attention(c["qkv"], B, S, Hq, Hkv, D, kv_lens=c["kv_lens"], causal=c["causal"])
    lib = ops.lib()
    old = lib.mls_flash_set_version(version)
    try:
        out = ops.flash_attention(c["qkv"], B, S, Hq, Hkv, D, kv_lens=c["kv_lens"], causal=c["causal"])
        again = ops.flash_attention(c["qkv"], B, S, Hq, Hkv, D, kv_lens=c["kv_lens"], causal=c["causal"])
        torch.cuda.synchronize()
    finally:
        lib.mls_flash_set_version(old)
    _check(f"prefill v{version} {name}", out, want, c["rows"], D)
    assert torch.equal(again, out)


@pytest.mark.parametrize("q_rows", [1, 3, 16, 77])  # 1-wave, 4-wave and 8-wave launches
def test_flash_attention_rows(ops, q_rows):
    c = A.case("prefill64-lens-128", DEV)
    B, S, H, D = c["B"], c["S"], c["Hq"], c["D"]
    qkv = c["qkv"]
    want = R.attention(qkv, B, S, H, H, D, kv_lens=c["kv_lens"]).view(B, S, H * D)[:, :q_rows].reshape(B * q_rows, -1)
    idx = (torch.arange(B, device=DEV)[:, None] * S + torch.arange(q_rows, device=DEV)[None]).reshape(-1)
    wide = qkv[idx]  # [B*q_rows, 3HD]: q is its first H*D columns (row stride 3HD)
    kv = qkv[:, H * D:].contiguous()
    out = ops.flash_attention_rows(wide[:, : H * D], kv, B, S, q_rows, H, H, D, kv_lens=c["kv_lens"])
    assert out.shape == (B * q_rows, H * D)
    rows = A.rows_prefill(qkv, B, S, H, H, D, c["kv_lens"], False, q_rows=q_rows)
    _check(f"prefill rows q_rows {q_rows}", out, want, rows, D)
