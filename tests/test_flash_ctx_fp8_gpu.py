"""Context attention on the e4m3 KV cache (ops/csrc/flash_ctx.hip ``flash_ctx_kernel<true, SPLIT>``,
``ops.flash_attention_ctx_fp8``): the chunk path of ``kv_prefill="cache"``, unsplit and split-KV, per-slot
and paged.  Cases as ``test_flash_ctx_split_gpu.py::_case`` builds them (ragged ``past``, shuffled slots,
a shuffled page pool holding the same rows); the cache rows are ``R.kv_quant_fp8`` of random bf16 rows and
everything a launch must not read -- unused slots, rows >= lens, the tail of a slot's last page, the K / V
columns of qkv -- is poisoned: bytes 0x7F (the e4m3 NaN) and NaN scales.

Oracle: ``R.attention_ctx`` on ``R.kv_dequant_fp8`` of the same bytes, so the test measures the kernel and
not the quantiser.  Bound: 2e-2 of the largest output magnitude, the bound ``test_flash_ctx_split_gpu.py``
applies to this tile (P is rounded to bf16 before the PV product; the kernel's bf16 rounding of
``e4m3 * scale``, 2^-9 relative per element, is below it)."""
import os
import subprocess
import sys

import pytest
import torch

import attn_cases as A
from mlmicroservicetemplate_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
MAX_SEQ = 333  # not a multiple of the 64-key tile: 6 tiles, the last ends inside a slot's rows
PASTS = [0, 1, 63, 64, 65, 200]  # ragged within one batch; 200 + 65 <= MAX_SEQ
BOUND = 2e-2
NAN8 = 0x7F


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@pytest.fixture(scope="module")
def ops():
    from mlmicroservicetemplate_amd import ops as o

    o.lib()
    return o


def _valid_counts(S, B):
    return [S, max(1, S - 1), max(1, S // 2), S, max(1, S - 7), S][:B]


def _case(Hq, Hkv, S, seed=0, pasts=PASTS, max_seq=MAX_SEQ, slot_ids=(7, 2, 8, 0, 5, 3)):
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = len(pasts)
    past = torch.tensor(pasts, dtype=torch.int32, device=DEV)
    n = torch.tensor(_valid_counts(S, B), dtype=torch.int32, device=DEV)
    lens = past + n
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    qkv[:, Hq * D:] = float("nan")
    n_slots = B + 3
    slot_ids = torch.tensor(list(slot_ids[:B]), dtype=torch.int32, device=DEV)  # some slots stay unused
    kc = torch.full((n_slots, Hkv, max_seq, D), NAN8, device=DEV, dtype=torch.uint8)
    vc = torch.full_like(kc, NAN8)
    ks = torch.full((n_slots, Hkv, max_seq), float("nan"), device=DEV, dtype=torch.float32)
    vs = torch.full_like(ks, float("nan"))
    for b in range(B):
        L, s = int(lens[b]), int(slot_ids[b])
        for c8, sc in ((kc, ks), (vc, vs)):
            # rows of different magnitude, so the per-row scales matter
            rows = torch.randn(Hkv, L, D, device=DEV, generator=g) * (0.25 + 2 * torch.rand(Hkv, L, 1, device=DEV, generator=g))
            c8[s, :, :L], sc[s, :, :L] = R.kv_quant_fp8(rows.to(torch.bfloat16))
    pps = -(-max_seq // 64)
    pages = n_slots * pps + 1
    table = (1 + torch.randperm(pages - 1, device=DEV, generator=g)).view(n_slots, pps).to(torch.int32)
    flat = table.long().flatten()
    pad = pps * 64 - max_seq
    kp = torch.full((pages, Hkv, 64, D), NAN8, device=DEV, dtype=torch.uint8)
    vp = torch.full_like(kp, NAN8)
    ksp = torch.full((pages, Hkv, 64), float("nan"), device=DEV, dtype=torch.float32)
    vsp = torch.full_like(ksp, float("nan"))
    for src, dst in ((kc, kp), (vc, vp)):
        rows = torch.nn.functional.pad(src, (0, 0, 0, pad), value=NAN8)  # [slots, Hkv, pps*64, D]
        dst[flat] = rows.view(n_slots, Hkv, pps, 64, D).permute(0, 2, 1, 3, 4).reshape(n_slots * pps, Hkv, 64, D)
    for src, dst in ((ks, ksp), (vs, vsp)):
        rows = torch.nn.functional.pad(src, (0, pad), value=float("nan"))
        dst[flat] = rows.view(n_slots, Hkv, pps, 64).permute(0, 2, 1, 3).reshape(n_slots * pps, Hkv, 64)
    ref = R.attention_ctx(qkv, R.kv_dequant_fp8(kc, ks), R.kv_dequant_fp8(vc, vs), past, lens, B, S, Hq, Hkv, D,
                          slot_ids=slot_ids, head_major=True)
    assert torch.isfinite(ref).all()
    # per (row, head) bound: 4 x the rounding model on the dequantised rows (tests/attn_cases.py)
    tol = A.tolerance(A.rows_ctx(qkv, R.kv_dequant_fp8(kc, ks), R.kv_dequant_fp8(vc, vs), past, lens, B, S, Hq, Hkv, D,
                                 slot_ids), D)
    return dict(tol=tol, B=B, S=S, Hq=Hq, Hkv=Hkv, past=past, n=n, lens=lens, qkv=qkv, slot_ids=slot_ids, kc=kc, vc=vc,
                ks=ks, vs=vs, table=table, kp=kp, vp=vp, ksp=ksp, vsp=vsp, ref=ref, max_ctx=int(lens.max()))


_CASES = {}


def _shared_case(Hq, Hkv, S):
    """One case (and its oracle output) per shape, shared by the split counts; never modified."""
    key = (Hq, Hkv, S)
    if key not in _CASES:
        _CASES[key] = _case(Hq, Hkv, S)
    return _CASES[key]


def _valid(out, c):
    o = out.view(c["B"], c["S"], -1)
    return torch.cat([o[b, : int(c["n"][b])] for b in range(c["B"])])


def _padding(out, c):
    o = out.view(c["B"], c["S"], -1)
    return torch.cat([o[b, int(c["n"][b]):] for b in range(c["B"])])


def _run(ops, c, paged, past=None, lens=None, **kw):
    caches = (c["kp"], c["vp"], c["ksp"], c["vsp"]) if paged else (c["kc"], c["vc"], c["ks"], c["vs"])
    return ops.flash_attention_ctx_fp8(c["qkv"], *caches, c["past"] if past is None else past,
                                       c["lens"] if lens is None else lens, c["B"], c["S"], c["Hq"], c["Hkv"], D,
                                       slot_ids=c["slot_ids"], page_table=c["table"] if paged else None, **kw)


@pytest.mark.parametrize("S", [1, 4, 64, 65])  # a verify step, one query tile, a second tile of one query
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (4, 4), (8, 1)])
def test_fp8_ctx_vs_oracle(ops, Hq, Hkv, S):
    """Splits 1 (the unsplit launch), 2, 4 and 8 (more than the 5 key tiles: empty splits), per-slot and paged."""
    c = _shared_case(Hq, Hkv, S)
    B = c["B"]
    want = _valid(c["ref"], c)
    for splits in (1, 2, 4, 8):
        kw = {}
        if splits > 1:
            ws = torch.full((ops.flash_ctx_workspace_elems(B, S, Hq, D, splits),), float("nan"), device=DEV)
            kw = dict(splits=splits, max_ctx=c["max_ctx"], workspace=ws)
        for paged in (False, True):
            out = torch.full((B * S, Hq * D), float("nan"), device=DEV, dtype=torch.bfloat16)
            ret = _run(ops, c, paged, out=out, **kw)
            torch.cuda.synchronize()
            assert ret.data_ptr() == out.data_ptr()
            assert torch.isfinite(out.float()).all()  # no poisoned byte, scale or column was read
            err = rel(_valid(out, c), want)
            print(f"Hq={Hq} Hkv={Hkv} S={S} splits={splits} paged={paged}: rel vs oracle {err:.5f}")
            assert err < BOUND
            assert A.head_err(_valid(out, c), want, D).max() < c["tol"]
            assert not _padding(out, c).any()  # rows q >= n are zeros


def test_graph_replay_follows_past_and_lens(ops):
    """past / lens are device arrays: one captured launch per route, replayed after they change."""
    c = _shared_case(8, 2, 4)
    B, S, Hq = c["B"], c["S"], c["Hq"]
    past, lens = c["past"].clone(), c["lens"].clone()
    ws = torch.zeros(ops.flash_ctx_workspace_elems(B, S, Hq, D, 2), device=DEV)
    outs = [torch.zeros(B * S, Hq * D, device=DEV, dtype=torch.bfloat16) for _ in range(2)]
    kws = [dict(out=outs[0]), dict(out=outs[1], splits=2, max_ctx=MAX_SEQ, workspace=ws)]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for kw in kws:
            _run(ops, c, True, past=past, lens=lens, **kw)
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for kw in kws:
            _run(ops, c, True, past=past, lens=lens, **kw)
    # the recorded contexts, then each row two keys shorter with one query fewer where it has two
    n2 = (c["n"] - 1).clamp(min=1)
    p2 = (c["past"] - 2).clamp(min=0)
    for pa, ln in ((c["past"], c["lens"]), (p2, p2 + n2)):
        past.copy_(pa)
        lens.copy_(ln)
        g.replay()
        torch.cuda.synchronize()
        eager = _run(ops, c, True, past=pa.clone(), lens=ln.clone())
        ref = R.attention_ctx(c["qkv"], R.kv_dequant_fp8(c["kc"], c["ks"]), R.kv_dequant_fp8(c["vc"], c["vs"]), pa, ln,
                              B, S, Hq, c["Hkv"], D, slot_ids=c["slot_ids"], head_major=True)
        assert torch.equal(outs[0], eager)
        cur = dict(c, n=ln - pa)
        tol = A.tolerance(A.rows_ctx(c["qkv"], R.kv_dequant_fp8(c["kc"], c["ks"]), R.kv_dequant_fp8(c["vc"], c["vs"]),
                                     pa, ln, B, S, Hq, c["Hkv"], D, c["slot_ids"]), D)
        for o in outs:
            assert torch.isfinite(o.float()).all()
            assert rel(_valid(o, cur), _valid(ref, cur)) < BOUND
            assert A.head_err(_valid(o, cur), _valid(ref, cur), D).max() < tol
            assert not _padding(o, cur).any()


def test_refusals_before_launch(ops):
    c = _shared_case(8, 2, 4)
    out = torch.full((c["B"] * c["S"], c["Hq"] * D), 7.0, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="splits"):
        _run(ops, c, False, splits=65, max_ctx=c["max_ctx"], out=out)
    with pytest.raises(ValueError, match="max_ctx"):
        _run(ops, c, False, splits=2, out=out)
    with pytest.raises(TypeError, match="k_cache"):  # bf16 caches are the other op's
        ops.flash_attention_ctx_fp8(c["qkv"], c["kc"].to(torch.bfloat16), c["vc"].to(torch.bfloat16), c["ks"], c["vs"],
                                    c["past"], c["lens"], c["B"], c["S"], c["Hq"], c["Hkv"], D, out=out)
    with pytest.raises(ValueError, match="scale"):
        ops.flash_attention_ctx_fp8(c["qkv"], c["kc"], c["vc"], c["ks"][:, :, :-1], c["vs"], c["past"], c["lens"],
                                    c["B"], c["S"], c["Hq"], c["Hkv"], D, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()  # nothing was launched


def test_debug_build_reports_a_bad_page_id():
    """The -DMLS_DEBUG build reports a page id outside the pool as NativeError instead of reading it
    (tests/flash_ctx_fp8_debug_probe.py, a child process as test_flash_ctx_gpu.py starts its probe: the
    library variant is chosen at import)."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, MLS_DEBUG="1", HIP_LAUNCH_BLOCKING="1",
               PYTHONPATH=os.pathsep.join([root, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.join(here, "flash_ctx_fp8_debug_probe.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FLASH-CTX-FP8-DEBUG-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
