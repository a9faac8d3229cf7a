"""Split-KV context attention on the GPU (ops/csrc/flash_ctx.hip ``mls_flash_attention_ctx_split`` + its
combine, ``ops.flash_attention_ctx(splits=...)``): few queries against a long cached context, the shape a
prefix-cache hit produces.  Cases as ``test_flash_ctx_gpu.py`` builds them (ragged ``past``, shuffled
slots, a shuffled page pool with the same rows, NaN wherever a launch must not read), against the fp32
oracle ``ops.reference.attention_ctx`` and against the unsplit kernel.

Tolerance: 2e-2 of the largest output magnitude, the unsplit kernel's bound (P is rounded to bf16 before
the PV product; the fp32 merge of the partials adds nothing of that order).  The split and the unsplit
outputs are not expected to be equal: the summation order differs."""
import pytest
import torch

import attn_cases as A
from mlmicroservicetemplate_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
MAX_SEQ = 333  # not a multiple of the 64-key tile: 6 tiles, the last ends inside a slot's rows
PASTS = [0, 1, 63, 64, 65, 200]  # ragged within one batch; 200 + 65 <= MAX_SEQ


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@pytest.fixture(scope="module")
def ops():
    from mlmicroservicetemplate_amd import ops as o

    o.lib()
    return o


def _valid_counts(S, B):
    """Valid queries per batch row: full chunks and chunks that end inside a tile."""
    return [S, max(1, S - 1), max(1, S // 2), S, max(1, S - 7), S][:B]


def _case(Hq, Hkv, S, seed=0, pasts=PASTS, max_seq=MAX_SEQ, slot_ids=(7, 2, 8, 0, 5, 3)):
    """qkv of the chunk (its K / V columns poisoned: the kernel reads K / V from the cache only), a
    per-slot head-major cache and the same rows in a shuffled page pool; everything a launch must not
    read (unused slots, rows >= lens, the tail of a slot's last page) is NaN."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = len(pasts)
    past = torch.tensor(pasts, dtype=torch.int32, device=DEV)
    n = torch.tensor(_valid_counts(S, B), dtype=torch.int32, device=DEV)
    lens = past + n
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    qkv[:, Hq * D:] = float("nan")
    n_slots = B + 3
    slot_ids = torch.tensor(list(slot_ids[:B]), dtype=torch.int32, device=DEV)  # some slots stay unused
    kc = torch.full((n_slots, Hkv, max_seq, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    vc = torch.full_like(kc, float("nan"))
    for b in range(B):
        L, s = int(lens[b]), int(slot_ids[b])
        kc[s, :, :L] = torch.randn(Hkv, L, D, device=DEV, generator=g).to(torch.bfloat16)
        vc[s, :, :L] = torch.randn(Hkv, L, D, device=DEV, generator=g).to(torch.bfloat16)
    pps = -(-max_seq // 64)
    pages = n_slots * pps + 1
    table = (1 + torch.randperm(pages - 1, device=DEV, generator=g)).view(n_slots, pps).to(torch.int32)
    kp = torch.full((pages, Hkv, 64, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    vp = torch.full_like(kp, float("nan"))
    flat = table.long().flatten()
    pad = pps * 64 - max_seq
    for src, dst in ((kc, kp), (vc, vp)):
        rows = torch.nn.functional.pad(src, (0, 0, 0, pad), value=float("nan"))  # [slots, Hkv, pps*64, D]
        dst[flat] = rows.view(n_slots, Hkv, pps, 64, D).permute(0, 2, 1, 3, 4).reshape(n_slots * pps, Hkv, 64, D)
    ref = R.attention_ctx(qkv, kc, vc, past, lens, B, S, Hq, Hkv, D, slot_ids=slot_ids, head_major=True)
    # per (row, head) bound: 4 x the rounding model on these inputs (tests/attn_cases.py)
    tol = A.tolerance(A.rows_ctx(qkv, kc, vc, past, lens, B, S, Hq, Hkv, D, slot_ids), D)
    return dict(B=B, S=S, Hq=Hq, Hkv=Hkv, past=past, n=n, lens=lens, qkv=qkv, slot_ids=slot_ids, kc=kc, vc=vc,
                table=table, kp=kp, vp=vp, ref=ref, max_ctx=int(lens.max()), tol=tol)


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


def _run(ops, c, paged, **kw):
    k, v = (c["kp"], c["vp"]) if paged else (c["kc"], c["vc"])
    return ops.flash_attention_ctx(c["qkv"], k, v, c["past"], c["lens"], c["B"], c["S"], c["Hq"], c["Hkv"], D,
                                   slot_ids=c["slot_ids"], page_table=c["table"] if paged else None, **kw)


def _check_split(ops, c, splits):
    B, S, Hq = c["B"], c["S"], c["Hq"]
    need = ops.flash_ctx_workspace_elems(B, S, Hq, D, splits)
    ws = torch.zeros(need, device=DEV, dtype=torch.float32)
    out = torch.full((B * S, Hq * D), float("nan"), device=DEV, dtype=torch.bfloat16)
    ret = _run(ops, c, False, splits=splits, max_ctx=c["max_ctx"], workspace=ws, out=out)
    assert ret.data_ptr() == out.data_ptr()
    unsplit = _run(ops, c, False)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()  # finite everywhere: no poisoned row or column was read
    got, want = _valid(out, c), _valid(c["ref"], c)
    err, err_u = rel(got, want), rel(got, _valid(unsplit, c))
    print(f"Hq={Hq} S={S} splits={splits}: rel vs oracle {err:.4f}, vs the unsplit kernel {err_u:.4f}")
    assert err < 2e-2
    assert err_u < 2e-2
    assert A.head_err(got, want, D).max() < c["tol"]
    assert A.head_err(got, _valid(unsplit, c), D).max() < 2 * c["tol"]  # two kernels, each within tol of the oracle
    assert not _padding(out, c).any()  # rows q >= n are zeros
    # layout invariance: the paged launch cuts the same tiles at the same boundaries
    out_p = _run(ops, c, True, splits=splits, max_ctx=c["max_ctx"], workspace=ws)
    assert torch.equal(out_p, out)
    # reproducible, and nothing is read before it is written: same workspace again, then one full of NaN
    again = _run(ops, c, False, splits=splits, max_ctx=c["max_ctx"], workspace=ws)
    assert torch.equal(again, out)
    ws.fill_(float("nan"))
    poisoned = _run(ops, c, False, splits=splits, max_ctx=c["max_ctx"], workspace=ws)
    assert torch.equal(poisoned, out)
    assert torch.equal(_run(ops, c, False, splits=splits, max_ctx=c["max_ctx"]), out)  # its own workspace


@pytest.mark.parametrize("splits", [2, 3, 8])  # 8 splits over <= 6 tiles: empty splits
@pytest.mark.parametrize("S", [1, 16, 63, 64, 65])
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (8, 2)])
def test_split_vs_oracle_unsplit_and_layouts(ops, Hq, Hkv, S, splits):
    _check_split(ops, _shared_case(Hq, Hkv, S), splits)


@pytest.mark.parametrize("splits", [4, 16])
def test_deeper_context_several_tiles_per_split(ops, splits):
    """18 key tiles: several per split, a ragged batch (the short row's late splits are empty)."""
    key = ("deep",)
    if key not in _CASES:
        _CASES[key] = _case(8, 2, 5, seed=3, pasts=[1000, 37], max_seq=1100, slot_ids=(3, 1))
    c = _CASES[key]
    assert c["lens"].tolist() == [1005, 41]
    _check_split(ops, c, splits)


def test_max_ctx_above_the_longest_row_cuts_elsewhere_same_result(ops):
    """The bound only has to cover lens: a looser one moves the cuts, not the answer."""
    c = _shared_case(8, 2, 16)
    tight = _run(ops, c, True, splits=4, max_ctx=c["max_ctx"])  # 216 rows: 4 tiles, one per split
    loose = _run(ops, c, True, splits=4, max_ctx=MAX_SEQ + 500)  # clamped to a slot's 6 pages: two per split
    assert rel(_valid(loose, c), _valid(tight, c)) < 2e-2
    assert A.head_err(_valid(loose, c), _valid(tight, c), D).max() < 2 * c["tol"]


def test_refusals_before_launch(ops):
    c = _shared_case(4, 1, 16)
    out = torch.full((c["B"] * c["S"], c["Hq"] * D), 7.0, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="splits"):
        _run(ops, c, False, splits=0, out=out)
    with pytest.raises(ValueError, match="splits"):
        _run(ops, c, False, splits=65, max_ctx=c["max_ctx"], out=out)
    with pytest.raises(ValueError, match="max_ctx"):
        _run(ops, c, False, splits=2, out=out)
    small = torch.zeros(ops.flash_ctx_workspace_elems(c["B"], c["S"], c["Hq"], D, 2) - 1, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        _run(ops, c, False, splits=2, max_ctx=c["max_ctx"], workspace=small, out=out)
    rm = c["kc"].transpose(1, 2).contiguous()  # the unsplit path's geometry refusals hold here too
    with pytest.raises(ValueError, match="head-major"):
        ops.flash_attention_ctx(c["qkv"], rm, rm, c["past"], c["lens"], c["B"], c["S"], c["Hq"], c["Hkv"], D,
                                slot_ids=c["slot_ids"], splits=2, max_ctx=c["max_ctx"], out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()  # nothing was launched
    # the host entry refuses the same itself
    lib = ops.lib()
    ws = torch.zeros(ops.flash_ctx_workspace_elems(c["B"], c["S"], c["Hq"], D, 2), device=DEV)

    def entry(nsplit, max_ctx, ws_elems):
        return lib.mls_flash_attention_ctx_split(
            c["qkv"].data_ptr(), c["kc"].data_ptr(), c["vc"].data_ptr(), out.data_ptr(), ws.data_ptr(), ws_elems,
            c["qkv"].shape[1], out.stride(0), c["past"].data_ptr(), c["lens"].data_ptr(), c["slot_ids"].data_ptr(),
            None, 0, c["kc"].shape[0], c["B"], c["S"], c["Hq"], c["Hkv"], D, c["kc"].shape[0], MAX_SEQ, max_ctx,
            nsplit, 1.0, ops.stream_ptr(torch.device(DEV)))

    BAD_ARG = 1001
    assert entry(0, c["max_ctx"], ws.numel()) == BAD_ARG
    assert entry(65, c["max_ctx"], ws.numel()) == BAD_ARG
    assert entry(2, 0, ws.numel()) == BAD_ARG
    assert entry(2, c["max_ctx"], ws.numel() - 1) == BAD_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all()
