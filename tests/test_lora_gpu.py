"""``ops.lora_qkv_`` (csrc/lora.hip: mls_lora_shrink + mls_lora_expand) against ``ops.lora_reference`` under the
per-element bound of tests/lora_cases.py, on its inputs: every rank set x K x row shape of the issue, at every
split count the host rule can return and at forced ones.  Every call gets a NaN-filled workspace and a pack
whose unnamed adapter slot is NaN-filled; base rows must come back bit-identical and repeats bit-identical."""
import functools

import pytest
import torch

import lora_cases as L
from mlmicroservicetemplate_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPARE = L.N_ADAPTERS  # an adapter slot no lora_slot entry names: NaN-filled


@functools.lru_cache(maxsize=None)
def _case(K, ranks, rows):
    c = L.Case(K, ranks, rows)
    ref = c.reference()
    return c, ref, c.bound(ref)


def _pack(c, layers=1, layer=0):
    pack = ops.pack_lora(layers, c.K, L.WIDTHS, L.N_ADAPTERS + 1, max(c.ranks), DEV)
    for a, ad in enumerate(c.adapters):
        tensors = {}
        for p, (A, Bm, s) in ad.items():
            tensors[f"l{layer}.{p}.lora_A"], tensors[f"l{layer}.{p}.lora_B"] = A, Bm
            for i in range(layers):
                if i != layer:  # the other layers of the pack: other content, never read
                    tensors[f"l{i}.{p}.lora_A"], tensors[f"l{i}.{p}.lora_B"] = A * 3, Bm * -2
        pack.load(a, tensors, {p: s for p, (_, _, s) in ad.items()}, gains=[c.gain] * layers)
    pack.A[:, SPARE] = float("nan")
    pack.B[:, SPARE] = float("nan")
    return pack


def _splits(c, pack):
    auto = ops.lora_split(c.B, c.S, c.K, pack.rcap)
    forced = [s for s in (1, 2, 4, 8, 16, 32) if c.K % (s * ops.LORA_K_GRAN) == 0]
    assert auto in forced
    return auto, forced


def _run(c, pack, nsplit, layer=0):
    qkv = c.qkv.to(DEV, torch.bfloat16)
    x = c.x.to(DEV, torch.bfloat16)
    ns = nsplit or ops.lora_split(c.B, c.S, c.K, pack.rcap)
    ws = torch.full((pack.workspace_elems(c.B * c.S, ns),), float("nan"), device=DEV)  # exactly what the call needs
    sid = None if c.slot_ids is None else c.slot_ids.to(DEV)
    out = ops.lora_qkv_(qkv, x, pack, layer, c.lora_slot.to(DEV), c.B, c.S, sid, eps=L.EPS, workspace=ws,
                        nsplit=nsplit)
    assert out is qkv
    return out.float().cpu()


def _check(c, ref, bound, got, what):
    assert torch.isfinite(got).all(), what
    for b in range(c.B):
        if c.adapter_of(b) < 0:
            sl = slice(b * c.S, (b + 1) * c.S)
            assert torch.equal(got[sl], c.qkv[sl]), f"{what}: base rows of sequence {b} changed"
    w = L.worst(got, ref, bound)
    print(f"{what}: {w:.3f} of the bound")
    assert w <= 1.0, what


@pytest.mark.parametrize("rows", sorted(L.ROWS))
@pytest.mark.parametrize("ranks", L.RANKS)
@pytest.mark.parametrize("K", [256, 4096])
def test_kernel_matches_reference(K, ranks, rows):
    c, ref, bound = _case(K, ranks, rows)
    pack = _pack(c)
    auto, forced = _splits(c, pack)
    first = _run(c, pack, 0)
    _check(c, ref, bound, first, f"K={K} ranks={ranks} {rows} auto split {auto}")
    assert torch.equal(_run(c, pack, auto), first)  # nsplit = 0 is the host rule, and repeats are bit-identical
    for s in forced:
        _check(c, ref, bound, _run(c, pack, s), f"K={K} ranks={ranks} {rows} split {s}")


@pytest.mark.parametrize("ranks", [(16, 16, 16), (4, 0, 12)])
@pytest.mark.parametrize("K", [256, 4096])
def test_plain_fp32_adapter_through_the_load_path(K, ranks):
    """A drawn in plain fp32: ``LoraPack.load``'s ``bf16(A diag(gain))`` rounds for real.  Judged under the bound
    plus the worst case of that quantisation (``Case.bound(a_quant=True)``)."""
    c = L.Case(K, ranks, "2x17_slot_ids", generic_a=True)
    ref = c.reference()
    bound = c.bound(ref, a_quant=True)
    pack = _pack(c)
    for s in (0, 1, 2):
        _check(c, ref, bound, _run(c, pack, s), f"plain fp32 A, K={K} ranks={ranks} split {s}")


def test_host_rule_reaches_every_split():
    """The split counts the host rule returns over the row shapes a server runs (K = 4096, rank 16)."""
    seen = {ops.lora_split(B, S, 4096, 48) for B, S in ((1, 1), (8, 1), (32, 1), (64, 1), (128, 1), (8, 512))}
    assert seen == {16, 8, 4, 2, 1}
    assert ops.lora_split(1, 1, 256, 48) == 1  # a slice is at least 256 wide
    for B, S in ((1, 1), (3, 1), (2, 17), (4, 1), (3, 17)):  # the shapes of test_kernel_matches_reference
        assert ops.lora_split(B, S, 4096, 48) == 16 and ops.lora_split(B, S, 4096, 192) in (8, 16)


def test_second_layer_of_a_pack():
    c, ref, bound = _case(256, (16, 16, 16), "2x17_slot_ids")
    pack = _pack(c, layers=2, layer=1)
    _check(c, ref, bound, _run(c, pack, 2, layer=1), "layer 1 of 2")


def test_reload_in_place_keeps_addresses():
    c, ref, bound = _case(256, (8, 0, 16), "3x1_mixed")
    pack = _pack(c)
    ptrs = (pack.A.data_ptr(), pack.B.data_ptr(), pack.seg.data_ptr(), pack.scale.data_ptr())
    ad = c.adapters[2]
    pack.load(0, {f"l0.{p}.lora_{n}": t for p, v in ad.items() for n, t in (("A", v[0]), ("B", v[1]))},
              {p: v[2] for p, v in ad.items()}, gains=[c.gain])
    assert ptrs == (pack.A.data_ptr(), pack.B.data_ptr(), pack.seg.data_ptr(), pack.scale.data_ptr())
    c2 = L.Case(256, (8, 0, 16), "3x1_mixed")
    c2.adapters[0] = ad
    ref2 = c2.reference()
    _check(c2, ref2, c2.bound(ref2), _run(c, pack, 0), "adapter 0 replaced by adapter 2's tensors")


def test_graph_replay_reads_lora_slot_in_place():
    c, _, _ = _case(4096, (16, 16, 16), "3x1_mixed")
    pack = _pack(c)
    base = c.qkv.to(DEV, torch.bfloat16)
    x = c.x.to(DEV, torch.bfloat16)
    qkv = base.clone()
    slot = c.lora_slot.to(DEV)
    ws = torch.full((pack.workspace_elems(c.B, 16),), float("nan"), device=DEV)

    def run():
        qkv.copy_(base)
        ops.lora_qkv_(qkv, x, pack, 0, slot, c.B, c.S, eps=L.EPS, workspace=ws)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for slots in ([1, -1, 0], [-1, 2, 2], [-1, -1, -1], [0, 1, 2]):
        slot.copy_(torch.tensor(slots, dtype=torch.int32))
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        c2 = L.Case(4096, (16, 16, 16), "3x1_mixed")
        c2.lora_slot = torch.tensor(slots, dtype=torch.int32)
        ref = c2.reference()
        _check(c2, ref, c2.bound(ref), qkv.float().cpu(), f"replay with lora_slot {slots}")


def test_host_side_refusals():
    with pytest.raises(ValueError, match="max_rank"):
        ops.pack_lora(1, 256, L.WIDTHS, 2, 65, DEV)
    with pytest.raises(ValueError, match="max_rank"):
        ops.pack_lora(1, 256, L.WIDTHS, 2, 0, DEV)
    with pytest.raises(ValueError, match="K granule"):
        ops.pack_lora(1, 192, L.WIDTHS, 2, 16, DEV)
    with pytest.raises(ValueError, match="multiples of 16"):
        ops.pack_lora(1, 256, (1024, 200, 256), 2, 16, DEV)
    c, _, _ = _case(256, (16, 16, 16), "2x17")
    pack = ops.pack_lora(1, 256, L.WIDTHS, 2, 16, DEV)
    A, Bm, s = c.adapters[0]["q"]
    with pytest.raises(ValueError, match="rank 17"):
        pack.load(0, {"l0.q.lora_A": torch.zeros(17, 256), "l0.q.lora_B": torch.zeros(1024, 17)}, {"q": 1.0})
    with pytest.raises(ValueError, match="expected"):
        pack.load(0, {"l0.q.lora_A": A, "l0.q.lora_B": Bm[:512]}, {"q": s})  # mismatched segment width
    with pytest.raises(ValueError, match="subset"):
        pack.load(0, {"l0.o.lora_A": A, "l0.o.lora_B": Bm}, {"o": s})
    with pytest.raises(ValueError, match="index"):
        pack.load(2, {"l0.q.lora_A": A, "l0.q.lora_B": Bm}, {"q": s})
    pack.load(0, {"l0.q.lora_A": A, "l0.q.lora_B": Bm}, {"q": s})
    qkv = c.qkv.to(DEV, torch.bfloat16)
    x = c.x.to(DEV, torch.bfloat16)
    slot = torch.tensor([0, -1], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        ops.lora_qkv_(qkv, x, pack, 0, slot, c.B, c.S, workspace=torch.empty(16, device=DEV))
    with pytest.raises(ValueError, match="segment widths"):
        ops.lora_qkv_(qkv[:, :1024].contiguous(), x, pack, 0, slot, c.B, c.S)
    with pytest.raises(ValueError, match="nsplit"):
        ops.lora_qkv_(qkv, x, pack, 0, slot, c.B, c.S, nsplit=4)
    with pytest.raises(ValueError, match="slots"):
        ops.lora_qkv_(qkv, x, pack, 0, slot[:1], c.B, c.S)
    assert torch.equal(qkv.float().cpu(), c.qkv)  # nothing was launched
