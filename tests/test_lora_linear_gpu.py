"""csrc/lora_linear.hip (``ops.lora_tiles`` + ``ops.lora_linear_`` / ``ops.lora_gate_up``) against the fp32 oracles
``ops.reference.lora_linear`` / ``lora_gate_up`` on bf16-valued inputs drawn as tests/lora_cases.py draws them.

Bounds, per element, derived (U = 2^-9, half a bf16 ulp; factor 4 as in lora_cases):
  add form   ``4 U (|ref| + s sum_j |t_j B_nj|)``: the final bf16 rounding plus t rounded to bf16 before the expand.
  SiLU form  with ``E_g``, ``E_u`` the second term alone for the two pre-activations (the kernel keeps them in fp32):
             ``1.1 |u| E_g + |silu(g)| E_u + 1.1 E_g E_u + 4 U |ref|`` -- |silu'| <= 1.1.
Every call gets a NaN-filled workspace, a NaN-filled spare adapter slot and a NaN-patterned tile table."""
import functools

import pytest
import torch
import torch.nn.functional as F

from lora_cases import U, _bf, worst
from mlmicroservicetemplate_amd import ops
from mlmicroservicetemplate_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV, EPS = "cuda:0", 1e-5
N_AD = 4  # adapters 0, 1, 2 loaded, 2 without the module(s) under test; 3 is never loaded: NaN-filled
NAN_BITS = 0x7FC00000
ROWS = {  # B, S, lora_slot, slot_ids
    "1x1": (1, 1, [0], None),
    "5x1": (5, 1, [0, 1, 0, -1, 0], None),           # grouping gathers non-adjacent rows
    "18x1": (18, 1, [1] * 18, None),                 # tiles of 16 + 2
    "2x17": (2, 17, [1, -1, 0], [2, 0]),             # two tiles per sequence, the second with one row
    "4x1_base": (4, 1, [-1] * 4, None),              # no tile
    "3x1_absent": (3, 1, [2, 0, 2], None),           # rows on an adapter that lacks the module
}
SHAPES = [(256, 48), (256, 80), (1792, 48), (1792, 80)]  # K: 1 slice / 14 granules; N: a partial block / 1 + partial
FORMS = {"plain": (("o",), False), "normed": (("o",), True), "silu": (("gate", "up"), True)}  # N = 2 I for silu


class Case:
    def __init__(self, K, N, rank, rows, mods, normed):
        """``mods``: under test, N columns each; adapter 1 holds only the first, adapter 2 only the unlaunched down."""
        self.B, self.S, slots, sid = ROWS[rows]
        self.mods, M = mods, self.B * self.S
        g = torch.Generator().manual_seed(K + N + rank)
        self.slots, self.sid = torch.tensor(slots, dtype=torch.int32), sid and torch.tensor(sid, dtype=torch.int32)
        self.x = _bf(torch.randn(M, K, generator=g) * 2.0)
        self.y = _bf(torch.randn(M, N * len(mods), generator=g))
        self.gain = torch.exp((torch.rand(K, generator=g) * 2 - 1) * 1.0986) if normed else None
        self.adapters = []
        for a in range(3):
            ad = {}
            for p in (mods, mods[:1], ("down",))[a]:
                A = torch.randn(rank, K, generator=g) / K ** 0.5
                A = _bf(A * self.gain) / self.gain if normed else _bf(A)
                n = N * len(mods) if p == "down" else N
                ad[p] = (A, _bf(torch.randn(n, rank, generator=g) * (0.5 + 0.5 * a) / rank ** 0.5), R.lora_scale(6.0, rank))
            self.adapters.append(ad)
        self.rows = (self.slots, self.B, self.S, self.sid)

    def terms(self, p):
        """Module p's pre-activation by the fp32 oracle, and ``4 U s sum_j |t_j B_nj|`` (zero on the rows without p)."""
        ads = [ad.get(p) for ad in self.adapters]
        n = ads[0][1].shape[0]
        y = self.y[:, self.mods.index(p) * n: (self.mods.index(p) + 1) * n]
        x, mag = self.x, torch.zeros_like(y)
        if self.gain is not None:
            x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * self.gain
        for rows, a in R._lora_rows(*self.rows):
            if ads[a]:
                mag[rows] = ads[a][2] * ((x[rows] @ ads[a][0].T).abs() @ ads[a][1].abs().T)
        return R.lora_linear(y, self.x, ads, *self.rows, self.gain, EPS), 4 * U * mag

    def judge(self):
        """``(reference, bound, base rows)``: the module docstring's bounds; a base row has no delta term at all."""
        (g, eg), (u, eu) = self.terms(self.mods[0]), self.terms(self.mods[-1])
        base = (eg + eu).sum(-1) == 0
        if len(self.mods) == 1:
            return g, 4 * U * g.abs() + eg, base
        ref = R.lora_gate_up(self.y, self.x, self.gain, self.adapters, *self.rows, EPS)
        return ref, 1.1 * u.abs() * eg + F.silu(g).abs() * eu + 1.1 * eg * eu + 4 * U * ref.abs(), base


@functools.lru_cache(maxsize=None)
def _case(K, N, rank, rows, mods, normed):
    c = Case(K, N, rank, rows, mods, normed)
    return (c, *c.judge())


def _pack(c, K, N, rank):
    pack = ops.pack_lora_linear(1, {**{p: (N, K) for p in c.mods}, "down": (N * len(c.mods), K)}, N_AD, rank, DEV)
    for a, ad in enumerate(c.adapters):
        tensors = {f"l0.{p}.lora_{n}": t for p, v in ad.items() for n, t in (("A", v[0]), ("B", v[1]))}
        pack.load(a, tensors, {p: v[2] for p, v in ad.items()},
                  gains=None if c.gain is None else {p: [c.gain] for p in c.mods})
    for t in (*pack.A.values(), *pack.B.values()):
        t[:, N_AD - 1] = float("nan")
    return pack


def _run(c, pack, nsplit, slot=None, ct=0):
    """One forward's launches on fresh NaN-filled scratch: ``(result, what its base rows must equal)`` on the device."""
    tab = torch.full((ops.lora_table_elems(c.B, c.S, N_AD),), NAN_BITS, dtype=torch.int32, device=DEV)
    tiles = ops.lora_tiles(c.slots.to(DEV) if slot is None else slot, c.B, c.S, None if c.sid is None else c.sid.to(DEV),
                           n_adapters=N_AD, out=tab)
    ns = nsplit or ops.lora_linear_split(tiles, c.x.shape[1], pack.dims[pack.group_of(c.mods[0])][2])
    ws = torch.full((pack.workspace_elems(tiles.max_tiles, ns, c.mods[0]),), float("nan"), device=DEV)
    x, y = c.x.to(DEV, torch.bfloat16), c.y.to(DEV, torch.bfloat16)
    kw = dict(normed=c.gain is not None, eps=EPS, workspace=ws, nsplit=nsplit, ct=ct)
    if c.mods == ("o",):
        return ops.lora_linear_(y.clone(), x, pack, "o", 0, tiles, **kw), y
    I = c.y.shape[1] // 2
    pre = ops.interleave_gate_up(y[:, :I].T.contiguous(), y[:, I:].T.contiguous()).T.contiguous()
    return ops.lora_gate_up(pre, x, pack, 0, tiles, **kw), ops.silu_mul_interleaved(pre)


@pytest.mark.parametrize("rows", sorted(ROWS))
@pytest.mark.parametrize("rank", [1, 16, 17, 64])
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_kernels_match_the_oracle(form, K, N, rank, rows):
    mods, normed = FORMS[form]
    c, ref, bound, base_rows = _case(K, N // len(mods), rank, rows, mods, normed)
    pack = _pack(c, K, N // len(mods), rank)
    for i, ns in enumerate((0, 0, 1, 2)):  # the host rule's split and its repeat, forced 1 and 2
        got, base = _run(c, pack, ns, ct=ns)  # ... the last with two 64-column groups per block (N = 80: 1 + partial)
        first = got if i == 0 else first
        assert torch.isfinite(got).all()
        assert torch.equal(got[base_rows], base[base_rows]), "a base row is not bit-identical"
        w = worst(got.float().cpu(), ref, bound)
        print(f"{form} K={K} N={N} r={rank} {rows} split {ns}: {w:.3f} of the bound")
        assert w <= 1.0
        assert ns or torch.equal(got, first), "repeats differ"


def test_graph_replay_regroups_rows():
    """``lora_slot`` rewritten between replays: the captured tile kernel regroups, no re-capture."""
    c = Case(256, 48, 16, "5x1", ("o",), False)
    pack = _pack(c, 256, 48, 16)
    slot, y0, x = c.slots.to(DEV), c.y.to(DEV, torch.bfloat16), c.x.to(DEV, torch.bfloat16)
    y = y0.clone()
    tab = torch.full((ops.lora_table_elems(5, 1, N_AD),), NAN_BITS, dtype=torch.int32, device=DEV)
    ws = torch.full((pack.workspace_elems(ops.lora_max_tiles(5, 1, N_AD), 1),), float("nan"), device=DEV)

    def run():
        y.copy_(y0)
        ops.lora_linear_(y, x, pack, "o", 0, ops.lora_tiles(slot, 5, 1, n_adapters=N_AD, out=tab), workspace=ws, nsplit=1)

    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for slots in ([1, 1, -1, 0, 0], [-1] * 5, [0, 1, 0, 1, 0], [2, 0, 0, 0, 0]):
        slot.copy_(torch.tensor(slots, dtype=torch.int32))
        c.rows = (torch.tensor(slots, dtype=torch.int32), 5, 1, None)
        eager, (ref, bound, _) = _run(c, pack, 1, slot=slot)[0], c.judge()
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager), f"replay with lora_slot {slots} differs from the eager run"
        assert worst(y.float().cpu(), ref, bound) <= 1.0
