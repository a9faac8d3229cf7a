"""Shared inputs, error bound and mutant oracles of the LoRA q/k/v tests (a plain helper module, as
``attn_cases.py`` is: ``tests/test_lora_cases_cpu.py`` checks what it builds, ``tests/test_lora_gpu.py`` launches
the kernels on the very same tensors).  Every builder draws on the CPU from a seeded generator.

The bound.  Per element ``4 * 2^-9 * (|ref| + s_p * sum_j |t_j * B_nj|)`` with ``t = A_p . xn`` in fp32: the first
term is the final bf16 rounding of ``qkv + delta`` (half an ulp = 2^-9 relative), the second lets ``t`` be rounded to bf16 before the expand product, where each of the r terms of an output element
moves by up to 2^-9 of its magnitude.  The factor 4 is the convention of ``test_attn_edges_gpu.py``.  fp32
accumulation order (split-K) is 2^-24 relative and disappears in it.

One more case family (``generic_a``) draws A in plain fp32 and is judged under the bound plus the load
quantisation's own worst-case term (``bound(a_quant=True)``), so the fold-and-round of the pack is exercised on
values it really rounds.

The inputs.  The base ``qkv``, the residual rows ``x``, ``B`` and the folded ``A diag(gain)`` are bf16-valued (A is
drawn as ``bf16(A0 gain) / gain``), so the oracle and the kernel read the same numbers: quantising an adapter
at load is no error of the kernels, and at rank 4 it alone would exceed the bound on rows whose t nearly cancels.  Gains are drawn log-uniform in [1/3, 3] (a gain left out moves t by a factor of up to 3
per column), ``x`` has standard deviation 2 (rstd is about 1/2: leaving it out doubles the delta), ``alpha = 6``
with ranks 4..64 gives scales 1.5 .. 0.09, never 1, and the adapters are independent draws whose ``B`` differ in
magnitude by adapter index, so a row served by the wrong adapter is off by a delta of its own size.  ``A`` is
scaled so that a delta is of the order of the base ``qkv`` values: the mutants below then miss the oracle by
hundreds of bounds, while rounding stays inside one."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from mlmicroservicetemplate_amd.ops import reference as R

HQ, HKV, D = 8, 2, 128
WIDTHS = (HQ * D, HKV * D, HKV * D)
N = sum(WIDTHS)
ALPHA = 6.0
EPS = 1e-5
N_ADAPTERS = 3
U = 2.0 ** -9  # half an ulp of bf16, relative

# (q, k, v) ranks of the issue; 0: the module is absent
RANKS = ((8, 0, 16), (16, 16, 16), (64, 64, 64), (4, 0, 12))
# B, S, lora_slot, slot_ids
ROWS = {
    "1x1": (1, 1, [0, -1, 1], None),
    "3x1_mixed": (3, 1, [1, -1, 0], None),
    "2x17": (2, 17, [2, 0, -1], None),
    "4x1_base": (4, 1, [-1, -1, -1, -1], None),
    "2x17_slot_ids": (2, 17, [1, -1, 0], [2, 0]),
    # the mutant case: two adapters and a base sequence, none in its own slot
    "3x17_slot_ids": (3, 17, [1, -1, 0], [2, 0, 1]),
}


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def make_adapters(K: int, ranks: Sequence[int], gain: torch.Tensor, seed: int = 0, n: int = N_ADAPTERS,
                  generic_a: bool = False) -> List[Dict[str, tuple]]:
    """``n`` adapters of clearly different content: ``{p: (A [r, K] fp32, B [N_p, r] bf16-valued fp32, s)}``, with
    ``A * gain`` bf16-valued (to one fp32 rounding)."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for a in range(n):
        ad = {}
        for j, p in enumerate(R.LORA_MODULES):
            r = ranks[j]
            if r == 0:
                continue
            A = torch.randn(r, K, generator=g) / (K ** 0.5)
            if not generic_a:
                A = _bf(A * gain.view(1, -1)) / gain.view(1, -1)
            Bm = _bf(torch.randn(WIDTHS[j], r, generator=g) * (0.5 + 0.5 * a) / (r ** 0.5))
            ad[p] = (A, Bm, R.lora_scale(ALPHA, r))
        out.append(ad)
    return out


class Case:
    def __init__(self, K: int, ranks, rows: str, seed: int = 0, generic_a: bool = False):
        """``generic_a``: A is a plain fp32 draw, so the pack's fold ``bf16(A diag(gain))`` rounds for real; judge
        such a case with ``bound(a_quant=True)``."""
        B, S, slots, sid = ROWS[rows]
        g = torch.Generator().manual_seed(seed)
        self.K, self.ranks, self.B, self.S = K, tuple(ranks), B, S
        self.lora_slot = torch.tensor(slots, dtype=torch.int32)
        self.slot_ids = None if sid is None else torch.tensor(sid, dtype=torch.int32)
        self.x = _bf(torch.randn(B * S, K, generator=g) * 2.0)
        self.qkv = _bf(torch.randn(B * S, N, generator=g))
        self.gain = torch.exp((torch.rand(K, generator=g) * 2 - 1) * 1.0986)  # log-uniform in [1/3, 3]
        self.adapters = make_adapters(K, ranks, self.gain, seed, generic_a=generic_a)

    def adapter_of(self, b: int) -> int:
        slot = b if self.slot_ids is None else int(self.slot_ids[b])
        return int(self.lora_slot[slot])

    def reference(self) -> torch.Tensor:
        return R.lora_qkv(self.qkv, self.x, self.gain, self.adapters, self.lora_slot, self.B, self.S, WIDTHS,
                          slot_ids=self.slot_ids, eps=EPS)

    def bound(self, ref: Optional[torch.Tensor] = None, a_quant: bool = False) -> torch.Tensor:
        """``4 * 2^-9 * (|ref| + s * sum_j |t_j * B_nj|)`` per element, ``[B*S, N]``.  ``a_quant``: plus the term of
        the adapter's quantisation at load, ``2^-9 * s * sum_j (sum_k |xn_k A_jk|) |B_nj|``: every element of
        ``A diag(gain)`` moves by at most half a bf16 ulp, 2^-9 of its magnitude, and so does every term of
        ``t_j`` -- the worst case, no factor on it."""
        ref = self.reference() if ref is None else ref
        xn = self.x * torch.rsqrt(self.x.pow(2).mean(-1, keepdim=True) + EPS) * self.gain.view(1, -1)
        mag = torch.zeros_like(ref)
        aq = torch.zeros_like(ref)
        for b in range(self.B):
            a = self.adapter_of(b)
            if a < 0:
                continue
            rows = slice(b * self.S, (b + 1) * self.S)
            c0 = 0
            for j, p in enumerate(R.LORA_MODULES):
                if p in self.adapters[a]:
                    A, Bm, s = self.adapters[a][p]
                    mag[rows, c0: c0 + WIDTHS[j]] = s * ((xn[rows] @ A.T).abs() @ Bm.abs().T)
                    aq[rows, c0: c0 + WIDTHS[j]] = s * ((xn[rows].abs() @ A.abs().T) @ Bm.abs().T)
                c0 += WIDTHS[j]
        return 4 * U * (ref.abs() + mag) + (U * aq if a_quant else 0.0)


def worst(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over the elements of ``|got - ref| / bound`` (a bound of 0 -- an all-zero element -- needs equality)."""
    err = (got.float() - ref.float()).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-30), torch.where(err > 0, torch.inf, 0.0))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------- mutants
def _delta(case: Case, b: int, a: int, *, rstd: bool = True, scale: bool = True, gain: bool = True, kdrop: int = 0,
           k_to_v: bool = False, rows: Optional[slice] = None) -> torch.Tensor:
    """Adapter ``a``'s delta for the rows of sequence b (``rows``: other rows), with one thing left out."""
    rows = slice(b * case.S, (b + 1) * case.S) if rows is None else rows
    x = case.x[rows]
    xn = x * (torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) if rstd else 1.0)
    if gain:
        xn = xn * case.gain.view(1, -1)
    K = case.K - kdrop
    out = torch.zeros(x.shape[0], N)
    starts = (0, WIDTHS[0], WIDTHS[0] + WIDTHS[1])
    for p, (A, Bm, s) in case.adapters[a].items():
        j = R.LORA_MODULES.index(p)
        if k_to_v and p == "k":
            j = 2
        t = xn[:, :K] @ A[:, :K].T
        out[:, starts[j]: starts[j] + WIDTHS[j]] += (s if scale else 1.0) * (t @ Bm.T)
    return out


def mutants(case: Case) -> Dict[str, torch.Tensor]:
    """Wrong results a kernel could plausibly produce, by name.  Needs a case of >= 2 sequences of 17 rows with
    ``slot_ids`` set, two different adapters among them, and k and v present."""
    B, S = case.B, case.S
    base = case.qkv.clone()

    def build(adapter_of, **kw):
        out = base.clone()
        for b in range(B):
            a = adapter_of(b)
            if a >= 0:
                out[b * S: (b + 1) * S] += _delta(case, b, a, **kw)
        return out

    true = case.adapter_of
    m = {
        "neighbour_adapter": build(lambda b: true((b + 1) % B)),
        "slot_ids_ignored": build(lambda b: int(case.lora_slot[b])),
        "k_delta_in_v": build(true, k_to_v=True),
        "rstd_omitted": build(true, rstd=False),
        "scale_omitted": build(true, scale=False),
        "gain_not_folded": build(true, gain=False),
        "last_k_split_dropped": build(true, kdrop=case.K // 2),
    }
    # row 16 of a 17-row sequence takes the next sequence's adapter (a tile that runs over the sequence end)
    out = build(true)
    for b in range(B):
        nxt = true((b + 1) % B)
        row = slice(b * S + 16, b * S + 17)
        out[row] = base[row] + (_delta(case, b, nxt, rows=row) if nxt >= 0 else 0.0)
    m["row16_next_sequence"] = out
    # an a = -1 row modified: the base rows get adapter 0's delta
    m["base_row_modified"] = build(lambda b: true(b) if true(b) >= 0 else 0)
    return m
