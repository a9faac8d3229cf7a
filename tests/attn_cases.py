"""Shared inputs, metric, rounding model and mutant oracles of the attention tests (a plain helper module:
``tests/test_attn_cases_cpu.py`` checks what it builds, ``tests/test_attn_edges_gpu.py`` and the older
attention tests import it).  Device-agnostic torch; every builder draws on the CPU from a seeded generator
and moves the result, so the CPU test checks the very tensors the GPU tests launch on.

The metric.  ``head_err`` normalises per (row, head): a batch that holds a one-key row (a raw V row,
magnitude 3-4) next to rows that average hundreds of keys (magnitude 0.1) no longer hides the long rows
behind the short one's magnitude, as ``max|a - b| / max|b|`` over the whole batch does.

The canonical form.  All three contracts -- prefill over a fused ``qkv``, decode (one query per sequence
against a cache) and ctx / verify (a chunk at ``past`` against a cache) -- reduce to a list of ``Row``:
``q [n, Hq, D]``, ``k, v [L, Hkv, D]`` in fp32 and ``pos [n]``; query ``i`` sees keys ``j <= pos[i]``.
``attend`` evaluates it exactly (the oracle, equal to ``ops.reference``'s functions), as the kernels round
(``attention_model``) or with one mutation (``mutants``).

The inputs.  On plain ``randn`` a single key of a 300-key row carries 1/300 of the softmax mass: losing it
moves the output by about as much as rounding does, so no bound separates the two.  The builders therefore
give the keys a kernel can lose real mass and an output column of their own:

* every query ``i`` gets a component ``u[pos_i]`` that its last visible key ``pos_i`` and the first hidden
  one ``pos_i + 1`` share (score boost ``BOOST`` each), and a common component ``e0`` shared with the edge
  keys: row 0, rows ``64 t - 1`` and ``64 t`` of the edge tiles, and row ``past - 1``;
* ``u[p]`` and ``e0`` come from one orthonormal basis, an edge key carries ``e0`` alone (one boost per pair,
  never two), and the boosted keys and the queries keep a quarter of their random part, so the boosted scores
  of a query agree to within a factor of a few;
* the V row of a boosted key has a spike of ``V_SPIKE`` in a column of its own, so its weight shows in one
  output column whatever the other keys do;
* the key in the middle of every even edge tile is a peak: boosted by ``PEAK_MORE`` more, with a small V row
  and no spike.  It takes mass without raising any column, and makes tile 0's running max differ from
  tile 1's, which is what a merge that forgets the ``exp(m_s - m)`` rescale gets wrong.

Edge tiles: every 64-row tile of a row of at most 8 tiles; the first two, a middle one and the last two of a
longer row (boosting all 260 edges of a 130-tile row would leave each 1/260 of the mass again)."""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from mlmicroservicetemplate_amd.ops import reference as R

TILE = 64         # key rows per split / tile / page of every attention kernel (Flash2Tile::BKV, decode chunk >= 64)
NAN8 = 0x7F       # the e4m3 NaN byte
BOOST = 6.0       # score added to a boosted (query, key) pair, in units of the softmax exponent
KEEP = 0.25       # share of its random part a boosted key keeps
Q_KEEP = 0.25     # ... and a query: the boosted scores then agree to about e^(+-1)
V_SPIKE = 6.0     # the spike in a boosted key's V row
PEAK_MORE = 1.0   # the peak key of an even tile is boosted by this much more
EPS = 1e-6
ROPE_THETA = 500000.0


def head_err(got: torch.Tensor, want: torch.Tensor, D: int) -> torch.Tensor:
    """Per (row, head): ``max|got - want| / (max|want| + eps)`` over the head's D columns, for ``[rows, H*D]``
    (pass valid rows only).  Returns ``[rows, H]``; the caller takes ``.max()``."""
    g = got.float().reshape(got.shape[0], -1, D)
    w = want.float().reshape(want.shape[0], -1, D)
    return (g - w).abs().amax(-1) / (w.abs().amax(-1) + EPS)


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """The older global metric (kept for the record in test_attn_cases_cpu.py)."""
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


class Row:
    """One batch row: fp32 ``q [n, Hq, D]``, ``k, v [L, Hkv, D]``, ``pos [n]`` (query i sees keys <= pos[i]);
    ``k_raw``: the un-rotated K of the appended row of a rope-mode decode step (mutant 8), else None."""

    def __init__(self, q, k, v, pos, k_raw=None):
        self.q, self.k, self.v, self.pos, self.k_raw = q, k, v, pos.long(), k_raw


def _visible(row: Row) -> torch.Tensor:
    L = row.k.shape[0]
    return torch.arange(L, device=row.k.device).view(1, L) <= row.pos.view(-1, 1)


def attend_row(row: Row, scale: Optional[float] = None, *, model: bool = False, visible=None, kv_shift: int = 0,
               merge=None, k=None) -> torch.Tensor:
    """softmax(q k^T scale, masked to ``visible [n, L]``) v of one row -> fp32 ``[n, Hq*D]``.
    ``model``: as the kernels round -- fp32 scores, P = exp(s - max) rounded to bf16 before P V, fp32
    accumulation and row sum, bf16 output (K / V as bf16, which only changes dequantised e4m3 rows).
    ``kv_shift``, ``merge``, ``k`` and a foreign ``visible`` are the mutants' hooks."""
    q, kk, vv = row.q, (row.k if k is None else k), row.v
    n, Hq, D = q.shape
    Hkv = kk.shape[1]
    scale = D ** -0.5 if scale is None else scale
    head = (torch.arange(Hq, device=q.device) // (Hq // Hkv) + kv_shift) % Hkv
    kk, vv = kk[:, head], vv[:, head]  # [L, Hq, D]
    if model:
        kk, vv = kk.to(torch.bfloat16).float(), vv.to(torch.bfloat16).float()
    s = torch.einsum("qhd,lhd->hql", q, kk) * scale
    vis = _visible(row) if visible is None else visible
    s = s.masked_fill(~vis.unsqueeze(0), float("-inf"))
    if merge is not None:
        return merge(s, vv).reshape(n, Hq * D)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))  # a row with no key: all zeros
    l = p.sum(-1, keepdim=True).clamp_min(1e-30)
    if model:
        p = p.to(torch.bfloat16).float()
    o = torch.einsum("hql,lhd->qhd", p, vv) / l.permute(1, 0, 2)
    if model:
        o = o.to(torch.bfloat16).float()
    return o.reshape(n, Hq * D)


def attend(rows: List[Row], scale: Optional[float] = None, **kw) -> torch.Tensor:
    """The valid rows of every batch row, concatenated: fp32 ``[sum n, Hq*D]``."""
    return torch.cat([attend_row(r, scale, **kw) for r in rows])


def attention_model(rows: List[Row], scale: Optional[float] = None) -> torch.Tensor:
    """The rounding model of the kernels on the same masks as the oracle (see ``attend_row``): the honest
    kernel against which a tolerance is measured."""
    return attend(rows, scale, model=True)


def tolerance(rows: List[Row], D: int, factor: float = 4.0, scale: Optional[float] = None) -> float:
    """``factor`` x the rounding model's per-head error against the fp32 oracle on these inputs.  The factor
    covers what the model leaves out: exp2 with a folded scale, split merges, MFMA summation order."""
    return factor * head_err(attention_model(rows, scale), attend(rows, scale), D).max().item()


# ------------------------------------------------------------------ rows of the three contracts' tensors
def rows_prefill(qkv, B, S, Hq, Hkv, D, kv_lens=None, causal=False, q_rows=None) -> List[Row]:
    """``R.attention``'s masks: key j is hidden at j >= kv_lens[b] and, causal, at j > i.  Every query row
    is an output row (``q_rows``: the first q_rows of each sequence, ``ops.flash_attention_rows``)."""
    q, k, v = R.split_qkv(qkv.float(), Hq, Hkv, D)
    rows = []
    for b in range(B):
        L = S if kv_lens is None else int(kv_lens[b])
        n = S if q_rows is None else q_rows
        i = torch.arange(n, device=qkv.device)
        pos = torch.clamp(i, max=L - 1) if causal else torch.full_like(i, L - 1)
        rows.append(Row(q[b * S: b * S + n], k[b * S: b * S + L], v[b * S: b * S + L], pos))
    return rows


def rows_decode(q, k_cache, v_cache, lens, Hq, Hkv, D, head_major=False) -> List[Row]:
    """``R.decode_attention``'s contract: fp32 (dequantised) caches ``[B, max_len, Hkv, D]``
    (``head_major``: ``[B, Hkv, max_len, D]``), one query per sequence that sees rows < lens[b]."""
    rows = []
    for b in range(lens.numel()):
        L = int(lens[b])
        kb, vb = (c[b].transpose(0, 1) if head_major else c[b] for c in (k_cache, v_cache))
        rows.append(Row(q[b, : Hq * D].float().view(1, Hq, D), kb[:L].float(), vb[:L].float(),
                        torch.tensor([L - 1], device=q.device)))
    return rows


def rows_ctx(qkv, k_cache, v_cache, past, lens, B, S, Hq, Hkv, D, slot_ids=None, page_table=None) -> List[Row]:
    """``R.attention_ctx``'s contract on head-major (dequantised) caches: query i of row b sits at
    ``past[b] + i`` and sees rows ``0 .. past[b] + i`` of its slot.  Rows with no valid query are left out."""
    q = qkv[:, : Hq * D].float().view(B, S, Hq, D)
    rows = []
    for b in range(B):
        P, L = int(past[b]), int(lens[b])
        n = min(L - P, S)
        if n <= 0:
            continue
        slot = b if slot_ids is None else int(slot_ids[b])
        kv = []
        for c in (k_cache, v_cache):
            blk = c[page_table[slot].long()] if page_table is not None else c[slot: slot + 1]
            kv.append(blk.transpose(1, 2).reshape(-1, Hkv, D)[:L].float())
        rows.append(Row(q[b, :n], kv[0], kv[1], P + torch.arange(n, device=qkv.device)))
    return rows


def valid_rows(out: torch.Tensor, B: int, S: int, n) -> torch.Tensor:
    """The first n[b] rows of every batch row of ``out [B*S, W]``, concatenated (``attend``'s order)."""
    o = out.view(B, S, -1)
    return torch.cat([o[b, : int(n[b])] for b in range(B) if int(n[b]) > 0])


# ------------------------------------------------------------------ mutants
def edge_tiles(ntile: int) -> List[int]:
    """The tiles whose edge keys are boosted and mutated: all of a short row, five of a long one."""
    if ntile <= 8:
        return list(range(ntile))
    return sorted({0, 1, ntile // 2, ntile - 2, ntile - 1})


def _merge_without_rescale(s, vv):
    """Mutant 7: each 64-key split's normalised O weighted by its own l_s, the exp(m_s - m) factor lost."""
    H, n, L = s.shape
    acc = torch.zeros(n, H, vv.shape[-1], device=s.device)
    lsum = torch.zeros(H, n, 1, device=s.device)
    for k0 in range(0, L, TILE):
        ss = s[..., k0: k0 + TILE]
        m = ss.amax(-1, keepdim=True)
        p = torch.exp(ss - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
        acc += torch.einsum("hql,lhd->qhd", p, vv[k0: k0 + TILE])
        lsum += p.sum(-1, keepdim=True)
    return acc / lsum.clamp_min(1e-30).permute(1, 0, 2)


def mutants(row: Row):
    """Yield ``(name, attend_row keywords, applies [n] bool)`` for every mutant that applies to this row.
    A mutant is applied to all queries of the row at once -- queries do not interact -- and judged per query
    on those it applies to.

    1. the last visible key of a query is hidden (``j >= pos`` for ``j > pos``);
    2. one key too many inside the row: query i sees key ``pos_i + 1`` (ctx / verify: the next chunk key;
       prefill: causal off by one).  It does not apply where ``pos_i + 1`` is past the row's keys (decode,
       bidirectional prefill, the last query of a chunk): those reads are what the NaN poison covers;
    3. the first key of an edge tile (row 64 t) is dropped;
    4. the last key of a tile before an edge tile (row 64 t - 1) is dropped;
    5. a whole 64-key split / tile is dropped: the first, a middle one (queries with >= 3 tiles), the last
       (partial) one (queries with >= 2 tiles; with one tile it is the first);
    6. query head h reads KV head ``(h / G + 1) % Hkv`` (rows with Hkv > 1);
    7. split partials merged without the ``exp(m_s - m)`` rescale (queries with >= 2 tiles);
    8. rope-mode decode: the appended K row is written un-rotated (rows with ``k_raw``; position 0 is not
       rotated, so such a row carries none); "the new row is not visible to its own query" is mutant 1."""
    vis = _visible(row)
    n, L = vis.shape
    dev = vis.device
    j = torch.arange(L, device=dev).view(1, L)
    pos = row.pos.view(n, 1)
    every = torch.ones(n, dtype=torch.bool, device=dev)
    last_tile = pos // TILE
    yield "1 last visible key hidden", dict(visible=vis & (j != pos)), every
    if bool((pos + 1 < L).any()):
        yield "2 one key too many", dict(visible=vis | (j == pos + 1)), (pos + 1 < L).view(n)
    for t in edge_tiles(-(-L // TILE)):
        if bool((pos >= TILE * t).any()):
            yield f"3 first key of tile {t} dropped", dict(visible=vis & (j != TILE * t)), (pos >= TILE * t).view(n)
        if t >= 1 and bool((pos >= TILE * t - 1).any()):
            yield (f"4 last key of tile {t - 1} dropped", dict(visible=vis & (j != TILE * t - 1)),
                   (pos >= TILE * t - 1).view(n))
    yield "5 first split dropped", dict(visible=vis & (j // TILE != 0)), every
    if bool((last_tile >= 2).any()):
        yield ("5 middle split dropped", dict(visible=vis & (j // TILE != (last_tile + 1) // 2)),
               (last_tile >= 2).view(n))
    if bool((last_tile >= 1).any()):
        yield "5 last split dropped", dict(visible=vis & (j // TILE != last_tile)), (last_tile >= 1).view(n)
        yield "7 merge without rescale", dict(merge=_merge_without_rescale), (last_tile >= 1).view(n)
    if row.k.shape[1] > 1:
        yield "6 next KV head", dict(kv_shift=1), every
    if row.k_raw is not None:
        k = row.k.clone()
        k[L - 1] = row.k_raw
        yield "8 appended K row not rotated", dict(k=k), every


def mutant_errors(rows: List[Row], D: int, scale: Optional[float] = None, metric=None):
    """Yield ``(name, batch row, per-query error over the queries the mutant applies to)``: the largest
    per-head error of each such query (``metric``: instead, one global figure of the whole batch, with the
    mutant applied to this row only -- how the older ``rel`` judged it)."""
    want = [attend_row(r, scale) for r in rows]
    for b, row in enumerate(rows):
        for name, kw, applies in mutants(row):
            got = attend_row(row, scale, **kw)
            if metric is None:
                yield name, b, head_err(got, want[b], D).amax(-1)[applies]
            else:
                full = torch.cat(want)
                for i in applies.nonzero().flatten().tolist():  # one query at a time, the rest of the batch right
                    g = [w if c != b else torch.cat([w[:i], got[i: i + 1], w[i + 1:]]) for c, w in enumerate(want)]
                    yield name, b, torch.tensor([metric(torch.cat(g), full)])


# ------------------------------------------------------------------ shaped inputs
def _basis(g, D):
    """A random orthonormal basis of R^D (exactly orthogonal rows, so two boost directions never leak into
    each other's scores; entries of varied size, so the roundings of a boosted K row do not line up)."""
    return torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64)).Q.float()


def _shaped_row(g, n, L, pos, Hq, Hkv, D, past=None):
    """fp32 ``q [n, Hq, D]``, ``k, v [L, Hkv, D]`` with the boosts of the module docstring."""
    pos = torch.as_tensor(pos).long()
    amp = math.sqrt(BOOST * math.sqrt(D))  # |u|^2 / sqrt(D) == BOOST
    basis = amp * _basis(g, D)
    e0 = basis[0]
    u = torch.zeros(L + 1, D)
    own = torch.zeros(L + 1, dtype=torch.bool)
    own[pos] = True
    # u[p] is orthogonal to e0 and to its neighbours' (it comes back every D - 1 positions: one more boosted key)
    u[own] = basis[1 + own.nonzero().flatten() % (D - 1)]
    edge = torch.zeros(L, dtype=torch.bool)
    for t in edge_tiles(-(-L // TILE)):
        edge[TILE * t] = True
        if t >= 1:
            edge[TILE * t - 1] = True
    if past is not None and past >= 1:
        edge[past - 1] = True
    nxt = torch.cat([torch.zeros(1, dtype=torch.bool), own[:L - 1]]) if L > 1 else torch.zeros(L, dtype=torch.bool)
    boosted = edge | own[:L] | nxt
    q = Q_KEEP * torch.randn(n, Hq, D, generator=g) + (u[pos] + e0).unsqueeze(1)
    k = torch.randn(L, Hkv, D, generator=g)
    k[boosted] *= KEEP
    # an edge key carries e0 alone: one boost per (query, key) pair, never two.  A peak key in the middle of
    # every even edge tile is boosted by PEAK_MORE more: tile 0's running max is never tile 1's (mutant 7)
    peak = torch.zeros(L, dtype=torch.bool)
    for t in edge_tiles(-(-L // TILE)):
        if t % 2 == 0 and TILE * t + TILE // 2 < L:
            peak[TILE * t + TILE // 2] = True
    k[peak & ~boosted] *= KEEP
    boosted &= ~peak  # (a peak key that is some query's own key is that query's boosted key all the same)
    part = torch.where(edge.unsqueeze(1), e0.expand(L, D), u[:L] + torch.cat([torch.zeros(1, D), u[:L - 1]]))
    k += torch.where(peak.unsqueeze(1), (1.0 + PEAK_MORE / BOOST) * e0.expand(L, D), part).unsqueeze(1)
    v = torch.randn(L, Hkv, D, generator=g)
    v[peak] *= KEEP  # a peak key takes mass and shows in no column
    jj = boosted.nonzero().flatten()
    for h in range(Hkv):
        v[jj, h, (37 * jj + 11 * (jj // TILE) + 17 * h) % D] += V_SPIKE  # rows 64 t apart: other columns
    return q, k, v


def _bf16(x):
    return x.to(torch.bfloat16)


def _paginate(cache, table, rows_per_page, fill):
    """Head-major ``[slots, Hkv, R, ...]`` -> the same rows in a page pool ``[pages, Hkv, rows_per_page, ...]``
    through ``table [slots, pages_per_seq]``; page 0 and the tail of a slot's last page are ``fill``."""
    slots, Hkv, Rw = cache.shape[:3]
    rest = tuple(cache.shape[3:])
    pps = table.shape[1]
    pad = pps * rows_per_page - Rw
    kw = dict(dtype=cache.dtype, device=cache.device)
    padded = torch.cat([cache, torch.full((slots, Hkv, pad) + rest, fill, **kw)], dim=2)
    pool = torch.full((slots * pps + 1, Hkv, rows_per_page) + rest, fill, **kw)
    pool[table.flatten().long()] = padded.view(slots, Hkv, pps, rows_per_page, *rest).transpose(1, 2).reshape(
        slots * pps, Hkv, rows_per_page, *rest)
    return pool


def _table(g, slots, pps):
    return (1 + torch.randperm(slots * pps, generator=g)).view(slots, pps).to(torch.int32)


def _store(caches, slot, L, k, v, fp8):
    """Write a row's K / V [L, Hkv, D] (bf16) into head-major caches; returns the fp32 rows a kernel sees."""
    seen = []
    for x, (c, sc) in zip((k, v), caches):
        xh = x.transpose(0, 1)  # [Hkv, L, D]
        if fp8:
            c[slot, :, :L], sc[slot, :, :L] = R.kv_quant_fp8(xh)
            seen.append(R.kv_dequant_fp8(c[slot, :, :L], sc[slot, :, :L]).transpose(0, 1).contiguous())
        else:
            c[slot, :, :L] = xh
            seen.append(x.float())
    return seen


def _empty_caches(slots, Hkv, rows, D, fp8):
    """Two (cache, scales) pairs, poisoned: NaN (bf16) or 0x7F bytes with NaN scales (e4m3)."""
    out = []
    for _ in range(2):
        if fp8:
            out.append((torch.full((slots, Hkv, rows, D), NAN8, dtype=torch.uint8),
                        torch.full((slots, Hkv, rows), float("nan"), dtype=torch.float32)))
        else:
            out.append((torch.full((slots, Hkv, rows, D), float("nan"), dtype=torch.bfloat16), None))
    return out


def _to(case, device):
    for key, val in list(case.items()):
        if torch.is_tensor(val):
            case[key] = val.to(device)
    for r in case["rows"]:
        for name in ("q", "k", "v", "pos", "k_raw"):
            if getattr(r, name) is not None:
                setattr(r, name, getattr(r, name).to(device))
    return case


def _add_cache_views(case, caches, table, page_rows, fp8):
    (kc, ks), (vc, vs) = caches
    case.update(kc=kc, vc=vc, fp8=fp8)
    if fp8:
        case.update(ks=ks, vs=vs)
    case.update(paged_views(case, page_rows, table))


def paged_views(case, page_rows, table=None, seed=0):
    """The case's head-major caches as page pools of ``page_rows`` rows: ``kp, vp`` (``ksp, vsp``), ``table``."""
    slots, _, rows = case["kc"].shape[:3]
    if table is None:
        table = _table(torch.Generator().manual_seed(seed), slots, -(-rows // page_rows)).to(case["kc"].device)
    fill = NAN8 if case["fp8"] else float("nan")
    out = dict(table=table, kp=_paginate(case["kc"], table, page_rows, fill),
               vp=_paginate(case["vc"], table, page_rows, fill))
    if case["fp8"]:
        out.update(ksp=_paginate(case["ks"], table, page_rows, float("nan")),
                   vsp=_paginate(case["vs"], table, page_rows, float("nan")))
    return out


def prefill_case(B, S, Hq, Hkv, D, causal, kv_lens=None, seed=0, device="cpu"):
    """A fused bf16 ``qkv [B*S, (Hq+2Hkv)*D]`` for ``ops.flash_attention`` / ``_rows``.  K / V rows at or past
    ``kv_lens[b]`` belong to the same launch's tiles (a kernel may load and mask them), so they are loud
    (8 x randn), not NaN."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.empty(B * S, (Hq + 2 * Hkv) * D)
    for b in range(B):
        L = S if kv_lens is None else int(kv_lens[b])
        i = torch.arange(S)
        pos = torch.clamp(i, max=L - 1) if causal else torch.full_like(i, L - 1)
        q, k, v = _shaped_row(g, S, L, pos, Hq, Hkv, D)
        pad = 8 * torch.randn(2, S - L, Hkv, D, generator=g)
        blk = qkv[b * S: (b + 1) * S]
        blk[:, : Hq * D] = q.reshape(S, -1)
        blk[:, Hq * D: (Hq + Hkv) * D] = torch.cat([k, pad[0]]).reshape(S, -1)
        blk[:, (Hq + Hkv) * D:] = torch.cat([v, pad[1]]).reshape(S, -1)
    qkv = _bf16(qkv)
    lens_t = None if kv_lens is None else torch.tensor(kv_lens, dtype=torch.int32)
    case = dict(B=B, S=S, Hq=Hq, Hkv=Hkv, D=D, causal=causal, qkv=qkv, kv_lens=lens_t,
                rows=rows_prefill(qkv, B, S, Hq, Hkv, D, lens_t, causal))
    return _to(case, device)


def decode_case(lens, Hq, Hkv, D, cache_rows, page_rows=TILE, seed=0, rope=False, fp8=False, device="cpu"):
    """One query per sequence against head-major caches ``kc, vc [B, Hkv, cache_rows, D]`` (``ks, vs`` scales
    when ``fp8``), the same rows in page pools of ``page_rows`` (``kp, vp, table``), ``q [B, (Hq+2Hkv)*D]``.
    Plain mode: the K / V columns of q are NaN.  ``rope``: q is the raw fused row of the step at
    ``positions = lens - 1``; cache row ``lens - 1`` is still poisoned and ``rows`` hold what the launch must
    leave there: bf16 RoPE of the raw K (quantised when ``fp8``) and the raw V."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    caches = _empty_caches(B, Hkv, cache_rows, D, fp8)
    qrow = torch.full((B, (Hq + 2 * Hkv) * D), float("nan"))
    cos, sin = R.rope_tables(cache_rows, D, ROPE_THETA)
    rows = []
    for b, L in enumerate(lens):
        p = torch.tensor([L - 1])
        q, k, v = (_bf16(t) for t in _shaped_row(g, 1, L, p, Hq, Hkv, D))
        k_raw = None
        if rope:
            # the shaped q and new K are the rotated ones: the launch is given their inverse rotation
            q_raw = _bf16(R.rope(q.float(), p, cos, -sin))
            k_new = _bf16(R.rope(k[L - 1:].float(), p, cos, -sin))
            qrow[b] = torch.cat([q_raw.reshape(-1), k_new.reshape(-1), v[L - 1].reshape(-1)]).float()
            q = _bf16(R.rope(q_raw.float(), p, cos, sin))
            k = torch.cat([k[:L - 1], _bf16(R.rope(k_new.float(), p, cos, sin))])
            if L > 1:
                k_raw = k_new[0]
        else:
            qrow[b, : Hq * D] = q.reshape(-1).float()
        ks_, vs_ = _store(caches, b, L, k, v, fp8)
        if rope:  # the appended row is the launch's to write
            if k_raw is not None and fp8:
                k_raw = R.kv_dequant_fp8(*R.kv_quant_fp8(k_raw))
            for c, sc in caches:
                c[b, :, L - 1] = NAN8 if fp8 else float("nan")
                if fp8:
                    sc[b, :, L - 1] = float("nan")
        rows.append(Row(q.float(), ks_, vs_, p, None if k_raw is None else k_raw.float()))
    case = dict(B=B, Hq=Hq, Hkv=Hkv, D=D, q=_bf16(qrow), lens=torch.tensor(lens, dtype=torch.int32), rows=rows,
                cos=cos, sin=sin, positions=torch.tensor(lens, dtype=torch.int32) - 1)
    _add_cache_views(case, caches, _table(g, B, -(-cache_rows // page_rows)), page_rows, fp8)
    return _to(case, device)


def ctx_case(pasts, counts, S, Hq, Hkv, D, max_seq=333, slot_ids=(7, 2, 8, 0, 5, 3), seed=0, fp8=False, device="cpu"):
    """The tensors of the ctx / verify tests' ``_case``: ``qkv [B*S, (Hq+2Hkv)*D]`` (K / V columns NaN: they
    come from the cache), ``past``, ``n`` = counts, ``lens``, shuffled ``slot_ids`` into head-major caches
    ``kc, vc [B + 3, Hkv, max_seq, D]`` and the same rows in 64-row page pools; unused slots, rows >= lens
    and page tails poisoned."""
    g = torch.Generator().manual_seed(seed)
    B = len(pasts)
    n_slots = B + 3
    caches = _empty_caches(n_slots, Hkv, max_seq, D, fp8)
    qkv = torch.full((B * S, (Hq + 2 * Hkv) * D), float("nan"))
    qkv[:, : Hq * D] = torch.randn(B * S, Hq * D, generator=g)  # rows past a row's count: unspecified, finite
    rows = []
    for b, (P, n) in enumerate(zip(pasts, counts)):
        L = P + n
        pos = P + torch.arange(n)
        q, k, v = (_bf16(t) for t in _shaped_row(g, n, L, pos, Hq, Hkv, D, past=P))
        qkv[b * S: b * S + n, : Hq * D] = q.reshape(n, -1).float()
        ks_, vs_ = _store(caches, slot_ids[b], L, k, v, fp8)
        rows.append(Row(q.float(), ks_, vs_, pos))
    past = torch.tensor(pasts, dtype=torch.int32)
    nt = torch.tensor(counts, dtype=torch.int32)
    case = dict(B=B, S=S, Hq=Hq, Hkv=Hkv, D=D, qkv=_bf16(qkv), past=past, n=nt, lens=past + nt, rows=rows,
                slot_ids=torch.tensor(list(slot_ids[:B]), dtype=torch.int32), max_ctx=int((past + nt).max()))
    _add_cache_views(case, caches, _table(g, n_slots, -(-max_seq // TILE)), TILE, fp8)
    return _to(case, device)


# ------------------------------------------------------------------ the cases of test_attn_edges_gpu.py
DECODE_LENS = [1, 63, 64, 65, 128, 129, 300]   # one key, either side of the 64- and 128-row splits, 5 splits
DECODE_ROWS = 320
VERIFY_PASTS = [0, 1, 62, 63, 64, 200]
CTX_PASTS = [0, 1, 63, 64, 65, 200]


def verify_counts(T):
    """Valid queries per batch row, ragged in [1, T]; the rows at 62 and 63 keep all of theirs (they cross row 64)."""
    return [T, max(1, T - 1), T, T, 1, max(1, T // 2)]


def ctx_counts(S):
    """Full chunks and chunks that end inside a tile."""
    return [S, max(1, S - 1), max(1, S // 2), S, max(1, S - 7), S]


def _specs():
    s = {}
    for Hq, Hkv, D in ((4, 1, 128), (8, 2, 128), (16, 2, 128), (12, 12, 64)):
        for rope in (False, True):
            s[f"decode-{Hq}-{Hkv}-{D}" + ("-rope" if rope else "")] = (
                decode_case, dict(lens=DECODE_LENS, Hq=Hq, Hkv=Hkv, D=D, cache_rows=DECODE_ROWS, rope=rope, seed=11))
            if D == 128:
                s[f"decode8-{Hq}-{Hkv}-{D}" + ("-rope" if rope else "")] = (
                    decode_case, dict(lens=DECODE_LENS, Hq=Hq, Hkv=Hkv, D=D, cache_rows=DECODE_ROWS, rope=rope,
                                      fp8=True, seed=12))
    # more splits than the combine kernel's D = 128 lanes: 130 splits of 64
    s["decode-130-splits"] = (decode_case, dict(lens=[8257], Hq=4, Hkv=1, D=128, cache_rows=8320, seed=13))
    for Hq, Hkv, T in ((4, 1, 4), (8, 2, 4), (8, 1, 2), (4, 2, 8), (2, 2, 16)):
        s[f"verify-{Hq}-{Hkv}-{T}"] = (ctx_case, dict(pasts=VERIFY_PASTS, counts=verify_counts(T), S=T, Hq=Hq, Hkv=Hkv,
                                                       D=128, seed=14))
    for S in (1, 4, 64, 65, 130):
        for fp8 in (False, True):
            s[f"ctx{'8' if fp8 else ''}-8-2-{S}"] = (ctx_case, dict(pasts=CTX_PASTS, counts=ctx_counts(S), S=S, Hq=8,
                                                                     Hkv=2, D=128, fp8=fp8, seed=15))
    for S in (63, 64, 65, 130, 200):  # D = 128, the 4-wave block: causal with GQA
        s[f"prefill-causal-{S}"] = (prefill_case, dict(B=2, S=S, Hq=8, Hkv=2, D=128, causal=True, seed=16))
    s["prefill-lens-130"] = (prefill_case, dict(B=4, S=130, Hq=4, Hkv=1, D=128, causal=False,
                                                kv_lens=[1, 64, 65, 130], seed=17))
    # D = 64, the 8-wave block
    s["prefill64-lens-128"] = (prefill_case, dict(B=4, S=128, Hq=12, Hkv=12, D=64, causal=False,
                                                  kv_lens=[1, 64, 65, 127], seed=18))
    s["prefill64-causal-100"] = (prefill_case, dict(B=2, S=100, Hq=4, Hkv=2, D=64, causal=True, seed=19))
    return s


SPECS = _specs()
_BUILT = {}


def case(name, device="cpu"):
    """One case per (name, device), shared by the tests that use it; never modified."""
    key = (name, str(device))
    if key not in _BUILT:
        fn, kw = SPECS[name]
        _BUILT[key] = fn(device=device, **kw)
    return _BUILT[key]
