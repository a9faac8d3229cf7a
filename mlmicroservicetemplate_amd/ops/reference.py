"""Plain-PyTorch fp32 oracles of every transformer kernel in ``ops`` (device-agnostic: they run
on CPU for the CPU test suite and on GPU as the numerics reference of the HIP kernels)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def layernorm(x, gamma, beta=None, residual=None, eps=1e-5, rms=False):
    """Returns (normed, residual_sum) in fp32."""
    h = x.float() + (residual.float() if residual is not None else 0.0)
    hs = h.to(torch.bfloat16).float() if x.dtype == torch.bfloat16 else h
    if rms:
        y = hs * torch.rsqrt(hs.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()
    else:
        y = F.layer_norm(hs, (hs.shape[-1],), gamma.float(), beta.float() if beta is not None else None, eps)
    return y, hs


def rope_tables(max_pos: int, head_dim: int, theta: float = 500000.0, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    t = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return ang.cos().float().to(device).contiguous(), ang.sin().float().to(device).contiguous()


def rope(x_heads: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """Rotate-half RoPE on ``[T, H, D]`` (fp32 result)."""
    x = x_heads.float()
    half = x.shape[-1] // 2
    c = cos[positions.long()].unsqueeze(1)
    s = sin[positions.long()].unsqueeze(1)
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def split_qkv(qkv: torch.Tensor, Hq: int, Hkv: int, D: int):
    T = qkv.shape[0]
    q = qkv[:, : Hq * D].reshape(T, Hq, D)
    k = qkv[:, Hq * D: (Hq + Hkv) * D].reshape(T, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D: (Hq + 2 * Hkv) * D].reshape(T, Hkv, D)
    return q, k, v


def attention(qkv: torch.Tensor, B: int, S: int, Hq: int, Hkv: int, D: int, kv_lens: Optional[torch.Tensor] = None,
              causal: bool = False, scale: Optional[float] = None) -> torch.Tensor:
    """softmax(QK^T*scale + mask) V over the fused projection; returns fp32 ``[B*S, Hq*D]``."""
    scale = D ** -0.5 if scale is None else scale
    q, k, v = split_qkv(qkv.float(), Hq, Hkv, D)
    q = q.view(B, S, Hq, D).transpose(1, 2)
    k = k.view(B, S, Hkv, D).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    v = v.view(B, S, Hkv, D).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    mask = torch.zeros(B, 1, S, S, dtype=torch.bool, device=qkv.device)
    if kv_lens is not None:
        mask |= (torch.arange(S, device=qkv.device).view(1, 1, 1, S) >= kv_lens.long().view(B, 1, 1, 1))
    if causal:
        mask |= torch.ones(S, S, dtype=torch.bool, device=qkv.device).triu(1).view(1, 1, S, S)
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)
    o = torch.matmul(p, v)
    return o.transpose(1, 2).reshape(B * S, Hq * D)


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor, Hq: int,
                     Hkv: int, D: int, scale: Optional[float] = None) -> torch.Tensor:
    """q ``[B, >=Hq*D]``, caches ``[B, max_len, Hkv, D]``; returns fp32 ``[B, Hq*D]``."""
    scale = D ** -0.5 if scale is None else scale
    B = lens.numel()
    out = []
    for b in range(B):
        L = int(lens[b])
        qb = q[b, : Hq * D].float().view(Hq, D)
        kb = k_cache[b, :L].float().repeat_interleave(Hq // Hkv, dim=1)  # [L, Hq, D]
        vb = v_cache[b, :L].float().repeat_interleave(Hq // Hkv, dim=1)
        s = torch.einsum("hd,lhd->hl", qb, kb) * scale
        p = torch.softmax(s, dim=-1)
        out.append(torch.einsum("hl,lhd->hd", p, vb).reshape(-1))
    return torch.stack(out)


def attention_ctx(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, past: torch.Tensor,
                  lens: torch.Tensor, B: int, S: int, Hq: int, Hkv: int, D: int,
                  slot_ids: Optional[torch.Tensor] = None, page_table: Optional[torch.Tensor] = None,
                  scale: Optional[float] = None, head_major: bool = False) -> torch.Tensor:
    """Chunked-prefill attention against the KV cache (the oracle of ``ops.flash_attention_ctx``):
    query ``i`` of batch row ``b`` (``i < lens[b] - past[b]``, read from the chunk's RoPE'd fused
    ``qkv [B*S, (Hq+2Hkv)*D]``) sits at position ``past[b] + i`` and attends to cache rows
    ``0 .. past[b] + i`` of slot ``slot_ids[b]`` (``b`` when None).  Caches ``[slots, rows, Hkv, D]``
    (``head_major``: ``[slots, Hkv, rows, D]``), or page pools of the same two layouts addressed
    through ``page_table [slots, pages_per_seq]``.  Returns fp32 ``[B*S, Hq*D]``; rows at or past a
    row's valid length are zero."""
    scale = D ** -0.5 if scale is None else scale
    q = qkv[:, : Hq * D].float().view(B, S, Hq, D)
    out = torch.zeros(B, S, Hq, D, dtype=torch.float32, device=qkv.device)
    rep = Hq // Hkv
    for b in range(B):
        P, L = int(past[b]), int(lens[b])
        n = min(L - P, S)
        if n <= 0:
            continue
        slot = b if slot_ids is None else int(slot_ids[b])
        kv = []
        for c in (k_cache, v_cache):  # this slot's rows [rows, Hkv, D], through the table when paged
            blk = c[page_table[slot].long()] if page_table is not None else c[slot: slot + 1]
            if head_major:
                blk = blk.transpose(1, 2)
            kv.append(blk.reshape(-1, Hkv, D)[:L].float().repeat_interleave(rep, dim=1))
        s = torch.einsum("qhd,lhd->hql", q[b, :n], kv[0]) * scale
        pos = P + torch.arange(n, device=qkv.device)
        hidden = torch.arange(L, device=qkv.device).view(1, L) > pos.view(n, 1)
        p = torch.softmax(s.masked_fill(hidden.unsqueeze(0), float("-inf")), dim=-1)
        out[b, :n] = torch.einsum("hql,lhd->qhd", p, kv[1])
    return out.reshape(B * S, Hq * D)


KV_FP8_MAX = 448.0          # largest finite e4m3fn value
KV_FP8_AMAX_FLOOR = 2.0 ** -40  # keeps the scale of an all-zero row finite (and its inverse below fp32 max)


def kv_quant_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The FP8 KV-cache rule, per head row ``x[..., D]`` (bf16-representable values):
    ``scale = max(max|x|, 2^-40) / 448`` in fp32, ``q = e4m3fn_rne(x * (1 / scale))``.
    Returns ``(uint8 [..., D], fp32 scale [...])``; every HIP writer matches this bit for bit."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    # tensor / tensor: true IEEE divisions on every device (a scalar divisor may become a multiply by
    # its reciprocal, one ulp off the rule)
    scale = torch.clamp(amax, min=KV_FP8_AMAX_FLOOR) / torch.full_like(amax, KV_FP8_MAX)
    inv = torch.ones_like(scale) / scale
    q = (xf * inv.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def kv_dequant_fp8(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 ``float(q) * scale`` of :func:`kv_quant_fp8`'s output."""
    return q.view(torch.float8_e4m3fn).float() * scale.float().unsqueeze(-1)


W4_GROUP = 128                 # k values that share one int4 scale
W4_SCALE_FLOOR = 2.0 ** -40    # keeps the scale of an all-zero group non-zero (q = 0 there)


def w4_quant(w: torch.Tensor, group: int = W4_GROUP) -> Tuple[torch.Tensor, torch.Tensor]:
    """The int4 (W4A16) weight rule for ``w [N, K]``, ``K % group == 0``: symmetric, per output row
    and per ``group`` consecutive k: ``scale = max(bf16_rne(max|w_group| / 7), 2^-40)`` held as bf16,
    ``q = clamp(rne(w / scale), -8, 7)`` held as int8.  ``scale * 7 * (1 + 2^-8) < 7.5 * scale``, so the
    clamp never bites and ``|q * scale - w| <= scale / 2``.  Returns ``(int8 [N, K], bf16 [N, K / group])``."""
    N, K = w.shape
    if group != W4_GROUP or K % group:
        raise ValueError(f"w4_quant: groups of {W4_GROUP} k values, K % {W4_GROUP} == 0 (got K {K}, group {group})")
    wf = w.float().reshape(N, K // group, group)
    amax = wf.abs().amax(dim=-1)
    # tensor / tensor: a true IEEE division on every device
    scale = (amax / torch.full_like(amax, 7.0)).to(torch.bfloat16)
    scale = torch.clamp(scale.float(), min=W4_SCALE_FLOOR)
    q = torch.clamp(torch.round(wf / scale.unsqueeze(-1)), -8, 7).to(torch.int8)
    return q.reshape(N, K), scale.to(torch.bfloat16)


def w4_dequant(q: torch.Tensor, scale: torch.Tensor, group: int = W4_GROUP) -> torch.Tensor:
    """fp32 ``float(q) * float(scale)`` of :func:`w4_quant`'s output, the scale expanded over its group:
    an exact product (4-bit times 8-bit significands) -- the quantised model's weights."""
    N, K = q.shape
    return (q.float().reshape(N, K // group, group) * scale.float().unsqueeze(-1)).reshape(N, K)


def w8_quant(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The W8A8 weight rule for ``w [N, K]``: :func:`kv_quant_fp8`'s rule with one scale per output row
    (``scale = max(max|row|, 2^-40) / 448`` in fp32, ``q = e4m3fn_rne(row * (1 / scale))``), applied to the
    weights as the backend holds them (RMSNorm gain folded in, gate / up interleaved on the fused backend).
    Returns ``(uint8 [N, K], fp32 [N])``."""
    if w.dim() != 2:
        raise ValueError("w8_quant: w [N, K]")
    return kv_quant_fp8(w)


def a8_quant(h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The W8A8 activation rule for ``h [M, K]``, the bf16-valued rows that enter a projection: the same
    rule, one dynamic scale per row.  Returns ``(uint8 [M, K], fp32 [M])``."""
    if h.dim() != 2:
        raise ValueError("a8_quant: h [M, K]")
    return kv_quant_fp8(h)


def w8_dequant(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 ``float(q) * scale[n]`` of :func:`w8_quant`'s output: exact (4-bit times 24-bit significands)."""
    return kv_dequant_fp8(q, scale)


def w8a8_product(hq: torch.Tensor, hs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """``(sum_k float(hq) * float(wq)) * (hs[m] * ws[n])`` with fp32 accumulation: every e4m3 x e4m3 product is
    exact in fp32, so two implementations differ in summation order only."""
    acc = hq.view(torch.float8_e4m3fn).float() @ wq.view(torch.float8_e4m3fn).float().T
    return acc * (hs.float().view(-1, 1) * ws.float().view(1, -1))


def w8a8_linear(h: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, rstd: Optional[torch.Tensor] = None):
    """The W8A8 projection of the rows ``h [M, K]`` (rounded to bf16 first: what enters a projection)
    against :func:`w8_quant`'s ``(wq, ws)``: ``(sum_k float(hq) * float(wq)) * (hs * rstd)[m] * ws[n]``.
    ``rstd [M]``: the normalised projections quantise the un-normalised residual row and multiply its scale
    by ``rstd(h)`` -- a per-row dynamic scale absorbs a per-row scalar."""
    hq, hs = a8_quant(h.to(torch.bfloat16))
    if rstd is not None:
        hs = hs * rstd.float().view(-1)
    return w8a8_product(hq, hs, wq, ws)


def gelu(x):
    return F.gelu(x)


# ------------------------------------------------------------------ LoRA on the q/k/v projection
LORA_MODULES = ("q", "k", "v")
LORA_MAX_RANK = 64


def lora_scale(alpha: float, rank: int, use_rslora: bool = False) -> float:
    """``alpha / r``, or ``alpha / sqrt(r)`` with rank-stabilised LoRA."""
    return float(alpha) / (float(rank) ** 0.5 if use_rslora else float(rank))


def lora_qkv(qkv: torch.Tensor, x: torch.Tensor, gain: torch.Tensor, adapters, lora_slot, B: int, S: int, widths,
             slot_ids=None, eps: float = 1e-5) -> torch.Tensor:
    """The per-request LoRA rule on the fused projection, in fp32.  Row m of sequence b (``qkv``, ``x``
    ``[B*S, .]``) lives in cache slot ``slot_ids[b]`` (default b) and takes adapter ``a = lora_slot[slot]``:
    ``a = -1`` leaves the row as it is, ``a >= 0`` adds ``s_p * B_p (A_p . xn[m])`` to segment p of ``widths
    = (Nq, Nk, Nv)`` for every module the adapter has, ``xn = RMSNorm(x[m]) * gain``.  ``adapters[a]``:
    ``{p: (A_p [r, hidden], B_p [N_p, r], s_p)}`` for a subset of ``"q", "k", "v"``.  Returns a new tensor."""
    out = qkv.float().clone()
    xf = x.float()
    xn = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * gain.float().view(1, -1)
    starts = (0, widths[0], widths[0] + widths[1])
    for b in range(B):
        slot = b if slot_ids is None else int(slot_ids[b])
        a = int(lora_slot[slot])
        if a < 0:
            continue
        rows = slice(b * S, (b + 1) * S)
        for p, (A, Bm, s) in adapters[a].items():
            j = LORA_MODULES.index(p)
            t = xn[rows] @ A.float().T
            out[rows, starts[j]: starts[j] + widths[j]] += float(s) * (t @ Bm.float().T)
    return out
