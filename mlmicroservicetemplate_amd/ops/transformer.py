"""Transformer ops: norms, embeddings, RoPE, KV cache writes, flash / decode attention, the on-device token pick."""
from __future__ import annotations

import os
from typing import Optional

import torch

from ._lib import check, lib, stream_ptr
from ._core import ACT_NONE, _need, _ptr


# ------------------------------------------------------------------ transformer ops
def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor] = None, *,
              residual: Optional[torch.Tensor] = None, residual_out: Optional[torch.Tensor] = None,
              eps: float = 1e-5, rms: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``LN(x [+ residual])`` (or RMSNorm with ``rms=True``) over the last dim, bf16.
    ``residual_out`` receives the bf16 sum ``x + residual`` (the pre-norm residual stream)."""
    dev = x.device
    _need(x, "x", torch.bfloat16, dev)
    _need(gamma, "gamma", torch.bfloat16, dev)
    D = x.shape[-1]
    rows = x.numel() // D
    if beta is not None:
        _need(beta, "beta", torch.bfloat16, dev)
    if residual is not None:
        _need(residual, "residual", torch.bfloat16, dev)
    out = torch.empty_like(x) if out is None else out
    rc = lib().mls_layernorm(x.data_ptr(), _ptr(residual), gamma.data_ptr(), _ptr(beta), out.data_ptr(),
                             _ptr(residual_out), rows, D, float(eps), int(rms), stream_ptr(dev))
    check(rc, "mls_layernorm")
    return out


def rmsnorm(x, gamma, *, residual=None, residual_out=None, eps: float = 1e-5, out=None):
    return layernorm(x, gamma, None, residual=residual, residual_out=residual_out, eps=eps, rms=True, out=out)


def embed_layernorm(ids: torch.Tensor, type_ids: Optional[torch.Tensor], word: torch.Tensor, pos: torch.Tensor,
                    typ: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, seq_len: int, eps: float = 1e-12,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BERT embeddings: ``LN(word[ids] + pos[t % S] + type[type_ids])``; ids int32 ``[T]``."""
    dev = ids.device
    _need(ids, "ids", torch.int32, dev)
    T = ids.numel()
    D = word.shape[1]
    out = torch.empty(T, D, device=dev, dtype=torch.bfloat16) if out is None else out
    rc = lib().mls_embed_ln(ids.data_ptr(), _ptr(type_ids), word.data_ptr(), pos.data_ptr(), typ.data_ptr(),
                            gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), T, seq_len, D, word.shape[0],
                            float(eps), stream_ptr(dev))
    check(rc, "mls_embed_ln")
    return out


def embed_layernorm_packed(x: torch.Tensor, seq_len: int, word: torch.Tensor, pos: torch.Tensor, typ: torch.Tensor,
                           gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-12):
    """:func:`embed_layernorm` straight from the engine's packed request rows ``x`` int32
    ``[B, 2S + 1]`` = ids | type ids | length (``models.bert.pack_requests``): no unpacking copies.
    Returns ``(out [B*S, D] bf16, lens [B] int32)`` -- the lengths copied out by the same launch."""
    dev = x.device
    _need(x, "x", torch.int32, dev)
    B, W = x.shape
    S = int(seq_len)
    if W != 2 * S + 1 or not x.is_contiguous():
        raise ValueError("x must be contiguous int32 [B, 2*S + 1]")
    D = word.shape[1]
    out = torch.empty(B * S, D, device=dev, dtype=torch.bfloat16)
    lens = torch.empty(B, device=dev, dtype=torch.int32)
    base = x.data_ptr()
    rc = lib().mls_embed_ln2(base, base + 4 * S, W, base + 8 * S, lens.data_ptr(), word.data_ptr(), pos.data_ptr(),
                             typ.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), B * S, S, D,
                             word.shape[0], float(eps), stream_ptr(dev))
    check(rc, "mls_embed_ln2")
    return out, lens


def prefill_slots(pos: torch.Tensor, lens: torch.Tensor, B: int, S: int, slot_ids: Optional[torch.Tensor] = None,
                  table: Optional[torch.Tensor] = None, page_rows: int = 0, max_seq: int = 0) -> torch.Tensor:
    """KV-cache row of every prefill token (int32 ``[B*S]``, -1 = past the sequence's length): batch
    row b = t // S (or ``slot_ids[b]``), position ``pos[t]``; through the page ``table``
    ``[slots][pages]`` (``page_rows`` rows each) or ``slot * max_seq + pos``.  One launch."""
    dev = pos.device
    _need(pos, "pos", torch.int32, dev)
    _need(lens, "lens", torch.int32, dev)
    if slot_ids is not None:
        _need(slot_ids, "slot_ids", torch.int32, dev)
    if table is not None:
        _need(table, "table", torch.int32, dev)
    out = torch.empty(B * S, device=dev, dtype=torch.int32)
    rc = lib().mls_prefill_slots(pos.data_ptr(), lens.data_ptr(), _ptr(slot_ids), _ptr(table),
                                 table.shape[1] if table is not None else 0, page_rows, max_seq, B, S, out.data_ptr(),
                                 stream_ptr(dev))
    check(rc, "mls_prefill_slots")
    return out


def last_rows(x: torch.Tensor, lens: torch.Tensor, B: int, S: int, x2: Optional[torch.Tensor] = None):
    """Row ``b * S + lens[b] - 1`` of ``x`` (and of ``x2``) for every sequence: ``[B, D]`` (pair)."""
    dev = x.device
    _need(x, "x", torch.bfloat16, dev)
    _need(lens, "lens", torch.int32, dev)
    D = x.shape[-1]
    out = torch.empty(B, D, device=dev, dtype=torch.bfloat16)
    out2 = None
    if x2 is not None:
        _need(x2, "x2", torch.bfloat16, dev)
        out2 = torch.empty(B, D, device=dev, dtype=torch.bfloat16)
    rc = lib().mls_last_rows(x.data_ptr(), _ptr(x2), lens.data_ptr(), B, S, D, out.data_ptr(), _ptr(out2),
                             stream_ptr(dev))
    check(rc, "mls_last_rows")
    return out if x2 is None else (out, out2)


def embedding(ids: torch.Tensor, table: torch.Tensor, lo: int = 0, hi: Optional[int] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row gather; with a vocab shard ``[lo, hi)`` out-of-shard ids give zero rows (TP)."""
    dev = ids.device
    _need(ids, "ids", torch.int32, dev)
    _need(table, "table", torch.bfloat16, dev)
    hi = lo + table.shape[0] if hi is None else hi
    T, D = ids.numel(), table.shape[1]
    out = torch.empty(T, D, device=dev, dtype=torch.bfloat16) if out is None else out
    rc = lib().mls_embedding(ids.data_ptr(), table.data_ptr(), out.data_ptr(), T, D, lo, hi, stream_ptr(dev))
    check(rc, "mls_embedding")
    return out


def rope_(qkv: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, n_rot_heads: int,
          head_dim: int) -> torch.Tensor:
    """In-place rotate-half RoPE on the first ``n_rot_heads`` heads of each row of ``qkv``
    (Q heads then K heads in the fused projection output).  cos/sin fp32 ``[max_pos, D/2]``."""
    dev = qkv.device
    _need(qkv, "qkv", torch.bfloat16, dev)
    _need(positions, "positions", torch.int32, dev)
    T = positions.numel()
    rc = lib().mls_rope(qkv.data_ptr(), positions.data_ptr(), cos.data_ptr(), sin.data_ptr(), T, qkv.shape[-1],
                        n_rot_heads, head_dim, stream_ptr(dev))
    check(rc, "mls_rope")
    return qkv


def rope_kv_(qkv: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, n_q_heads: int,
             n_kv_heads: int, head_dim: int, slots: Optional[torch.Tensor] = None, k_cache=None, v_cache=None,
             lens: Optional[torch.Tensor] = None, seq: int = 1, max_seq: int = 0, hm_rows: int = 0):
    """Fused RoPE (Q and K heads, in place) + KV-cache append in one launch.  Cache slots come from
    ``slots`` (-1 = skip) or, with ``slots=None`` and ``max_seq > 0``, from the token index: token t
    is (batch t // seq, position p) -> slot ``b * max_seq + p``, skipped unless ``p < lens[b]``.
    ``hm_rows = R > 0``: head-major cache ``[slots / R][Hkv][R][D]`` (see :func:`decode_attention`)."""
    dev = qkv.device
    _need(qkv, "qkv", torch.bfloat16, dev)
    _need(positions, "positions", torch.int32, dev)
    T = positions.numel()
    rc = lib().mls_rope_kv(qkv.data_ptr(), positions.data_ptr(), cos.data_ptr(), sin.data_ptr(), T, qkv.shape[-1],
                           n_q_heads, n_kv_heads, head_dim, _ptr(slots), _ptr(k_cache), _ptr(v_cache), _ptr(lens),
                           seq, max_seq, k_cache.numel() // (n_kv_heads * head_dim) if k_cache is not None else 0,
                           cos.shape[0], int(hm_rows), stream_ptr(dev))
    check(rc, "mls_rope_kv")
    return qkv


def kv_append(qkv: torch.Tensor, k_col: int, v_col: int, slots: torch.Tensor, k_cache: torch.Tensor,
              v_cache: torch.Tensor, n_kv_heads: int, head_dim: int, hm_rows: int = 0) -> None:
    """Scatter the K/V heads of each token row of ``qkv`` into cache slot ``slots[t]``
    (``hm_rows`` as in :func:`rope_kv_`)."""
    dev = qkv.device
    _need(slots, "slots", torch.int32, dev)
    T = slots.numel()
    rc = lib().mls_kv_append(qkv.data_ptr(), qkv.shape[-1], k_col, v_col, slots.data_ptr(), k_cache.data_ptr(),
                             v_cache.data_ptr(), T, n_kv_heads, head_dim, int(hm_rows), stream_ptr(dev))
    check(rc, "mls_kv_append")


def flash_attention(qkv: torch.Tensor, batch: int, seq: int, n_q_heads: int, n_kv_heads: int, head_dim: int, *,
                    kv_lens: Optional[torch.Tensor] = None, causal: bool = False, scale: Optional[float] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused attention reading Q/K/V in place from the fused projection ``qkv [B*S, (Hq+2Hkv)*D]``.
    Returns ``[B*S, Hq*D]``."""
    dev = qkv.device
    _need(qkv, "qkv", torch.bfloat16, dev)
    T, W = qkv.shape
    if T != batch * seq or W != (n_q_heads + 2 * n_kv_heads) * head_dim:
        raise ValueError("qkv shape does not match batch/seq/heads")
    if kv_lens is not None:
        _need(kv_lens, "kv_lens", torch.int32, dev)
    out = torch.empty(T, n_q_heads * head_dim, device=dev, dtype=torch.bfloat16) if out is None else out
    scale = head_dim ** -0.5 if scale is None else scale
    base = qkv.data_ptr()
    es = qkv.element_size()
    rc = lib().mls_flash_attention(base, base + n_q_heads * head_dim * es, base + (n_q_heads + n_kv_heads) * head_dim * es,
                                   out.data_ptr(), W, W, W, out.shape[1], batch, seq, n_q_heads, n_kv_heads, head_dim,
                                   _ptr(kv_lens), int(causal), float(scale), stream_ptr(dev))
    check(rc, "mls_flash_attention")
    return out


def flash_attention_rows(q: torch.Tensor, kv: torch.Tensor, batch: int, seq: int, q_rows: int, n_q_heads: int,
                         n_kv_heads: int, head_dim: int, *, kv_lens: Optional[torch.Tensor] = None,
                         causal: bool = False, scale: Optional[float] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention of the first ``q_rows`` positions of every sequence against all of its keys:
    ``q [B*q_rows, >= Hq*D]`` (row-strided), ``kv [B*S, 2*Hkv*D]`` (K then V, e.g. a fused K/V
    projection).  Returns ``[B*q_rows, Hq*D]``.  BERT's last layer runs its [CLS] rows this way
    (``q_rows = 1``: one wave per (sequence, head))."""
    dev = q.device
    if q.dtype != torch.bfloat16:  # row-strided: not _need's contiguity check
        raise TypeError(f"q: expected torch.bfloat16, got {q.dtype}")
    _need(kv, "kv", torch.bfloat16, dev)
    HD, KD = n_q_heads * head_dim, n_kv_heads * head_dim
    if q.dim() != 2 or q.shape[0] != batch * q_rows or q.shape[1] < HD or q.stride(1) != 1:
        raise ValueError("q must be [batch * q_rows, >= Hq*D] with unit column stride")
    if tuple(kv.shape) != (batch * seq, 2 * KD) or not kv.is_contiguous():
        raise ValueError("kv must be a contiguous [batch * seq, 2 * Hkv * D]")
    if not 0 < q_rows <= seq:
        raise ValueError("q_rows must be in 1..seq")
    if kv_lens is not None:
        _need(kv_lens, "kv_lens", torch.int32, dev)
    out = torch.empty(batch * q_rows, HD, device=dev, dtype=torch.bfloat16) if out is None else out
    scale = head_dim ** -0.5 if scale is None else scale
    es = kv.element_size()
    rc = lib().mls_flash_attention_rows(q.data_ptr(), kv.data_ptr(), kv.data_ptr() + KD * es, out.data_ptr(),
                                        q.stride(0), 2 * KD, 2 * KD, out.stride(0), batch, seq, q_rows, n_q_heads,
                                        n_kv_heads, head_dim, _ptr(kv_lens), int(causal), float(scale),
                                        stream_ptr(dev))
    check(rc, "mls_flash_attention_rows")
    return out


def flash_ctx_workspace_elems(batch: int, seq: int, n_q_heads: int, head_dim: int, splits: int) -> int:
    """fp32 elements of :func:`flash_attention_ctx`'s split-KV workspace: per (split, token, q head)
    the unnormalised O row and (m, l)."""
    return int(splits) * batch * seq * n_q_heads * (head_dim + 2)


def _need_kv_hm(k_cache, v_cache, n_kv_heads: int, head_dim: int, dev) -> None:
    """The bf16 KV cache :func:`flash_attention_ctx` reads: head-major ``[blocks, Hkv, R, 128]``."""
    _need(k_cache, "k_cache", torch.bfloat16, dev)
    _need(v_cache, "v_cache", torch.bfloat16, dev)
    if head_dim != 128:
        raise ValueError(f"flash_attention_ctx: head_dim must be 128, got {head_dim}")
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        raise ValueError("k_cache and v_cache must be 4-d and of the same shape")
    if k_cache.shape[1] != n_kv_heads or k_cache.shape[3] != head_dim:
        raise ValueError(f"flash_attention_ctx reads head-major caches [blocks, Hkv={n_kv_heads}, rows, {head_dim}] "
                         f"only (a row-major cache is not supported), got {tuple(k_cache.shape)}")


def _flash_attention_ctx(op: str, need_caches, qkv, caches, past, lens, batch: int, seq: int, n_q_heads: int,
                         n_kv_heads: int, head_dim: int, slot_ids, page_table, scale, out, splits, max_ctx, workspace):
    """The body of :func:`flash_attention_ctx` and :func:`flash_attention_ctx_fp8`: ``op`` names the
    caller in the messages and the library's entry points (``mls_<op>`` and ``mls_<op>_split``),
    ``need_caches(*caches, n_kv_heads, head_dim, dev)`` checks ``caches`` = (k_cache, v_cache[, k_scale,
    v_scale]), which the entry points take in that order."""
    dev = qkv.device
    splits = int(splits)
    if splits < 1 or splits > 64:
        raise ValueError(f"{op}: splits must be in [1, 64], got {splits}")
    if splits > 1 and max_ctx is None:
        raise ValueError(f"{op}: splits > 1 needs max_ctx (a host bound on lens)")
    _need(qkv, "qkv", torch.bfloat16, dev)
    need_caches(*caches, n_kv_heads, head_dim, dev)
    _need(past, "past", torch.int32, dev)
    _need(lens, "lens", torch.int32, dev)
    if batch <= 0 or seq <= 0 or n_kv_heads <= 0 or n_q_heads % n_kv_heads:
        raise ValueError("batch, seq > 0 and Hq a multiple of Hkv")
    W = (n_q_heads + 2 * n_kv_heads) * head_dim
    if qkv.dim() != 2 or tuple(qkv.shape) != (batch * seq, W):
        raise ValueError("qkv shape does not match batch/seq/heads")
    if past.numel() != batch or lens.numel() != batch:
        raise ValueError(f"past and lens must have {batch} elements")
    blocks, rows = caches[0].shape[0], caches[0].shape[2]
    if slot_ids is not None:
        _need(slot_ids, "slot_ids", torch.int32, dev)
        if slot_ids.numel() != batch:
            raise ValueError(f"slot_ids must have {batch} elements")
    if page_table is not None:
        _need(page_table, "page_table", torch.int32, dev)
        if page_table.dim() != 2:
            raise ValueError("page_table must be [slots, pages_per_seq]")
        if rows != 64:
            raise ValueError(f"paged {op}: pages of 64 rows (one K/V tile), got {rows}")
        slots, pps = page_table.shape
    else:
        slots, pps = blocks, 0
    if slot_ids is None and batch > slots:
        raise ValueError("the cache holds fewer slots than the batch")
    if out is not None:
        _need(out, "out", torch.bfloat16, dev)
        if out.dim() != 2 or out.shape[0] < batch * seq or out.shape[1] != n_q_heads * head_dim:
            raise ValueError("out must be [B*S, Hq*D]")
    else:
        out = torch.empty(batch * seq, n_q_heads * head_dim, device=dev, dtype=torch.bfloat16)
    scale = head_dim ** -0.5 if scale is None else scale
    head = (qkv.data_ptr(), *(t.data_ptr() for t in caches), out.data_ptr())
    tail = (W, out.stride(0), past.data_ptr(), lens.data_ptr(), _ptr(slot_ids), _ptr(page_table), pps, slots, batch,
            seq, n_q_heads, n_kv_heads, head_dim, blocks, rows)
    if splits > 1:
        if int(max_ctx) < 1:
            raise ValueError(f"{op}: max_ctx must be positive, got {max_ctx}")
        need = flash_ctx_workspace_elems(batch, seq, n_q_heads, head_dim, splits)
        if workspace is None:
            workspace = torch.empty(need, device=dev, dtype=torch.float32)
        _need(workspace, "workspace", torch.float32, dev)
        if workspace.numel() < need or not workspace.is_contiguous():
            raise ValueError(f"{op}: the workspace holds {workspace.numel()} fp32 elements, "
                             f"{splits} splits need {need} (contiguous)")
        if batch * splits > 65535:
            raise ValueError(f"{op}: batch x splits = {batch * splits} exceeds the grid's 65535")
        rc = getattr(lib(), f"mls_{op}_split")(*head, workspace.data_ptr(), workspace.numel(), *tail,
                                               min(int(max_ctx), 0x7FFFFFFF), splits, float(scale), stream_ptr(dev))
        check(rc, f"mls_{op}_split")
        return out
    rc = getattr(lib(), f"mls_{op}")(*head, *tail, float(scale), stream_ptr(dev))
    check(rc, f"mls_{op}")
    return out


def flash_attention_ctx(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, past: torch.Tensor,
                        lens: torch.Tensor, batch: int, seq: int, n_q_heads: int, n_kv_heads: int, head_dim: int, *,
                        slot_ids: Optional[torch.Tensor] = None, page_table: Optional[torch.Tensor] = None,
                        scale: Optional[float] = None, out: Optional[torch.Tensor] = None, splits: int = 1,
                        max_ctx: Optional[int] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Chunked-prefill attention: a chunk of ``seq`` new queries per batch row against the KV cache.
    Query ``i`` of row ``b`` (``i < lens[b] - past[b]``) sits at position ``past[b] + i`` and attends to
    cache rows ``0 .. past[b] + i`` of slot ``slot_ids[b]`` (``b`` when None).  Q is read in place from
    the chunk's fused, RoPE'd ``qkv [B*S, (Hq+2Hkv)*D]``; K / V come only from the cache, so the chunk's
    own rows must have been appended first (:func:`rope_kv_`).  ``past`` / ``lens`` (the absolute end
    after this chunk, as :func:`prefill_slots` takes it) / ``slot_ids`` are int32 ``[B]`` on the device;
    nothing is read on the host (capturable).  Head-major bf16 caches only, D = 128:
    ``[slots, Hkv, max_seq, D]``, or page pools ``[pages, Hkv, 64, D]`` through ``page_table
    [slots, pages_per_seq]``.  Returns ``[B*S, Hq*D]``; rows at or past a row's valid length (padding
    rows) are zeros.

    ``splits`` > 1 (at most 64): split-KV -- every (row, query tile)'s key tiles are cut into ``splits``
    runs that separate blocks walk, then merged (few queries against a long context: a prefix-cache
    hit).  It needs ``max_ctx``, a host bound on ``lens`` that fixes where the runs are cut, and an
    fp32 ``workspace`` of :func:`flash_ctx_workspace_elems` elements (allocated when None).  Padding
    rows are zeros on this route too.  ``max_ctx`` is the caller's promise: ``lens`` is device data the host
    never reads, so a ``lens[b]`` above it is NOT refused -- the key tiles past the last split are
    dropped and that row's result is silently wrong (nothing is read or written out of bounds); only the
    ``MLS_DEBUG`` build reports it (code 314).  A bound that is too large is always safe."""
    return _flash_attention_ctx("flash_attention_ctx", _need_kv_hm, qkv, (k_cache, v_cache), past, lens, batch, seq,
                                n_q_heads, n_kv_heads, head_dim, slot_ids, page_table, scale, out, splits, max_ctx,
                                workspace)


def decode_attention_multi(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, past: torch.Tensor,
                           lens: torch.Tensor, batch: int, seq: int, n_q_heads: int, n_kv_heads: int, head_dim: int, *,
                           slot_ids: Optional[torch.Tensor] = None, page_table: Optional[torch.Tensor] = None,
                           chunk: int = 64, max_len: Optional[int] = None, scale: Optional[float] = None,
                           workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A few queries per sequence against the KV cache, split-KV on the matrix cores: the attention of
    a speculative-decoding verify step.  The contract is :func:`flash_attention_ctx`'s (same arguments,
    same oracle ``reference.attention_ctx``): query ``t`` of row ``b`` (``t < lens[b] - past[b]``) sits
    at position ``past[b] + t`` and attends cache rows ``0 .. past[b] + t`` of slot ``slot_ids[b]``; the
    step's own rows must have been appended first (:func:`rope_kv_`); nothing is read on the host.
    ``seq * Hq / Hkv <= 16`` (the queries and heads of a KV head share one MFMA's lane columns),
    Hq / Hkv in 1, 2, 4, 8.  ``chunk``: cache rows per split block, 64 or 128 (paged: 64, one page);
    ``max_len``: a host bound on ``lens`` (default: what a slot holds) that sizes the split grid, as
    :func:`decode_attention` takes it.  ``workspace``: fp32, ``B*seq*Hq*nsplit*(D+2)`` elements."""
    dev = qkv.device
    _need(qkv, "qkv", torch.bfloat16, dev)
    _need(k_cache, "k_cache", torch.bfloat16, dev)
    _need(v_cache, "v_cache", torch.bfloat16, dev)
    _need(past, "past", torch.int32, dev)
    _need(lens, "lens", torch.int32, dev)
    if batch <= 0 or seq <= 0 or n_kv_heads <= 0 or n_q_heads % n_kv_heads:
        raise ValueError("batch, seq > 0 and Hq a multiple of Hkv")
    if head_dim != 128:
        raise ValueError(f"decode_attention_multi: head_dim must be 128, got {head_dim}")
    G = n_q_heads // n_kv_heads
    if G not in (1, 2, 4, 8) or seq * G > 16:
        raise ValueError(f"decode_attention_multi: Hq / Hkv in 1, 2, 4, 8 and seq * Hq / Hkv <= 16 "
                         f"(got seq {seq}, Hq / Hkv {n_q_heads} / {n_kv_heads})")
    W = (n_q_heads + 2 * n_kv_heads) * head_dim
    if qkv.dim() != 2 or tuple(qkv.shape) != (batch * seq, W):
        raise ValueError("qkv shape does not match batch/seq/heads")
    if past.numel() != batch or lens.numel() != batch:
        raise ValueError(f"past and lens must have {batch} elements")
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        raise ValueError("k_cache and v_cache must be 4-d and of the same shape")
    if k_cache.shape[1] != n_kv_heads or k_cache.shape[3] != head_dim:
        raise ValueError(f"decode_attention_multi reads head-major caches [blocks, Hkv={n_kv_heads}, rows, {head_dim}] "
                         f"only (a row-major cache is not supported), got {tuple(k_cache.shape)}")
    blocks, rows = k_cache.shape[0], k_cache.shape[2]
    if slot_ids is not None:
        _need(slot_ids, "slot_ids", torch.int32, dev)
        if slot_ids.numel() != batch:
            raise ValueError(f"slot_ids must have {batch} elements")
    if chunk not in (64, 128):
        raise ValueError(f"decode_attention_multi: splits of 64 or 128 rows, got {chunk}")
    if page_table is not None:
        _need(page_table, "page_table", torch.int32, dev)
        if page_table.dim() != 2:
            raise ValueError("page_table must be [slots, pages_per_seq]")
        if rows != 64 or chunk != 64:
            raise ValueError(f"paged decode_attention_multi: pages and splits of 64 rows, got {rows} / {chunk}")
        slots, pps = page_table.shape
        cap = pps * 64
    else:
        slots, pps, cap = blocks, 0, rows
    if slot_ids is None and batch > slots:
        raise ValueError("the cache holds fewer slots than the batch")
    max_len = cap if max_len is None else max(1, min(int(max_len), cap))
    nsplit = (max_len + chunk - 1) // chunk
    if nsplit > 1024:
        raise ValueError(f"decode_attention_multi: at most 1024 splits (max_len {max_len} / chunk {chunk})")
    n_o = batch * seq * n_q_heads * nsplit * head_dim
    need = n_o // head_dim * (head_dim + 2)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=dev, dtype=torch.float32)
    _need(workspace, "workspace", torch.float32, dev)
    if out is not None:
        _need(out, "out", torch.bfloat16, dev)
        if tuple(out.shape) != (batch * seq, n_q_heads * head_dim) or not out.is_contiguous():
            raise ValueError("out must be a contiguous [B*S, Hq*D]")
    else:
        out = torch.empty(batch * seq, n_q_heads * head_dim, device=dev, dtype=torch.bfloat16)
    scale = head_dim ** -0.5 if scale is None else scale
    rc = lib().mls_decode_attention_multi(qkv.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(),
                                          workspace.data_ptr(), workspace[n_o:].data_ptr(), W, out.stride(0),
                                          past.data_ptr(), lens.data_ptr(), _ptr(slot_ids), _ptr(page_table), pps,
                                          slots, batch, seq, n_q_heads, n_kv_heads, head_dim, blocks, rows, max_len,
                                          chunk, float(scale), stream_ptr(dev))
    check(rc, "mls_decode_attention_multi")
    return out


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor,
                     n_q_heads: int, n_kv_heads: int, head_dim: int, *, chunk: int = 64,
                     scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None,
                     counters: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                     positions: Optional[torch.Tensor] = None, cos: Optional[torch.Tensor] = None,
                     sin: Optional[torch.Tensor] = None, max_len: Optional[int] = None,
                     page_table: Optional[torch.Tensor] = None, combine: bool = True, head_major: bool = False,
                     impl: Optional[str] = None):
    """One query token per sequence vs the cache ``[B, max_len, Hkv, D]``; q rows ``[B, >= Hq*D]``
    (head h at column h*D, e.g. the fused QKV row).  Split-KV, combined in the same launch.
    With ``positions``/``cos``/``sin`` (rope mode) q is the raw fused QKV row: RoPE is applied to q
    and to the new K (row ``lens - 1 == positions``), and the new K/V are appended to the cache.
    ``max_len``: a host-side bound on ``lens`` (default: the cache length) -- it sizes the split grid,
    so a tight bound keeps idle split blocks out of short-context launches; keys beyond it are not
    visited, so it must be >= every ``lens[b]``.
    Paged KV (``page_table [B, pages_per_seq]`` int32): the caches are page pools ``[pages, chunk,
    Hkv, D]`` and row ``r`` of sequence ``b`` is row ``r % chunk`` of page ``page_table[b, r // chunk]``.
    ``combine=False``: multi-split rows are left as fp32 partials for the consumer GEMM to merge
    (:func:`skinny_packed_combine`); returns ``(out, DecodePartials)``.
    ``head_major``: caches laid out ``[B, Hkv, max_len, D]`` (paged: ``[pages, Hkv, chunk, D]``) --
    one head's rows contiguous, so each split block streams one run instead of 256-B slices.
    ``impl``: "mfma" (matrix-core kernel: D = 128, chunk 64 / 128, G <= 8), "valu", or "auto"
    (default, env ``MLS_DECODE_ATTN``): the matrix-core kernel wherever it applies."""
    impl = impl or os.environ.get("MLS_DECODE_ATTN", "auto")
    impl_code = {"auto": 0, "valu": 1, "mfma": 2}[impl]
    dev = q.device
    B = lens.numel()
    rows_dim = 2 if head_major else 1
    if page_table is not None:
        _need(page_table, "page_table", torch.int32, dev)
        if page_table.dim() != 2 or page_table.shape[0] < B or k_cache.shape[rows_dim] != chunk:
            raise ValueError("paged decode: page_table [>= B, pages_per_seq], caches [pages, chunk, Hkv, D] "
                             "(head-major: [pages, Hkv, chunk, D])")
        cap = page_table.shape[1] * chunk
        max_len = cap if max_len is None else min(int(max_len), cap)
    else:
        L = k_cache.shape[rows_dim]
        max_len = L if max_len is None else min(int(max_len), L)
    hm_rows = k_cache.shape[2] if head_major else 0
    nsplit = (max_len + chunk - 1) // chunk
    need = B * n_q_heads * nsplit * (head_dim + 2)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=dev, dtype=torch.float32)
    if counters is None or counters.numel() < B * n_kv_heads:
        counters = torch.zeros(B * n_kv_heads, device=dev, dtype=torch.int32)
    ws = workspace[: B * n_q_heads * nsplit * head_dim]
    ws_ml = workspace[B * n_q_heads * nsplit * head_dim: need]
    out = torch.empty(B, n_q_heads * head_dim, device=dev, dtype=torch.bfloat16) if out is None else out
    scale = head_dim ** -0.5 if scale is None else scale
    if positions is not None:
        _need(positions, "positions", torch.int32, dev)
    rc = lib().mls_decode_attention(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(),
                                    ws.data_ptr(), ws_ml.data_ptr(), counters.data_ptr(), q.stride(0), out.stride(0),
                                    k_cache.stride(0), lens.data_ptr(), _ptr(positions), _ptr(cos), _ptr(sin),
                                    cos.shape[0] if cos is not None else 0, B, n_q_heads, n_kv_heads, head_dim, max_len,
                                    chunk, float(scale), _ptr(page_table),
                                    page_table.shape[1] if page_table is not None else 0, int(not combine),
                                    int(hm_rows), impl_code, stream_ptr(dev))
    check(rc, "mls_decode_attention")
    if not combine:
        return out, DecodePartials(ws, ws_ml, nsplit, chunk, lens, n_q_heads, head_dim)
    return out


class DecodePartials:
    """Split-KV decode attention partials left for a consumer to merge (see ``combine=False``)."""

    def __init__(self, ws, ws_ml, nsplit, chunk, lens, n_q_heads, head_dim):
        self.ws, self.ws_ml, self.nsplit, self.chunk = ws, ws_ml, int(nsplit), int(chunk)
        self.lens, self.n_q_heads, self.head_dim = lens, int(n_q_heads), int(head_dim)


def _need_kv_fp8(k_cache, v_cache, k_scale, v_scale, n_kv_heads: int, head_dim: int, dev) -> None:
    """The FP8 KV cache: head-major uint8 ``[blocks, Hkv, R, 128]`` and fp32 scales ``[blocks, Hkv, R]``."""
    if head_dim != 128:
        raise ValueError(f"fp8 KV cache: head_dim must be 128, got {head_dim}")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        _need(t, name, torch.uint8, dev)
        if t.dim() != 4 or t.shape[1] != n_kv_heads or t.shape[3] != head_dim:
            raise ValueError(f"{name}: the fp8 cache is head-major [blocks, Hkv={n_kv_heads}, rows, {head_dim}], "
                             f"got {tuple(t.shape)}")
    if k_cache.shape != v_cache.shape:
        raise ValueError("k_cache and v_cache must have the same shape")
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        _need(t, name, torch.float32, dev)
        if tuple(t.shape) != tuple(k_cache.shape[:3]):
            raise ValueError(f"{name}: expected {tuple(k_cache.shape[:3])} (the cache's shape without its last "
                             f"dimension), got {tuple(t.shape)}")


def rope_kv_fp8_(qkv: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, n_q_heads: int,
                 n_kv_heads: int, head_dim: int, slots: Optional[torch.Tensor], k_cache: torch.Tensor,
                 v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                 lens: Optional[torch.Tensor] = None, seq: int = 1, max_seq: int = 0, hm_rows: int = 0):
    """:func:`rope_kv_` writing an FP8 (e4m3) cache: RoPE on the Q and K heads in place in the bf16
    ``qkv`` rows (bit-identical to :func:`rope_kv_`), then each token's K / V head rows quantised by
    ``ops.reference.kv_quant_fp8``'s rule into cache slot ``slots[t]`` (or the derived slot) of the
    head-major uint8 caches ``[blocks, Hkv, R, 128]`` and fp32 scales ``[blocks, Hkv, R]``;
    ``hm_rows`` = R (default: the cache's)."""
    dev = qkv.device
    _need(qkv, "qkv", torch.bfloat16, dev)
    _need(positions, "positions", torch.int32, dev)
    _need_kv_fp8(k_cache, v_cache, k_scale, v_scale, n_kv_heads, head_dim, dev)
    if slots is not None:
        _need(slots, "slots", torch.int32, dev)
    if lens is not None:
        _need(lens, "lens", torch.int32, dev)
    R = k_cache.shape[2]
    hm_rows = int(hm_rows) or R
    if hm_rows != R:
        raise ValueError(f"hm_rows must be the cache's rows per block ({R}), got {hm_rows}")
    if qkv.shape[-1] != (n_q_heads + 2 * n_kv_heads) * head_dim:
        raise ValueError("qkv width does not match the heads")
    T = positions.numel()
    _need(cos, "cos", torch.float32, dev)
    _need(sin, "sin", torch.float32, dev)
    if cos.dim() != 2 or cos.shape[1] != head_dim // 2 or sin.shape != cos.shape:
        raise ValueError("cos / sin must be [max_pos, D/2]")
    if qkv.numel() < T * qkv.shape[-1] or (slots is not None and slots.numel() < T):
        raise ValueError("qkv / slots hold fewer tokens than positions")
    if slots is None and max_seq > 0 and (seq <= 0 or (lens is not None and lens.numel() * seq < T)):
        raise ValueError("derived slots: lens must cover every sequence of seq tokens")
    rc = lib().mls_rope_kv_fp8(qkv.data_ptr(), positions.data_ptr(), cos.data_ptr(), sin.data_ptr(), T, qkv.shape[-1],
                               n_q_heads, n_kv_heads, head_dim, _ptr(slots), k_cache.data_ptr(), v_cache.data_ptr(),
                               k_scale.data_ptr(), v_scale.data_ptr(), _ptr(lens), seq, max_seq,
                               k_cache.shape[0] * R, cos.shape[0], hm_rows, stream_ptr(dev))
    check(rc, "mls_rope_kv_fp8")
    return qkv


def flash_attention_ctx_fp8(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor,
                            v_scale: torch.Tensor, past: torch.Tensor, lens: torch.Tensor, batch: int, seq: int,
                            n_q_heads: int, n_kv_heads: int, head_dim: int, *,
                            slot_ids: Optional[torch.Tensor] = None, page_table: Optional[torch.Tensor] = None,
                            scale: Optional[float] = None, out: Optional[torch.Tensor] = None, splits: int = 1,
                            max_ctx: Optional[int] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`flash_attention_ctx` on an FP8 (e4m3) cache: the contract, arguments and split-KV route
    (``splits``, ``max_ctx``, ``workspace`` of :func:`flash_ctx_workspace_elems` elements) are that
    function's; the caches are :func:`rope_kv_fp8_`'s -- head-major uint8 ``[slots, Hkv, max_seq, 128]``
    or page pools ``[pages, Hkv, 64, 128]`` with fp32 scales of the same shape without the last
    dimension.  A row is attended as ``bf16(e4m3 * scale)``; padding rows (at or past a row's valid
    length) are zeros on both routes; the oracle is
    ``reference.attention_ctx`` on ``reference.kv_dequant_fp8`` of the same bytes."""
    return _flash_attention_ctx("flash_attention_ctx_fp8", _need_kv_fp8, qkv, (k_cache, v_cache, k_scale, v_scale), past,
                                lens, batch, seq, n_q_heads, n_kv_heads, head_dim, slot_ids, page_table, scale, out,
                                splits, max_ctx, workspace)


def decode_attention_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor,
                         v_scale: torch.Tensor, lens: torch.Tensor, n_q_heads: int, n_kv_heads: int, head_dim: int, *,
                         chunk: int = 64, scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None,
                         counters: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                         positions: Optional[torch.Tensor] = None, cos: Optional[torch.Tensor] = None,
                         sin: Optional[torch.Tensor] = None, max_len: Optional[int] = None,
                         page_table: Optional[torch.Tensor] = None, combine: bool = True):
    """:func:`decode_attention` on an FP8 (e4m3) KV cache: head-major uint8 caches ``[B, Hkv, max_len,
    128]`` (paged: ``[pages, Hkv, chunk, 128]``) with one fp32 scale per (row, KV head) in ``k_scale`` /
    ``v_scale`` (the caches' shape without the last dimension).  The matrix-core kernel only:
    D = 128, G = Hq / Hkv in {1, 2, 4, 8}, chunk 64 or 128 -- anything else raises ``ValueError``.
    Rope mode quantises the new K / V row as :func:`rope_kv_fp8_` does and attends to the stored
    (round-tripped) row, so the output is a function of the cache contents after the call.
    Returns what :func:`decode_attention` returns (``combine=False``: ``(out, DecodePartials)``)."""
    dev = q.device
    if q.dtype != torch.bfloat16 or q.dim() != 2 or q.stride(1) != 1 or q.device != lens.device:
        raise ValueError("q must be bf16 rows [B, >= Hq*D] with unit column stride, on the device of lens")
    _need(lens, "lens", torch.int32, dev)
    _need_kv_fp8(k_cache, v_cache, k_scale, v_scale, n_kv_heads, head_dim, dev)
    if n_q_heads % n_kv_heads or n_q_heads // n_kv_heads not in (1, 2, 4, 8):
        raise ValueError(f"fp8 KV cache: Hq / Hkv must be 1, 2, 4 or 8, got {n_q_heads} / {n_kv_heads}")
    if chunk not in (64, 128):
        raise ValueError(f"fp8 KV cache: chunk must be 64 or 128, got {chunk}")
    B = lens.numel()
    R = k_cache.shape[2]
    if R % 4:
        raise ValueError(f"fp8 KV cache: rows per block must be a multiple of 4, got {R}")
    if q.shape[0] < B or q.shape[1] < n_q_heads * head_dim:
        raise ValueError("q must be [B, >= Hq*D]")
    if page_table is not None:
        _need(page_table, "page_table", torch.int32, dev)
        if page_table.dim() != 2 or page_table.shape[0] < B or R != chunk:
            raise ValueError(f"paged fp8 decode: page_table [>= B, pages_per_seq], caches [pages, Hkv, chunk={chunk}, D]"
                             f" (got pages of {R} rows)")
        cap = page_table.shape[1] * chunk
    else:
        if k_cache.shape[0] < B:
            raise ValueError("the cache holds fewer sequences than lens")
        cap = R
    max_len = cap if max_len is None else min(int(max_len), cap)
    if (positions is None) != (cos is None) or (cos is None) != (sin is None):
        raise ValueError("rope mode takes positions, cos and sin together")
    if positions is not None:
        _need(positions, "positions", torch.int32, dev)
        _need(cos, "cos", torch.float32, dev)
        _need(sin, "sin", torch.float32, dev)
        if q.shape[1] < (n_q_heads + 2 * n_kv_heads) * head_dim:
            raise ValueError("rope mode: q must be the fused QKV rows")
        if positions.numel() < B or cos.dim() != 2 or cos.shape[1] != head_dim // 2 or sin.shape != cos.shape:
            raise ValueError("rope mode: positions [B], cos / sin [max_pos, D/2]")
    if out is not None:
        _need(out, "out", torch.bfloat16, dev)
        if out.dim() != 2 or out.shape[0] < B or out.shape[1] < n_q_heads * head_dim:
            raise ValueError("out must be [>= B, >= Hq*D]")
    nsplit = (max_len + chunk - 1) // chunk
    need = B * n_q_heads * nsplit * (head_dim + 2)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=dev, dtype=torch.float32)
    if counters is None or counters.numel() < B * n_kv_heads:
        counters = torch.zeros(B * n_kv_heads, device=dev, dtype=torch.int32)
    ws = workspace[: B * n_q_heads * nsplit * head_dim]
    ws_ml = workspace[B * n_q_heads * nsplit * head_dim: need]
    out = torch.empty(B, n_q_heads * head_dim, device=dev, dtype=torch.bfloat16) if out is None else out
    scale = head_dim ** -0.5 if scale is None else scale
    rc = lib().mls_decode_attention_fp8(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(),
                                        v_scale.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_ml.data_ptr(),
                                        counters.data_ptr(), q.stride(0), out.stride(0), k_cache.shape[0],
                                        lens.data_ptr(), _ptr(positions), _ptr(cos), _ptr(sin),
                                        cos.shape[0] if cos is not None else 0, B, n_q_heads, n_kv_heads, head_dim,
                                        max_len, chunk, float(scale), _ptr(page_table),
                                        page_table.shape[1] if page_table is not None else 0, int(not combine), R,
                                        stream_ptr(dev))
    check(rc, "mls_decode_attention_fp8")
    if not combine:
        return out, DecodePartials(ws, ws_ml, nsplit, chunk, lens, n_q_heads, head_dim)
    return out


def skinny_packed_combine(attn_out: torch.Tensor, parts: DecodePartials, wp: torch.Tensor, N: int, *,
                          bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                          variant: int = 9) -> torch.Tensor:
    """``merge(attention partials) @ W^T (+ bias) (+ residual)`` with W packed (:func:`pack_skinny`):
    the o-projection of a decode step that also does the split-KV combine in its prologue (one
    launch instead of two).  ``attn_out``: the attention's direct-written rows ``[M, Hq*D]``."""
    dev = attn_out.device
    _need(attn_out, "attn_out", torch.bfloat16, dev)
    M, K = attn_out.shape
    if M > 4 or K != parts.n_q_heads * parts.head_dim or wp.numel() != N * K or M * K * 2 > 65536:
        raise ValueError("skinny_packed_combine: M <= 4, K == Hq * D, M * K * 2 <= 64 KiB, wp of N*K elements")
    if residual is not None:
        _need(residual, "residual", torch.bfloat16, dev)
        if tuple(residual.shape) != (M, N):
            raise ValueError("residual must be [M, N]")
    if bias is not None:
        _need(bias, "bias", torch.float32, dev)
    out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    rc = lib().mls_skinny_packed_combine(attn_out.data_ptr(), parts.ws.data_ptr(), parts.ws_ml.data_ptr(),
                                         parts.lens.data_ptr(), parts.nsplit, parts.chunk, parts.n_q_heads,
                                         parts.head_dim, wp.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(),
                                         M, N, K, ACT_NONE, int(variant), stream_ptr(dev))
    check(rc, "mls_skinny_packed_combine")
    return out


def skinny_packed_combine_ar(attn_out: torch.Tensor, parts: DecodePartials, wp: torch.Tensor, N: int, car, *,
                             variant: int = 9) -> torch.Tensor:
    """:func:`skinny_packed_combine` for a row-parallel TP o-projection with its all-reduce fused into
    the same launch (csrc/ar_protocol.h): the split-KV combine in the prologue, the one-shot IPC
    all-reduce of the output in the epilogue -- one kernel where there were three."""
    dev = attn_out.device
    _need(attn_out, "attn_out", torch.bfloat16, dev)
    M, K = attn_out.shape
    if M > 4 or K != parts.n_q_heads * parts.head_dim or wp.numel() != N * K or M * K * 2 > 65536:
        raise ValueError("skinny_packed_combine_ar: M <= 4, K == Hq * D, M * K * 2 <= 64 KiB, wp of N*K elements")
    out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    rc = lib().mls_skinny_packed_combine_ar(attn_out.data_ptr(), parts.ws.data_ptr(), parts.ws_ml.data_ptr(),
                                            parts.lens.data_ptr(), parts.nsplit, parts.chunk, parts.n_q_heads,
                                            parts.head_dim, wp.data_ptr(), out.data_ptr(), M, N, K, int(variant),
                                            car.ctx_ptr(), stream_ptr(dev))
    check(rc, "mls_skinny_packed_combine_ar")
    return out


def decode_pick(cand_v: torch.Tensor, cand_i: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, lens: torch.Tensor,
                step: torch.Tensor, *, topk: Optional[torch.Tensor] = None, temp: Optional[torch.Tensor] = None,
                seed: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None,
                rows: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None,
                emit: Optional[torch.Tensor] = None) -> None:
    """X4 merge + next-token pick on device (csrc/decode_pick.hip): ``cand_v`` / ``cand_i`` are the
    all-gathered ``[tp, B, k]`` candidates; per row picks greedily (``topk <= 1``) or samples
    (top-k, temperature, counter-based ``seed`` x step draw -- :func:`models.llama.sample_uniform`),
    then advances ``tok`` / ``pos`` / ``lens`` / ``step`` in place and records the token in
    ``hist[., step]``.  Capturable (the TP decode graph ends with it).

    Serving (``models/llama_serving.ContinuousLlama``): the per-sequence state arrays may have more
    rows than ``B`` -- ``rows`` int32 ``[B]`` maps candidate row b to its state row (a prefill of new
    sequences into their slots), ``active`` int32 skips idle state rows, ``emit`` int32 receives
    each picked token at its state row."""
    dev = cand_v.device
    tp, B, k = cand_v.shape
    _need(cand_v, "cand_v", torch.float32, dev)
    _need(cand_i, "cand_i", torch.int32, dev)
    if tuple(cand_i.shape) != (tp, B, k) or tp * k > 512:
        raise ValueError("cand_i must match cand_v [tp, B, k] with tp * k <= 512")
    S = tok.numel()  # state rows
    if rows is None and S != B:
        raise ValueError(f"tok must have {B} elements")
    if rows is not None:
        _need(rows, "rows", torch.int32, dev)
        if rows.numel() != B:
            raise ValueError(f"rows must have {B} elements")
    for name, t, dt in (("tok", tok, torch.int32), ("pos", pos, torch.int32), ("lens", lens, torch.int32),
                        ("step", step, torch.int32)):
        _need(t, name, dt, dev)
        if t.numel() != S:
            raise ValueError(f"{name} must have {S} elements")
    for name, t, dt in (("topk", topk, torch.int32), ("temp", temp, torch.float32), ("seed", seed, torch.int64),
                        ("active", active, torch.int32), ("emit", emit, torch.int32)):
        if t is not None:
            _need(t, name, dt, dev)
            if t.numel() != S:
                raise ValueError(f"{name} must have {S} elements")
    cols = 0
    if hist is not None:
        _need(hist, "hist", torch.int32, dev)
        if hist.shape[0] != S:
            raise ValueError("hist must be [state rows, cols]")
        cols = hist.shape[1]
    rc = lib().mls_decode_pick(cand_v.data_ptr(), cand_i.data_ptr(), tp, B, k, _ptr(topk), _ptr(temp), _ptr(seed),
                               tok.data_ptr(), pos.data_ptr(), lens.data_ptr(), _ptr(hist), cols, step.data_ptr(),
                               _ptr(rows), _ptr(active), _ptr(emit), stream_ptr(dev))
    check(rc, "mls_decode_pick")


def _need_rows(t: torch.Tensor, name: str, dt, dev, n: int) -> None:
    _need(t, name, dt, dev)
    if t.numel() != n:
        raise ValueError(f"{name} must have {n} elements")


def spec_draft(rows: torch.Tensor, prompt: torch.Tensor, plen: torch.Tensor, hist: torch.Tensor, step: torch.Tensor,
               max_new: torch.Tensor, pos: torch.Tensor, ids: torch.Tensor, n: torch.Tensor, past: torch.Tensor,
               lens: torch.Tensor, *, K: int, max_ngram: int = 3, min_ngram: int = 1) -> None:
    """Speculative decoding's drafter on device (csrc/spec_step.hip): for verify row r of slot ``rows[r]``
    the feed ``ids[r, :n[r]]`` (the slot's last token and up to K prompt-lookup drafts, zero-padded to
    ``T = ids.shape[1]``), ``past[r] = pos[slot]`` and ``lens[r] = past[r] + n[r]`` -- the static inputs of
    the verify forward.  The slot's tokens are ``prompt[slot, :plen]`` then ``hist[slot, :step]``; the rule
    is ``speculative.spec_feed(tokens, K, max_new - step, prompt_lookup_draft(max_ngram, min_ngram))``, and a
    slot that may emit nothing more (``max_new - step <= 0``) feeds ``n = 0``.  Capturable."""
    dev = rows.device
    _need(rows, "rows", torch.int32, dev)
    Bv = rows.numel()
    _need(prompt, "prompt", torch.int32, dev)
    _need(hist, "hist", torch.int32, dev)
    if prompt.dim() != 2 or tuple(prompt.shape) != tuple(hist.shape):
        raise ValueError("prompt and hist must both be [slots, cols]")
    S, cols = prompt.shape
    for name, t in (("plen", plen), ("step", step), ("max_new", max_new), ("pos", pos)):
        _need_rows(t, name, torch.int32, dev, S)
    _need(ids, "ids", torch.int32, dev)
    if ids.dim() != 2 or ids.shape[0] != Bv:
        raise ValueError(f"ids must be [{Bv}, T]")
    T = ids.shape[1]
    K = int(K)
    if K < 0 or T < K + 1 or Bv < 1 or int(max_ngram) < 1:
        raise ValueError(f"spec_draft: need rows, 0 <= K < T = {T} and max_ngram >= 1 (got K {K}, max_ngram {max_ngram})")
    for name, t in (("n", n), ("past", past), ("lens", lens)):
        _need_rows(t, name, torch.int32, dev, Bv)
    rc = lib().mls_spec_draft(rows.data_ptr(), Bv, S, prompt.data_ptr(), plen.data_ptr(), hist.data_ptr(),
                              step.data_ptr(), max_new.data_ptr(), pos.data_ptr(), cols, K, T, int(max_ngram),
                              int(min_ngram), ids.data_ptr(), n.data_ptr(), past.data_ptr(), lens.data_ptr(),
                              stream_ptr(dev))
    check(rc, "mls_spec_draft")


def spec_accept(cand_v: torch.Tensor, cand_i: torch.Tensor, ids: torch.Tensor, n: torch.Tensor, rows: torch.Tensor,
                tok: torch.Tensor, pos: torch.Tensor, lens: torch.Tensor, step: torch.Tensor, hist: torch.Tensor,
                readback: torch.Tensor, *, topk: Optional[torch.Tensor] = None, temp: Optional[torch.Tensor] = None,
                seed: Optional[torch.Tensor] = None, eos: Optional[torch.Tensor] = None) -> None:
    """Speculative decoding's acceptance on device (csrc/spec_step.hip): ``cand_v`` / ``cand_i`` are the
    all-gathered ``[tp, Bv * T, k]`` candidates of a verify step whose row r (slot ``rows[r]``) fed
    ``ids[r, :n[r]]``.  Row r emits ``y[0]``, then ``y[t]`` while ``ids[r, t] == y[t - 1]`` and ``t < n[r]``,
    stopping after the first token in ``eos`` (``speculative.accept``), with ``y[t]`` the pick of candidate
    row ``r * T + t`` at generated-token index ``step[slot] + t`` by :func:`decode_pick`'s rule.  The ``got``
    tokens go to ``hist[slot, step : step + got]``; ``step`` / ``pos`` advance by ``got``, ``tok`` is the last
    one, ``lens = pos + 1``; ``readback[slot] = (n fed, got, the got tokens)`` (int32 ``[slots, T + 2]``).
    Slots not in ``rows`` are untouched; rows ``t >= n[r]`` are never read.  Capturable."""
    dev = cand_v.device
    _need(cand_v, "cand_v", torch.float32, dev)
    _need(cand_i, "cand_i", torch.int32, dev)
    _need(ids, "ids", torch.int32, dev)
    _need(rows, "rows", torch.int32, dev)
    Bv = rows.numel()
    if ids.dim() != 2 or ids.shape[0] != Bv or Bv < 1:
        raise ValueError(f"ids must be [{Bv}, T]")
    T = ids.shape[1]
    if cand_v.dim() != 3 or cand_v.shape[1] != Bv * T or tuple(cand_i.shape) != tuple(cand_v.shape):
        raise ValueError(f"cand_v / cand_i must be [tp, {Bv * T}, k]")
    tp, _, k = cand_v.shape
    if tp * k > 512:
        raise ValueError("spec_accept: tp * k must be <= 512")
    _need_rows(n, "n", torch.int32, dev, Bv)
    S = tok.numel()
    for name, t in (("tok", tok), ("pos", pos), ("lens", lens), ("step", step)):
        _need_rows(t, name, torch.int32, dev, S)
    for name, t, dt in (("topk", topk, torch.int32), ("temp", temp, torch.float32), ("seed", seed, torch.int64)):
        if t is not None:
            _need_rows(t, name, dt, dev, S)
    _need(hist, "hist", torch.int32, dev)
    if hist.dim() != 2 or hist.shape[0] != S:
        raise ValueError("hist must be [state rows, cols]")
    _need_rows(readback, "readback", torch.int32, dev, S * (T + 2))
    n_eos = 0
    if eos is not None and eos.numel():
        _need(eos, "eos", torch.int32, dev)
        n_eos = eos.numel()
    rc = lib().mls_spec_accept(cand_v.data_ptr(), cand_i.data_ptr(), tp, Bv, T, k, ids.data_ptr(), n.data_ptr(),
                               rows.data_ptr(), S, _ptr(topk), _ptr(temp), _ptr(seed), tok.data_ptr(), pos.data_ptr(),
                               lens.data_ptr(), step.data_ptr(), hist.data_ptr(), hist.shape[1],
                               _ptr(eos) if n_eos else None, n_eos, readback.data_ptr(), stream_ptr(dev))
    check(rc, "mls_spec_accept")


# ------------------------------------------------------------------ LoRA on the q/k/v projection
LORA_GRAN = 16      # ranks are padded to this many rows of A' (one MFMA column tile of t)
LORA_MAX_RANK = 64
LORA_K_GRAN = 128   # hidden must be a multiple (4 waves x one k-step of 32 per split)
_LORA_MODULES = ("q", "k", "v")


class LoraPack:
    """The adapters of one model as the LoRA kernels read them: fixed-address device arrays sized for
    ``max_adapters x max_rank`` at construction, so a captured graph stays valid across :meth:`load`.

    ``A [layers][max_adapters][rcap][hidden]`` bf16: ``A' = bf16(A diag(gain))``, the q, k, v ranks padded
    to ``LORA_GRAN`` with zero rows and laid end to end (``rcap = 3 * padded max_rank``);
    ``B [layers][max_adapters][Nq + Nk + Nv][rb]`` bf16, each row's rank zero-padded to ``rb`` (32 or 64);
    ``seg [max_adapters][4]`` int32 the padded ranks (0: module absent, all 0: slot empty) and
    ``scale [max_adapters][4]`` fp32 the ``s_p``, shared by every layer."""

    def __init__(self, layers: int, hidden: int, widths, max_adapters: int, max_rank: int, device):
        widths = tuple(int(w) for w in widths)
        if not 1 <= int(max_rank) <= LORA_MAX_RANK:
            raise ValueError(f"max_rank must be in 1..{LORA_MAX_RANK}, got {max_rank}")
        if int(max_adapters) < 1:
            raise ValueError(f"max_adapters must be positive, got {max_adapters}")
        if hidden % LORA_K_GRAN:
            raise ValueError(f"hidden {hidden} is not a multiple of the LoRA kernels' K granule {LORA_K_GRAN}")
        if len(widths) != 3 or any(w < 0 or w % 16 for w in widths) or sum(widths) == 0:
            raise ValueError(f"segment widths (Nq, Nk, Nv) must be multiples of 16, got {widths}")
        self.layers, self.hidden, self.widths = int(layers), int(hidden), widths
        self.max_adapters, self.max_rank = int(max_adapters), int(max_rank)
        rpad = -(-self.max_rank // LORA_GRAN) * LORA_GRAN
        self.rcap, self.rb = 3 * rpad, 32 if rpad <= 32 else 64
        self.device = torch.device(device)
        dev, n = self.device, self.max_adapters
        self.A = torch.zeros(self.layers, n, self.rcap, self.hidden, device=dev, dtype=torch.bfloat16)
        self.B = torch.zeros(self.layers, n, sum(widths), self.rb, device=dev, dtype=torch.bfloat16)
        self.seg = torch.zeros(n, 4, device=dev, dtype=torch.int32)
        self.scale = torch.zeros(n, 4, device=dev, dtype=torch.float32)
        self.loaded = [False] * n

    def workspace_elems(self, rows: int, nsplit: int) -> int:
        return int(nsplit) * int(rows) * (self.rcap + 1)

    def load(self, index: int, tensors, scales, gains=None) -> None:
        """Write adapter ``index`` in place.  ``tensors``: ``l{i}.{q,k,v}.lora_A`` ``[r, hidden]`` and
        ``.lora_B`` ``[N_p, r]`` (this rank's rows) for every layer and every module of ``scales = {p: s_p}``;
        ``gains``: per layer the RMSNorm gain ``[hidden]`` folded into A (None: ones)."""
        if not 0 <= int(index) < self.max_adapters:
            raise ValueError(f"adapter index {index} outside [0, {self.max_adapters})")
        mods = [p for p in _LORA_MODULES if p in scales]
        if not mods or len(mods) != len(scales):
            raise ValueError(f"LoRA modules must be a non-empty subset of {_LORA_MODULES}, got {sorted(scales)}")
        ranks = {}
        for p in mods:
            j = _LORA_MODULES.index(p)
            for i in range(self.layers):
                A, Bm = tensors[f"l{i}.{p}.lora_A"], tensors[f"l{i}.{p}.lora_B"]
                r = A.shape[0]
                if not 1 <= r <= self.max_rank:
                    raise ValueError(f"l{i}.{p}: rank {r} outside 1..{self.max_rank} (the pack's max_rank)")
                if ranks.setdefault(p, r) != r:
                    raise ValueError(f"l{i}.{p}: rank {r} differs from layer 0's {ranks[p]} (per-layer ranks)")
                if tuple(A.shape) != (r, self.hidden) or tuple(Bm.shape) != (self.widths[j], r):
                    raise ValueError(f"l{i}.{p}: lora_A {tuple(A.shape)} / lora_B {tuple(Bm.shape)}; expected "
                                     f"({r}, {self.hidden}) / ({self.widths[j]}, {r})")
        pad = {p: -(-ranks[p] // LORA_GRAN) * LORA_GRAN for p in mods}
        self.seg[index].zero_()  # the slot serves as base while its rows change
        self.A[:, index].zero_()
        self.B[:, index].zero_()
        off, col = 0, 0
        for j, p in enumerate(_LORA_MODULES):
            if p in pad:
                for i in range(self.layers):
                    A = tensors[f"l{i}.{p}.lora_A"].to(self.device, torch.float32)
                    if gains is not None:
                        A = A * gains[i].to(self.device, torch.float32).view(1, -1)
                    self.A[i, index, off: off + ranks[p]] = A.to(torch.bfloat16)
                    self.B[i, index, col: col + self.widths[j], : ranks[p]] = tensors[f"l{i}.{p}.lora_B"].to(
                        self.device, torch.bfloat16)
                off += pad[p]
            col += self.widths[j]
        self.scale[index] = torch.tensor([float(scales.get(p, 0.0)) for p in _LORA_MODULES] + [0.0],
                                         dtype=torch.float32)
        self.seg[index] = torch.tensor([pad.get(p, 0) for p in _LORA_MODULES] + [0], dtype=torch.int32)
        self.loaded[index] = True


def pack_lora(layers: int, hidden: int, widths, max_adapters: int, max_rank: int, device) -> LoraPack:
    """An empty :class:`LoraPack`; adapters go in with :meth:`LoraPack.load`."""
    return LoraPack(layers, hidden, widths, max_adapters, max_rank, device)


def lora_split(B: int, S: int, K: int, rcap: int) -> int:
    """The K slices ``lora_qkv_`` runs the shrink with (host values only: safe under graph capture)."""
    return int(lib().mls_lora_split(int(B), int(S), int(K), int(rcap)))


def _lora_args(pack: LoraPack, layer: int, lora_slot: torch.Tensor, B: int, S: int, slot_ids, workspace, nsplit: int,
               dev) -> int:
    """The checks the two launches share; returns the split count."""
    _need(lora_slot, "lora_slot", torch.int32, dev)
    if slot_ids is not None:
        _need(slot_ids, "slot_ids", torch.int32, dev)
        if slot_ids.numel() != B:
            raise ValueError(f"slot_ids has {slot_ids.numel()} entries for {B} sequences")
    elif B > lora_slot.numel():
        raise ValueError(f"{B} sequences but lora_slot has {lora_slot.numel()} slots")
    if pack.A.device != dev:  # the arrays' device: "cuda" given at construction is cuda:0 here
        raise ValueError(f"pack lives on {pack.A.device}, the rows on {dev}")
    if not 0 <= int(layer) < pack.layers:
        raise ValueError(f"layer {layer} outside the pack's {pack.layers}")
    nsplit = int(nsplit) or lora_split(B, S, pack.hidden, pack.rcap)
    if nsplit < 1 or nsplit > 64 or pack.hidden % (nsplit * LORA_K_GRAN):
        raise ValueError(f"nsplit {nsplit}: hidden {pack.hidden} must be a multiple of nsplit * {LORA_K_GRAN}")
    _need(workspace, "workspace", torch.float32, dev)
    if workspace.numel() < pack.workspace_elems(B * S, nsplit):
        raise ValueError(f"workspace holds {workspace.numel()} floats, {nsplit} splits of {B * S} rows need "
                         f"{pack.workspace_elems(B * S, nsplit)}")
    return nsplit


def lora_shrink(resid: torch.Tensor, pack: LoraPack, layer: int, lora_slot: torch.Tensor, B: int, S: int,
                slot_ids: Optional[torch.Tensor] = None, *, workspace: torch.Tensor, nsplit: int = 0) -> int:
    """``mls_lora_shrink``: the split-K partials of ``t = resid . A'[a]^T`` and of each row's square sum into
    ``workspace`` (fp32 slabs ``[nsplit][B * S][pack.rcap + 1]``) for the rows whose sequence names an adapter.
    Returns the split count used (``nsplit = 0``: :func:`lora_split`)."""
    dev = resid.device
    _need(resid, "resid", torch.bfloat16, dev)
    if resid.dim() != 2 or tuple(resid.shape) != (B * S, pack.hidden):
        raise ValueError(f"resid is {tuple(resid.shape)}, expected ({B * S}, {pack.hidden})")
    nsplit = _lora_args(pack, layer, lora_slot, B, S, slot_ids, workspace, nsplit, dev)
    rc = lib().mls_lora_shrink(resid.data_ptr(), pack.hidden, pack.A[layer].data_ptr(), pack.seg.data_ptr(),
                               lora_slot.data_ptr(), _ptr(slot_ids), workspace.data_ptr(), workspace.numel() * 4, B, S,
                               pack.hidden, pack.rcap, pack.max_adapters, lora_slot.numel(), nsplit, stream_ptr(dev))
    check(rc, "mls_lora_shrink")
    return nsplit


def lora_expand_(qkv: torch.Tensor, pack: LoraPack, layer: int, lora_slot: torch.Tensor, B: int, S: int,
                 slot_ids: Optional[torch.Tensor] = None, *, eps: float = 1e-5, workspace: torch.Tensor,
                 nsplit: int = 0) -> torch.Tensor:
    """``mls_lora_expand``: ``qkv[m, seg_p] += s_p * rstd[m] * (t[m] . B_p[a]^T)`` in place from the slabs
    :func:`lora_shrink` wrote with the same arguments."""
    dev = qkv.device
    _need(qkv, "qkv", torch.bfloat16, dev)
    N = sum(pack.widths)
    if qkv.dim() != 2 or tuple(qkv.shape) != (B * S, N):
        raise ValueError(f"qkv is {tuple(qkv.shape)}; the pack's segment widths {pack.widths} need ({B * S}, {N})")
    nsplit = _lora_args(pack, layer, lora_slot, B, S, slot_ids, workspace, nsplit, dev)
    rc = lib().mls_lora_expand(qkv.data_ptr(), N, pack.B[layer].data_ptr(), pack.seg.data_ptr(),
                               pack.scale.data_ptr(), lora_slot.data_ptr(), _ptr(slot_ids), workspace.data_ptr(),
                               workspace.numel() * 4, B, S, pack.hidden, float(eps), *pack.widths, pack.rcap, pack.rb,
                               pack.max_adapters, lora_slot.numel(), nsplit, stream_ptr(dev))
    check(rc, "mls_lora_expand")
    return qkv


def lora_qkv_(qkv: torch.Tensor, resid: torch.Tensor, pack: LoraPack, layer: int, lora_slot: torch.Tensor, B: int,
              S: int, slot_ids: Optional[torch.Tensor] = None, *, eps: float = 1e-5,
              workspace: Optional[torch.Tensor] = None, nsplit: int = 0) -> torch.Tensor:
    """``qkv[m, seg_p] += s_p * B_p (A_p . RMSNorm(resid[m]) * gain)`` in place for the adapter of row m's
    sequence (``lora_slot[slot_ids[b] or b]``, -1: the row is left alone), layer ``layer`` of ``pack``:
    :func:`lora_shrink` then :func:`lora_expand_`, two launches.  ``workspace``: fp32,
    ``pack.workspace_elems(B * S, nsplit)`` elements (None: allocated here); ``nsplit = 0``: :func:`lora_split`."""
    N = sum(pack.widths)
    if qkv.dim() != 2 or tuple(qkv.shape) != (B * S, N):  # before anything is launched
        raise ValueError(f"qkv is {tuple(qkv.shape)}; the pack's segment widths {pack.widths} need ({B * S}, {N})")
    _need(qkv, "qkv", torch.bfloat16, qkv.device)
    if workspace is None:
        ns = int(nsplit) or lora_split(B, S, pack.hidden, pack.rcap)
        workspace = torch.empty(pack.workspace_elems(B * S, max(ns, 1)), device=qkv.device, dtype=torch.float32)
    nsplit = lora_shrink(resid, pack, layer, lora_slot, B, S, slot_ids, workspace=workspace, nsplit=nsplit)
    return lora_expand_(qkv, pack, layer, lora_slot, B, S, slot_ids, eps=eps, workspace=workspace, nsplit=nsplit)
