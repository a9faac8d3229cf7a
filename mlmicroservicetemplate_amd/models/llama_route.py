"""Which kernels one fused Llama forward runs: a pure function of the launch shape and of what the
model holds and has switched on -- host integers and booleans only (no torch: it runs inside graph
capture and must not touch a device tensor), so every measured threshold below is a unit-testable
rule (tests/test_llama_route_cpu.py).  ``models/llama.py`` asks once per step (:func:`step_route`)
and once more for the rows that reach the lm_head (:func:`proj_tiers`)."""
from dataclasses import dataclass


@dataclass(frozen=True)
class ProjTiers:
    """The weight copies a projection of ``rows`` activation rows may stream, best first: int4 codes,
    e4m3, granule-packed bf16, then the row-major matrix (fused-norm skinny GEMM while ``fuse``,
    RMSNorm + ``ops.linear`` above).  A copy is taken only if the model holds one of that matrix.  ``w8``
    stands apart: a ``weight_dtype="w8a8"`` model holds its layer matrices as e4m3 codes only, so that tier
    serves them at every row count (the lm_head, never quantised, walks the ladder without it)."""

    rows: int
    w4: bool
    fp8: bool
    packed: bool
    fuse: bool
    w8: bool = False  # weight_dtype="w8a8": the only copy of a layer matrix, at every row count

    def fp8_for(self, K: int) -> bool:
        """The e4m3 tier for a projection of inner size K: ops.skinny_fp8 takes rows * K bf16 activations
        of at most 64 KiB."""
        return self.fp8 and self.rows * K * 2 <= 65536


def proj_tiers(rows: int, have_packed: bool, have_w4: bool, have_fp8: bool, w4_max_rows: int,
               have_w8: bool = False) -> ProjTiers:
    return ProjTiers(
        # weight_dtype="w8a8": every layer projection, at every row count, is ops.quant_rows_fp8 +
        # ops.gemm_w8a8 on the e4m3 codes (the model holds nothing else of those matrices); the all-reduce
        # and the split-KV combine run as their own launches, as with int4.  Steps of <= 4 rows stay on it
        # too: ops.skinny_fp8 would need a second packed copy and was not measured ahead
        w8=have_w8,
        rows=rows,
        # weight_dtype="int4": the layer projections stream their 4-bit codes (ops.skinny_w4) instead;
        # no all-reduce tail / combine prologue there, so those run as separate launches.  Up to
        # w4_max_rows rows: the kernel's own limit (32), it was ahead of the bf16 routes at every row count
        # measured, 1 to 32 (Llama-3-8B, batch 32: 4.13 vs 4.50 ms/step; profiles/w4_decode_ab.jsonl,
        # docs/PERF_NOTES.md "W4A16 decode")
        w4=have_w4 and rows <= w4_max_rows,
        # opt-in FP8 decode (MLS_DECODE_FP8=1): W8A8 e4m3 copies (ops.skinny_fp8) for <= 4 tokens per step
        # -- half the weight stream (profiles/r2_decode_fp8_weight_probe.jsonl)
        fp8=have_fp8 and rows <= 4,
        # packed decode GEMMs up to 24 rows: at 25-32 (two 16-row A fragments per weight granule)
        # every column-tile block re-reads A, and the row-major split-K kernel is ahead (batch 24:
        # 4.99 vs 5.36 ms/step, batch 32: 5.75 vs 5.64; profiles/r2_llama8b_decode_packed_ab.jsonl)
        packed=have_packed and rows <= 24,
        # decode-shaped token counts: each pre-norm + residual add rides inside the skinny GEMM
        # (ops.gemm_rmsnorm); larger counts run a gain-free RMSNorm and ops.linear
        fuse=rows <= 16,
    )


@dataclass(frozen=True)
class StepRoute:
    """One forward's step-level decisions.  ``proj``: the projection ladder at the step's B * S rows."""

    proj: ProjTiers
    fold: bool          # residual adds in the o / down GEMM epilogues
    fuse_combine: bool  # split-KV combine in the o-projection's prologue
    ar_fuse: bool       # TP all-reduce in the row-parallel projections' epilogue
    fuse_rn: bool       # o / down through ops.linear_add_rmsnorm
    multi: bool         # verify step on ops.decode_attention_multi
    overlap: bool       # TP prefill as two interleaved batch halves
    dec_chunk: int      # decode split rows

    @property
    def fuse(self) -> bool:
        return self.proj.fuse

    @property
    def packed(self) -> bool:
        return self.proj.packed

    @property
    def w4(self) -> bool:
        return self.proj.w4

    @property
    def fp8(self) -> bool:
        return self.proj.fp8


def step_route(*, B: int, S: int, decode: bool, has_past: bool, all_rows: bool, tp: int, hq: int, hkv: int,
               head_dim: int, hidden: int, have_packed: bool, have_w4: bool, have_fp8: bool, o_packed: bool,
               o_fp8: bool, w4_max_rows: int, pk_fold: bool, prefill_fold: bool, fuse_combine: bool,
               fuse_add_norm: bool, ar_fuse: bool, tp_overlap: bool, verify_attn: str, spec_max_tokens: int,
               dec_chunk: int, ar_fusable: bool, capturing: bool, kv_fp8: bool = False,
               have_w8: bool = False) -> StepRoute:
    """``have_*``: the model holds such copies at all; ``o_packed`` / ``o_fp8``: of ``l0.o``;
    ``ar_fusable``: the comm's one-shot all-reduce can ride in a GEMM producing ``B * S * hidden``
    outputs; ``capturing``: the current stream is capturing a graph.  The rest are the model's
    dimensions on this rank and its switches under their own names; ``kv_fp8``: the cache is e4m3."""
    T = B * S
    proj = proj_tiers(T, have_packed, have_w4, have_fp8, w4_max_rows, have_w8)
    # TP = 1: the residual add rides in the o / down epilogues (h = r + a Wo^T, r' = h + g Wd^T), so
    # the next pre-norm GEMM reads one activation stream instead of two (r + delta) and writes no
    # residual copy.  With TP > 1 the add has to wait for the all-reduce.  prefill_fold: prefill at
    # TP = 1 with the residual add in the o / down GEMM epilogues too (the following RMSNorm then reads
    # one stream and writes one: 64 instead of 128 B per element)
    fold = tp == 1 and (((proj.packed or proj.w4 or proj.w8) and pk_fold) or (not decode and prefill_fold))
    # decode: the o-projection merges the split-KV partials in its prologue (one launch instead of
    # two) while every block's share of partials is small -- B x local q heads <= 32: one emulated
    # TP = 8 rank 1.166 -> 1.125 ms/token at batch 1, 1.294 -> 1.254 at 4; TP = 1 batch 1 level,
    # batch 4 (128 head rows per block) 3.17 -> 3.37, so off there (profiles/r2_llama8b_fused_combine_ab.jsonl)
    combine = (decode and fuse_combine and proj.packed and o_packed and not o_fp8 and B <= 4
               and B * hq <= 32 and B * hq * head_dim * 2 <= 65536)
    # TP > 1 decode: the row-parallel o / down projections run their all-reduce in their own
    # epilogue (ops.skinny_packed_ar / skinny_packed_combine_ar, csrc/ar_protocol.h): one launch
    # per projection + all-reduce instead of two, and each 2048-element chunk of the output is
    # reduced as soon as the blocks producing it finish.  MLS_AR_FUSE=0: separate kernels.
    ar = tp > 1 and ar_fusable and ar_fuse and proj.packed
    # TP = 1 above 24 tokens (no packed / fused-norm GEMMs): o_proj and down_proj leave their split-K
    # slabs to one kernel that adds them to the residual stream and normalises it for the next
    # projection (ops.linear_add_rmsnorm) -- one launch instead of reduce + RMSNorm, bit-identical.
    # A projection it cannot take (no split on that shape) runs the plain pair.
    fuse_rn = tp == 1 and not proj.packed and not proj.fuse and not fold and fuse_add_norm and not proj.w8
    # a verify step (all_rows: every row's candidates) of a few positions per sequence: its attention
    # runs split-KV on the matrix cores with the T positions x G heads of a KV head on one MFMA's lane
    # columns (ops.decode_attention_multi); MLS_VERIFY_ATTN=ctx keeps the chunk kernel (the A/B arm).
    # Chunked prefill (all_rows False) stays on flash_attention_ctx.  An e4m3 cache has no verify kernel
    # of its own: its verify steps take the context kernel too (ops.flash_attention_ctx_fp8, split-KV).
    multi = (has_past and all_rows and verify_attn != "ctx" and S <= spec_max_tokens
             and S * (hq // max(hkv, 1)) <= 16 and not kv_fp8)
    # TP prefill: two batch halves interleaved so each o / down all-reduce overlaps the other half's
    # compute (LlamaTP._prefill_overlapped); MLS_TP_OVERLAP=0 runs the plain layer loop
    overlap = not decode and not has_past and tp > 1 and B >= 2 and T >= 64 and tp_overlap and not capturing
    # decode split size: 64 rows measured best from batch 1 to 32, at TP = 1 and on an emulated
    # TP = 8 rank (one KV head).  A single 256-row split per KV head (no combine launch) was
    # 1.6 % slower at batch 1, and one 8-wave block walking a whole <= 1024 context in passes
    # was 26 % slower at TP = 8 (latency-bound on one CU) -- profiles/r1_llama_decode_sweep.jsonl.
    # From batch 32 up the grid is already >= 4k blocks and 128-row splits halve the combine
    # traffic: -3 % step time at batch 128 (profiles/r2_llama8b_decode_chunk_sweep.jsonl).
    chunk = dec_chunk if dec_chunk > 0 else (128 if B >= 32 else 64)
    return StepRoute(proj=proj, fold=bool(fold), fuse_combine=bool(combine), ar_fuse=bool(ar), fuse_rn=bool(fuse_rn),
                     multi=bool(multi), overlap=bool(overlap), dec_chunk=chunk)
