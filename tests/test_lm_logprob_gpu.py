"""csrc/lm_logprob.hip (``ops.linear_logprob``) against float64 on the same bf16 inputs, and ``LlamaTP.score`` fused
against the reference backend.

Bound on ``|d log p|``, derived (u = 2^-24):
  * a logit is K products summed in fp32, at most K sequential additions: ``|dl_n| <= E_n = K u sum_k |x_k w_nk|``;
    ``t`` moves by at most ``E = max_n E_n`` and so does the log-sum-exp (1-Lipschitz in the sup norm): ``2 E``;
  * ``exp(l - m)``: the fp32 subtraction and ``__expf``'s scaling by log2 e each cost ``|l - m| u`` relative, v_exp_f32
    one ulp more: ``(2 |l - m| + 2) u <= 178 u`` for a term that does not underflow (``|l - m| <= 88``); the wave ->
    block and tile -> row folds rescale by ``exp(m_i - m)`` once each: ``3 * 178 u``.  The sums are fewer than 64
    sequential additions (16 per lane, 2 lane swaps, 4 waves, ceil(tiles / 64) per lane and 6 steps in the merge):
    ``64 u``.  ``d log s = ds / s``: ``EXP = (3 * 178 + 64) u = 3.6e-5``.
The test forms ``t - m - log s`` in float64 from the fp32 triple, so nothing else rounds.

Inputs that expose a lost or double-counted tile: row r's logits are N(0, ~1.5) but for one column near 12, placed in
tile ``(r + tiles - 1) % tiles`` (row 0: the ragged last tile) at a varying offset.  ``_case`` checks on the float64
reference alone that dropping that tile, or counting it twice, moves the row's log-sum-exp by over 100 bounds.
``WALK`` holds the one shape at which a block walks several tiles (more tiles than the device has CUs) and the merge
folds more than 64 tiles per row; there the dominant logit is raised by ``log(N / 536)`` so it still dominates.

Not crossed: ``lo`` follows a parity of (M, N, tail), so both values occur but a given (M, N, valid) runs with one of
them; M = 1 has only the first target kind (the first column of the last tile).  Every call passes ``vocab`` well
above the deliberate out-of-shard targets, so the file also runs against a ``-DMLS_DEBUG`` build (the default
``vocab = lo + N`` would report them as code 515)."""
import functools
import math

import pytest
import torch

from mlmicroservicetemplate_amd import ops
from mlmicroservicetemplate_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BN, BM_S, BM_L = ops.LOGPROB_BN, 64, 256  # the column tile and the two row tiles (M <= 128: the small one)
U = 2.0 ** -24
EXP = (3 * 178 + 64) * U
NINF = float("-inf")

CASES = [(M, N, 256, tail, 1000 * ((M + N // 8 + tail) % 2))
         for M in (1, 17, BM_S + 1, BM_L + 1) for N in (BN, BN + 8, 2 * BN + 24) for tail in (0, 5)]
CASES.append((17, BN + 8, 128, 5, 1000))  # one ring step fewer: K = 128 is two k-steps, 256 four
# 161 column tiles: 2 x 161 = 322 (tile by M) and 5 x 161 = 805 (64-row tile forced) tiles on <= 304 CUs, so blocks
# cross tile ends with the loader already in the next tile, in the XCD-remapped order; the merge strides 161 > 64
WALK_N = 160 * BN + 24
WALK = [(BM_S + 1, 0), (BM_L + 1, 0), (BM_L + 1, 2), (BM_S + 1, 1)]  # (M, tile): by M, by M, 64 rows, 256 rows


@functools.lru_cache(maxsize=None)
def _case(M, N, K, tail, lo):
    """bf16 inputs, targets, and from float64 alone: log p (``-inf`` where no column is scored), the row's
    log-sum-exp, and the bounds ``(2 E + EXP, E + EXP)``."""
    valid, tiles = N - tail, -(-N // BN)
    g = torch.Generator().manual_seed(1000 * M + N + K + tail)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    r = torch.arange(M)
    tile = (r + tiles - 1) % tiles
    t_lo, t_hi = tile * BN, torch.minimum((tile + 1) * BN, torch.tensor(valid))
    dom = t_lo + (r * 37) % (t_hi - t_lo)
    wd = w[dom].float()
    peak = 12.0 + max(0.0, math.log(N / 536))  # the other columns' log-sum-exp grows by log N
    x = (torch.randn(M, K, generator=g) + peak * wd / wd.pow(2).sum(1, keepdim=True)).bfloat16()
    outside = torch.where((r // 8) % 2 == 0 if lo else r >= 0, torch.tensor(N + 3), torch.tensor(-5))
    col = torch.stack([torch.full((M,), (tiles - 1) * BN), torch.full((M,), BN - 1), torch.full((M,), valid - 1),
                       torch.full((M,), valid), outside, torch.zeros(M, dtype=torch.long), dom,
                       (r * 101) % valid])[r % 8, r]  # first / last of a tile, last valid, tail, outside, -1, ...
    targets = torch.where(r % 8 == 5, torch.tensor(-1), lo + col).to(torch.int32)
    logits = x.double() @ w.double().T
    logits[:, valid:] = NINF
    scored = (r % 8 != 5) & (col >= 0) & (col < valid)
    want = torch.where(scored, torch.log_softmax(logits, 1).gather(1, col.clamp(0, N - 1).unsqueeze(1)).squeeze(1),
                       torch.tensor(NINF, dtype=torch.float64))
    lse = torch.logsumexp(logits, 1)
    E = K * U * (x.double().abs() @ w.double().abs().T)[:, :valid].max(1).values
    bound = 2 * E + EXP
    # every tile is some row's dominant one (while there are rows enough), and losing or doubling it shows
    assert len(set(tile.tolist())) == min(M, tiles)
    in_tile = (torch.arange(N) // BN).unsqueeze(0) == tile.unsqueeze(1)
    lse_tile = torch.logsumexp(logits.masked_fill(~in_tile, NINF), 1)
    lse_rest = torch.logsumexp(logits.masked_fill(in_tile, NINF), 1)
    assert (lse - lse_rest > 100 * bound).all() and (torch.logaddexp(lse, lse_tile) - lse > 100 * bound).all()
    return x, w, targets, want, lse, bound, E + EXP


def _run(x, w, targets, fill=float("nan"), **kw):
    ws = torch.full((ops.logprob_workspace_elems(x.shape[0], w.shape[0]),), fill, device=DEV)
    kw.setdefault("vocab", 1 << 30)
    return ops.linear_logprob(x.to(DEV), w.to(DEV), targets.to(DEV), workspace=ws, **kw)


def _worst(out, want, lse, bound, lse_bound):
    """The largest error / bound ratio of log p and of the log-sum-exp; unscored rows must hold t = -inf exactly."""
    m, s, t = out.double().cpu().unbind(1)
    scored = want > NINF
    assert (t[~scored] == NINF).all() and torch.isfinite(t[scored]).all()
    got = (t - m - torch.log(s))[scored]
    return max(float(((got - want[scored]).abs() / bound[scored]).max()) if scored.any() else 0.0,
               float(((m + torch.log(s) - lse).abs() / lse_bound).max()))


@pytest.mark.parametrize("M,N,K,tail,lo", CASES)
def test_against_float64(M, N, K, tail, lo):
    x, w, targets, *judge = _case(M, N, K, tail, lo)
    worst = _worst(_run(x, w, targets, lo=lo, valid=N - tail), *judge)
    print(f"M={M} N={N} K={K} valid={N - tail} lo={lo}: {worst:.3f} of the bound")
    assert worst <= 1.0


@pytest.mark.parametrize("M,tile", WALK)
def test_blocks_walk_several_tiles(M, tile):
    x, w, targets, *judge = _case(M, WALK_N, 128, 5, 1000)
    worst = _worst(_run(x, w, targets, lo=1000, valid=WALK_N - 5, tile=tile), *judge)
    print(f"M={M} N={WALK_N} K=128 tile={tile}: {worst:.3f} of the bound")
    assert worst <= 1.0


def test_two_shards_merge_to_the_unsharded_result():
    M, N, n0 = BM_S + 1, 2 * BN + 24, BN + 8
    x, w, targets, want, _, bound, _ = _case(M, N, 256, 0, 0)
    whole = _run(x, w, targets)
    parts = torch.stack([_run(x, w[:n0].contiguous(), targets), _run(x, w[n0:].contiguous(), targets, lo=n0)])
    got, one = R.logprob_merge(parts.double().cpu()), R.logprob_merge(whole[None].double().cpu())
    scored = want > NINF
    assert torch.equal(got[~scored], want[~scored])
    assert ((got - want)[scored].abs() <= bound[scored]).all()
    assert ((got - one)[scored].abs() <= 2 * EXP).all()  # the same logits, folded in another grouping


def test_runs_are_bit_identical_and_capturable():
    M, N = BM_L + 1, 2 * BN + 24
    x, w, targets, *_ = _case(M, N, 256, 5, 1000)
    eager = _run(x, w, targets, lo=1000, valid=N - 5)
    assert torch.equal(eager, _run(x, w, targets, fill=0.0, lo=1000, valid=N - 5))
    xd, wdev, td = x.to(DEV), w.to(DEV), targets.to(DEV)
    ws = torch.empty(ops.logprob_workspace_elems(M, N), device=DEV)
    out = torch.empty(M, 3, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.linear_logprob(xd, wdev, td, lo=1000, valid=N - 5, workspace=ws, out=out, vocab=1 << 30)
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_unsupported_k_is_an_error():
    x, w, targets, *_ = _case(17, BN + 8, 128, 5, 1000)
    with pytest.raises(ops.NativeError):
        _run(x[:, :64].contiguous(), w[:, :64].contiguous(), targets)


def test_out_and_workspace_sizes_are_checked():
    x, w, targets, *_ = _case(17, BN + 8, 128, 5, 1000)
    for shape in ((16, 3), (17, 2), (51,)):  # the merge writes M * 3 floats: anything but [M, 3] is refused
        with pytest.raises(ValueError):
            _run(x, w, targets, out=torch.empty(shape, device=DEV))
    with pytest.raises(ValueError):
        ops.linear_logprob(x.to(DEV), w.to(DEV), targets.to(DEV), workspace=torch.empty(8, device=DEV))


@pytest.mark.parametrize("weight_dtype", ["bf16", "int4", "w8a8"])
def test_model_score_fused_matches_reference(weight_dtype):
    """Tolerance from what tests/test_models_gpu.py already allows between the two backends' logits, not from the
    code under test: there ``max |dlogit| < 5e-2 max |logit|``; log p = t - lse moves by at most twice a logit's error,
    so ``2 * 5e-2 * max |logit|`` with the reference's own last-token logits as the scale.  Measured on MI355X:
    the worst |d log p| is 0.060 (bf16), 0.050 (int4) and 0.302 (w8a8) of that tolerance."""
    from mlmicroservicetemplate_amd.models.llama import LlamaTP, init_llama_shard, tiny_config

    cfg = tiny_config(layers=3, hidden=512, heads=4, kv_heads=1, head_dim=128, intermediate=1024, vocab=16384)
    p = init_llama_shard(cfg, 1, 0, seed=3, device=DEV)
    kw = dict(device=DEV, max_batch=4, max_seq=128, weight_dtype=weight_dtype)
    ref, fus = LlamaTP(p, cfg, backend="reference", **kw), LlamaTP(p, cfg, backend="fused", **kw)
    B, S = 3, 70
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab - 1, (B, S), device=DEV, dtype=torch.int32)
    lens = torch.tensor([70, 41, 5], device=DEV, dtype=torch.int32)
    want = ref.score(ids, lens)
    ref.keep_logits = True
    ref.step(ids, torch.arange(S, device=DEV, dtype=torch.int32).expand(B, S).contiguous(), lens, decode=False, k=1)
    tol = 2 * 5e-2 * float(ref.last_logits.abs().max())
    fus.score(ids, lens)  # first use allocates what later calls keep
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = fus.score(ids, lens)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    err = float((got - want).abs().max())
    print(f"{weight_dtype}: max |d log p| {err:.4f}, tolerance {tol:.4f} ({err / tol:.3f}); peak {peak} B")
    assert peak < B * S * cfg.vocab * 2  # no [rows, vocab] tensor, even in bf16
    assert got.shape == (B, S) and err <= tol
    pad = torch.arange(S, device=DEV).unsqueeze(0) >= lens.unsqueeze(1)
    assert (got[:, 0] == 0).all() and (got[pad] == 0).all() and (got[~pad][want[~pad] != 0] != 0).all()
