"""FP8 (e4m3) KV cache on the GPU (csrc/kv_fp8.hip): the prefill writer, decode attention on the
quantised cache (plain, RoPE + append, paged, captured in a graph) against ops.reference on the
dequantised cache, and the fused Llama with ``kv_dtype="fp8"`` against its reference-backend oracle."""
import pytest
import torch

import attn_cases as A
from mlmicroservicetemplate_amd.ops import reference as R
from test_kv_fp8_cpu import CFG128, D_REF, decode_top5_deviation, roundtrip_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
FUSED_VS_REF = 5e-2  # tests/test_models_gpu.py test_llama_fused_matches_reference_tiny: top-k logit values


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@pytest.fixture(scope="module")
def ops():
    from mlmicroservicetemplate_amd import ops as o

    o.lib()
    return o


def _fp8_cache(B, L, Hkv, seed):
    """Random bf16 rows quantised by the reference rule: head-major (k8, v8 [B, Hkv, L, D] uint8,
    ks, vs [B, Hkv, L] fp32) and the dequantised row-major fp32 caches [B, L, Hkv, D] of the oracle."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(2):
        x = torch.randn(B, L, Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
        q, s = R.kv_quant_fp8(x)
        out.append((q.permute(0, 2, 1, 3).contiguous(), s.permute(0, 2, 1).contiguous(), R.kv_dequant_fp8(q, s)))
    (k8, ks, kd), (v8, vs, vd) = out
    return k8, v8, ks, vs, kd, vd


def _deq_rows(c8, sc):
    """head-major (uint8 [B, Hkv, L, D], fp32 [B, Hkv, L]) -> dequantised row-major [B, L, Hkv, D]"""
    return R.kv_dequant_fp8(c8, sc).permute(0, 2, 1, 3)


def _paged_copy_hm(cache, pages_per_seq, num_pages, perm_seed=0):
    """tests/test_kv_pages_gpu.py _paged_copy for head-major tensors: [B, Hkv, L(, D)] contiguous ->
    (pool [num_pages, Hkv, 64(, D)], table [B, pages_per_seq]), pages scattered, page 0 scratch."""
    B = cache.shape[0]
    g = torch.Generator().manual_seed(perm_seed)
    order = (torch.randperm(num_pages - 1, generator=g) + 1)[: B * pages_per_seq]
    table = order.view(B, pages_per_seq).to(torch.int32)
    pool = torch.zeros((num_pages, cache.shape[1], 64) + tuple(cache.shape[3:]), device=cache.device, dtype=cache.dtype)
    for b in range(B):
        for p in range(pages_per_seq):
            pool[int(table[b, p])] = cache[b, :, p * 64:(p + 1) * 64]
    return pool, table.to(cache.device)


# ------------------------------------------------------------------------------- 1. writer
def _check_written(k8, ks, kh, written):
    """k8 / ks against the bf16 rows kh that rope_kv_ wrote ([blocks, Hkv, R, D]); `written`: bool [blocks, R]"""
    x = kh.float()
    deq = R.kv_dequant_fp8(k8, ks)
    w = written.unsqueeze(1).expand(-1, kh.shape[1], -1)  # [blocks, Hkv, R]
    assert w.any()
    assert ((deq - x).abs() <= roundtrip_bound(x, ks))[w].all()
    want = torch.clamp(x.abs().amax(-1), min=2.0 ** -40) / 448
    assert torch.allclose(ks[w], want[w], rtol=1e-6, atol=0)
    q_ref, s_ref = R.kv_quant_fp8(x.cpu())  # the rule itself, evaluated on the CPU: the very bytes and scales
    print("bytes differing from the reference:", int((k8.cpu() != q_ref)[w.cpu()].sum()),
          "scales:", int((ks.cpu() != s_ref)[w.cpu()].sum()))
    assert torch.equal(k8.cpu()[w.cpu()], q_ref[w.cpu()]) and torch.equal(ks.cpu()[w.cpu()], s_ref[w.cpu()])
    assert not k8[~w].any() and not ks[~w].any()  # everything else untouched


@pytest.mark.parametrize("R_", [64, 128])
def test_writer_explicit_slots(ops, R_):
    torch.manual_seed(12)
    T, Hq, Hkv, MS = 6, 8, 2, 128
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    slots = torch.tensor([0, 5, 127, 128, 200, -1], device=DEV, dtype=torch.int32)
    pos = torch.tensor([0, 5, 127, 0, 72, 3], device=DEV, dtype=torch.int32)
    cos, sin = R.rope_tables(256, D, 500000.0, DEV)
    kh = torch.zeros(2 * MS // R_, Hkv, R_, D, device=DEV, dtype=torch.bfloat16)
    vh = torch.zeros_like(kh)
    k8 = torch.zeros(kh.shape, device=DEV, dtype=torch.uint8)
    v8 = torch.zeros_like(k8)
    ks = torch.zeros(kh.shape[:3], device=DEV, dtype=torch.float32)
    vs = torch.zeros_like(ks)
    q1, q2 = qkv.clone(), qkv.clone()
    ops.rope_kv_(q1, pos, cos, sin, Hq, Hkv, D, slots, kh, vh, hm_rows=R_)
    ops.rope_kv_fp8_(q2, pos, cos, sin, Hq, Hkv, D, slots, k8, v8, ks, vs, hm_rows=R_)
    assert torch.equal(q1, q2)
    written = torch.zeros(2 * MS, dtype=torch.bool, device=DEV)
    written[slots[slots >= 0].long()] = True
    written = written.view(-1, R_)
    _check_written(k8, ks, kh, written)
    _check_written(v8, vs, vh, written)


def test_writer_derived_slots(ops):
    torch.manual_seed(13)
    B, S, Hq, Hkv, MS = 2, 3, 8, 2, 128
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    pos = torch.tensor([0, 1, 2, 0, 1, 2], device=DEV, dtype=torch.int32)
    lens = torch.tensor([3, 2], device=DEV, dtype=torch.int32)  # the second sequence is padded
    cos, sin = R.rope_tables(256, D, 500000.0, DEV)
    kh = torch.zeros(B, Hkv, MS, D, device=DEV, dtype=torch.bfloat16)
    vh = torch.zeros_like(kh)
    k8 = torch.zeros(kh.shape, device=DEV, dtype=torch.uint8)
    v8 = torch.zeros_like(k8)
    ks = torch.zeros(kh.shape[:3], device=DEV, dtype=torch.float32)
    vs = torch.zeros_like(ks)
    q1, q2 = qkv.clone(), qkv.clone()
    ops.rope_kv_(q1, pos, cos, sin, Hq, Hkv, D, None, kh, vh, lens=lens, seq=S, max_seq=MS, hm_rows=MS)
    ops.rope_kv_fp8_(q2, pos, cos, sin, Hq, Hkv, D, None, k8, v8, ks, vs, lens=lens, seq=S, max_seq=MS)
    assert torch.equal(q1, q2)
    written = torch.zeros(B, MS, dtype=torch.bool, device=DEV)
    written[0, :3] = True
    written[1, :2] = True
    _check_written(k8, ks, kh, written)
    _check_written(v8, vs, vh, written)


# ------------------------------------------------------------------------------- 2. decode, plain
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (32, 8), (8, 1), (4, 2), (2, 2)])  # G = 4, 4, 8, 2, 1
@pytest.mark.parametrize("chunk", [64, 128])
def test_decode_plain(ops, Hq, Hkv, chunk):
    B, max_len = 5, 512
    k8, v8, ks, vs, kd, vd = _fp8_cache(B, max_len, Hkv, seed=5)
    torch.manual_seed(5)
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    lens = torch.tensor([1, 64, 65, 300, 512], device=DEV, dtype=torch.int32)
    cnt = torch.zeros(B * Hkv, device=DEV, dtype=torch.int32)
    ref = R.decode_attention(q, kd, vd, lens, Hq, Hkv, D)
    tol = A.tolerance(A.rows_decode(q, kd, vd, lens, Hq, Hkv, D), D)  # per (row, head): tests/attn_cases.py
    for _ in range(3):
        out = ops.decode_attention_fp8(q, k8, v8, ks, vs, lens, Hq, Hkv, D, chunk=chunk, counters=cnt)
        print("plain rel", rel(out, ref))
        assert rel(out, ref) < 2e-2
        assert A.head_err(out, ref, D).max() < tol
    assert not cnt.any()
    # combine=False + the o-projection's fused combine == combine=True + the plain packed GEMM
    # (tests/test_skinny_packed_gpu.py test_packed_combine_matches_attention_then_gemm, M <= 4 rows)
    M, N = 4, 256
    w = (torch.randn(N, Hq * D, device=DEV) * (Hq * D) ** -0.5).to(torch.bfloat16)
    wp = ops.pack_skinny(w)
    args = (q[:M], k8[:M], v8[:M], ks[:M], vs[:M], lens[:M], Hq, Hkv, D)
    a_ref = ops.decode_attention_fp8(*args, chunk=chunk)
    assert torch.equal(a_ref, out[:M])
    a, parts = ops.decode_attention_fp8(*args, chunk=chunk, combine=False)
    assert isinstance(parts, ops.DecodePartials) and parts.chunk == chunk
    single = (lens[:M] <= chunk)
    assert torch.equal(a[single], a_ref[single])  # rows of one split are written directly
    got = ops.skinny_packed_combine(a, parts, wp, N)
    assert rel(got, ops.skinny_packed(a_ref, wp, N)) < 1e-2


@pytest.mark.parametrize("L,max_len", [(700, 704), (8257, 8320)])
def test_decode_plain_many_splits(ops, L, max_len):
    """The split combine beyond test_decode_plain's 8 splits: 11 splits run its blocks of 8 plus the
    remainder loop, 130 splits (> D, the block's threads) a second trip of its strided (m, l) passes."""
    B, Hq, Hkv, chunk = 1, 4, 1, 64
    k8, v8, ks, vs, kd, vd = _fp8_cache(B, max_len, Hkv, seed=7)
    torch.manual_seed(7)
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    lens = torch.tensor([L], device=DEV, dtype=torch.int32)
    ref = R.decode_attention(q, kd, vd, lens, Hq, Hkv, D)
    out = ops.decode_attention_fp8(q, k8, v8, ks, vs, lens, Hq, Hkv, D, chunk=chunk)
    print("many splits rel", rel(out, ref))
    assert rel(out, ref) < 2e-2
    assert A.head_err(out, ref, D).max() < A.tolerance(A.rows_decode(q, kd, vd, lens, Hq, Hkv, D), D)


# ------------------------------------------------------------------------------- 3. rope + append
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (32, 8), (8, 1)])
@pytest.mark.parametrize("chunk", [64, 128])
def test_decode_rope_append(ops, Hq, Hkv, chunk):
    B, max_len = 4, 512
    k8, v8, ks, vs, _, _ = _fp8_cache(B, max_len, Hkv, seed=6)
    torch.manual_seed(6)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    lens = torch.tensor([1, 77, 129, 512], device=DEV, dtype=torch.int32)
    pos = lens - 1
    cos, sin = R.rope_tables(max_len, D, 500000.0, DEV)
    k2, v2, ks2, vs2, qkv2 = k8.clone(), v8.clone(), ks.clone(), vs.clone(), qkv.clone()
    k0, ks0 = k8.clone(), ks.clone()
    ops.rope_kv_fp8_(qkv2, pos, cos, sin, Hq, Hkv, D, None, k2, v2, ks2, vs2, lens=lens, seq=1, max_seq=max_len)
    out = ops.decode_attention_fp8(qkv, k8, v8, ks, vs, lens, Hq, Hkv, D, positions=pos, cos=cos, sin=sin, chunk=chunk)
    # the shared-writer contract: the appended bytes and scales are the prefill writer's, nothing else moved
    assert not torch.equal(k2, k0) and not torch.equal(ks2, ks0)  # (the writer did write)
    assert torch.equal(k8, k2) and torch.equal(v8, v2)
    assert torch.equal(ks, ks2) and torch.equal(vs, vs2)
    ref = R.decode_attention(qkv2, _deq_rows(k8, ks), _deq_rows(v8, vs), lens, Hq, Hkv, D)
    print("rope rel", rel(out, ref))
    assert rel(out, ref) < 1e-2
    rows = A.rows_decode(qkv2, _deq_rows(k8, ks), _deq_rows(v8, vs), lens, Hq, Hkv, D)
    assert A.head_err(out, ref, D).max() < A.tolerance(rows, D)


# ------------------------------------------------------------------------------- 4. paged == contiguous
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (32, 8)])
def test_paged_equals_contiguous(ops, Hq, Hkv):
    B, max_len = 5, 512
    k8, v8, ks, vs, _, _ = _fp8_cache(B, max_len, Hkv, seed=5)
    torch.manual_seed(5)
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    lens = torch.tensor([1, 64, 65, 300, 512], device=DEV, dtype=torch.int32)
    pos = lens - 1
    cos, sin = R.rope_tables(max_len, D, 500000.0, DEV)
    n = max_len // 64
    pools = [_paged_copy_hm(t, n, 50, 1) for t in (k8, v8, ks, vs)]
    table = pools[0][1]
    kp, vp, ksp, vsp = (p[0] for p in pools)
    want = ops.decode_attention_fp8(q, k8, v8, ks, vs, lens, Hq, Hkv, D, chunk=64)
    got = ops.decode_attention_fp8(q, kp, vp, ksp, vsp, lens, Hq, Hkv, D, chunk=64, page_table=table)
    assert torch.equal(got, want)
    kw = dict(positions=pos, cos=cos, sin=sin, chunk=64)
    want = ops.decode_attention_fp8(q, k8, v8, ks, vs, lens, Hq, Hkv, D, **kw)
    got = ops.decode_attention_fp8(q, kp, vp, ksp, vsp, lens, Hq, Hkv, D, page_table=table, **kw)
    assert torch.equal(got, want)
    for b in range(B):  # the appended row landed in the right page
        p_ = int(pos[b])
        page = int(table[b, p_ // 64])
        assert torch.equal(kp[page, :, p_ % 64], k8[b, :, p_]) and torch.equal(vp[page, :, p_ % 64], v8[b, :, p_])
        assert torch.equal(ksp[page, :, p_ % 64], ks[b, :, p_]) and torch.equal(vsp[page, :, p_ % 64], vs[b, :, p_])
    # and nothing else in the pool moved
    for pool, cache in ((kp, k8), (vp, v8), (ksp, ks), (vsp, vs)):
        assert torch.equal(pool, _paged_copy_hm(cache, n, 50, 1)[0])


# ------------------------------------------------------------------------------- 5. bad geometry
def test_bad_geometry_raises_before_launch(ops):
    def caches(blocks, hkv, rows, d=D):
        c = torch.zeros(blocks, hkv, rows, d, device=DEV, dtype=torch.uint8)
        s = torch.zeros(blocks, hkv, rows, device=DEV, dtype=torch.float32)
        return c, c.clone(), s, s.clone()

    lens = torch.ones(1, device=DEV, dtype=torch.int32)
    q = torch.zeros(1, 18 * D, device=DEV, dtype=torch.bfloat16)
    k, v, ks, vs = caches(1, 1, 64, 64)
    with pytest.raises(ValueError):  # D = 64
        ops.decode_attention_fp8(q, k, v, ks, vs, lens, 4, 1, 64)
    k, v, ks, vs = caches(1, 1, 64)
    with pytest.raises(ValueError):  # G = 16
        ops.decode_attention_fp8(q, k, v, ks, vs, lens, 16, 1, D)
    rm = torch.zeros(1, 64, 2, D, device=DEV, dtype=torch.uint8)  # row-major [B, rows, Hkv, D]
    rs = torch.zeros(1, 64, 2, device=DEV, dtype=torch.float32)
    with pytest.raises(ValueError):
        ops.decode_attention_fp8(q, rm, rm, rs, rs, lens, 4, 2, D)
    k, v, ks, vs = caches(4, 1, 32)
    with pytest.raises(ValueError):  # 32-row pages, chunk 64
        ops.decode_attention_fp8(q, k, v, ks, vs, lens, 4, 1, D, chunk=64,
                                 page_table=torch.zeros(1, 2, device=DEV, dtype=torch.int32))
    k, v, ks, vs = caches(1, 1, 64)
    with pytest.raises(ValueError):  # scale tensor of the wrong shape
        ops.decode_attention_fp8(q, k, v, ks[:, :, :60].contiguous(), vs, lens, 4, 1, D)
    with pytest.raises(ValueError):  # chunk 256: the bf16 kernel's, not this one's
        ops.decode_attention_fp8(q, k, v, ks, vs, lens, 4, 1, D, chunk=256)
    # the writer checks the same layout
    cos, sin = R.rope_tables(64, D, 500000.0, DEV)
    pos = torch.zeros(1, device=DEV, dtype=torch.int32)
    qkv = torch.zeros(1, 8 * D, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.rope_kv_fp8_(qkv, pos, cos, sin, 4, 2, D, pos, rm, rm, rs, rs)
    k2, v2, ks2, vs2 = caches(1, 2, 64)
    with pytest.raises(ValueError):
        ops.rope_kv_fp8_(qkv, pos, cos, sin, 4, 2, D, pos, k2, v2, ks2.view(1, 64, 2), vs2)
    assert not k2.any() and not ks2.any()


# ------------------------------------------------------------------------------- 6. graph replay
def test_graph_replay_across_a_split_boundary(ops):
    B, L, Hq, Hkv = 2, 256, 8, 2
    k8, v8, ks, vs, _, _ = _fp8_cache(B, L, Hkv, seed=7)
    torch.manual_seed(7)
    steps = [torch.randn(B, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16) for _ in range(3)]
    lens0 = torch.tensor([63, 190], device=DEV, dtype=torch.int32)  # -> 64 | 65 (second split), 191 | 192 | 193
    cos, sin = R.rope_tables(L, D, 500000.0, DEV)

    def run(qkv, caches, lens, pos, **kw):
        return ops.decode_attention_fp8(qkv, *caches, lens, Hq, Hkv, D, positions=pos, cos=cos, sin=sin, chunk=64,
                                        max_len=L, **kw)

    # eager sequence
    eager = [t.clone() for t in (k8, v8, ks, vs)]
    lens, want = lens0.clone(), []
    for qkv in steps:
        lens += 1
        want.append(run(qkv, eager, lens, lens - 1).clone())
    # captured step on static tensors
    static = [t.clone() for t in (k8, v8, ks, vs)]
    s_qkv, s_lens, s_pos = steps[0].clone(), lens0 + 1, lens0.clone()
    kw = dict(workspace=torch.empty(B * Hq * (L // 64) * (D + 2), device=DEV, dtype=torch.float32),
              counters=torch.zeros(B * Hkv, device=DEV, dtype=torch.int32),
              out=torch.empty(B, Hq * D, device=DEV, dtype=torch.bfloat16))
    run(s_qkv, static, s_lens, s_pos, **kw)  # warm-up outside the capture, then the caches are restored
    torch.cuda.synchronize()
    for t, src in zip(static, (k8, v8, ks, vs)):
        t.copy_(src)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s_out = run(s_qkv, static, s_lens, s_pos, **kw)
    for t, src in zip(static, (k8, v8, ks, vs)):  # a capture launches nothing, but start from the same state anyway
        t.copy_(src)
    for i, qkv in enumerate(steps):
        s_qkv.copy_(qkv)
        if i:
            s_lens += 1
            s_pos += 1
        g.replay()
        assert torch.equal(s_out, want[i])
    torch.cuda.synchronize()
    for a, b in zip(static, eager):
        assert torch.equal(a, b)
    assert not kw["counters"].any()


# ------------------------------------------------------------------------------- 7. model
@pytest.fixture(scope="module")
def tiny():
    from mlmicroservicetemplate_amd.models.llama import init_llama_shard, tiny_config

    cfg = tiny_config(**CFG128)
    return cfg, init_llama_shard(cfg, 1, 0, seed=5, device=DEV)


def _prompts():
    ids = torch.randint(3, 2000, (2, 20), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(DEV)
    return ids, torch.tensor([20, 20], dtype=torch.int32, device=DEV)


def test_model_fused_fp8_vs_reference_fp8(tiny):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    ids, lens = _prompts()
    ref = LlamaTP(p, cfg, backend="reference", device=DEV, max_batch=2, max_seq=64, kv_dtype="fp8")
    fus = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, kv_dtype="fp8")
    dev = decode_top5_deviation(fus, ref, ids, lens)
    print("fused fp8 vs reference fp8:", dev)
    assert dev < FUSED_VS_REF


def test_model_fused_fp8_vs_fused_bf16(tiny):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    ids, lens = _prompts()
    b16 = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64)
    fp8 = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, kv_dtype="fp8")
    dev = decode_top5_deviation(fp8, b16, ids, lens)
    print("fused fp8 vs fused bf16:", dev)
    assert dev <= 2 * D_REF + FUSED_VS_REF


def test_model_cache_bytes(tiny):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    for kv_pages in (0, 9):
        b16 = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=4, max_seq=256, kv_pages=kv_pages)
        fp8 = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=4, max_seq=256, kv_pages=kv_pages, kv_dtype="fp8")
        nbytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)  # noqa: E731
        bf16_bytes = nbytes(b16.k_cache + b16.v_cache)
        assert fp8.k_cache[0].dtype == torch.uint8 and fp8.k_scale[0].shape == fp8.k_cache[0].shape[:3]
        assert nbytes(fp8.k_cache + fp8.v_cache + fp8.k_scale + fp8.v_scale) * 256 == bf16_bytes * (128 + 4)


def test_model_bad_geometry(tiny, monkeypatch):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP, init_llama_shard, tiny_config

    cfg, p = tiny
    with pytest.raises(ValueError):
        LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, kv_dtype="int4")
    cfg64 = tiny_config(layers=1, hidden=256, heads=4, kv_heads=2, head_dim=64, intermediate=512)
    with pytest.raises(ValueError):
        LlamaTP(init_llama_shard(cfg64, 1, 0, seed=1, device=DEV), cfg64, backend="fused", device=DEV, max_batch=2,
                max_seq=64, kv_dtype="fp8")
    monkeypatch.setenv("MLS_KV_HEAD_MAJOR", "0")
    with pytest.raises(ValueError):
        LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, kv_dtype="fp8")


def test_model_decode_runs_the_fp8_kernel(tiny, monkeypatch):
    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    ids, lens = _prompts()
    m = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, kv_dtype="fp8")
    m.use_graphs = False  # eager decode so the counters see the calls
    calls = {"fp8": 0, "bf16": 0}
    real8, real16 = ops.decode_attention_fp8, ops.decode_attention

    def spy8(*a, **k):
        calls["fp8"] += 1
        return real8(*a, **k)

    def spy16(*a, **k):
        calls["bf16"] += 1
        return real16(*a, **k)

    monkeypatch.setattr(ops, "decode_attention_fp8", spy8)
    monkeypatch.setattr(ops, "decode_attention", spy16)
    pos = torch.arange(20, device=DEV, dtype=torch.int32).unsqueeze(0).expand(2, 20).contiguous()
    m.step(ids, pos, lens, decode=False, k=5)
    assert calls == {"fp8": 0, "bf16": 0}
    tok = torch.tensor([[7], [9]], device=DEV, dtype=torch.int32)
    m.decode_step(tok, lens.view(2, 1).clone(), 5, max_ctx=21)
    assert calls == {"fp8": cfg.layers, "bf16": 0}


def test_model_paged_matches_per_slot(tiny):
    from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    cfg, p = tiny
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(3, 2000, (3, 90), generator=g)
    lens = torch.tensor([90, 33, 4])
    gp = GenParams(max_new_tokens=10)
    want = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=4, max_seq=256, kv_dtype="fp8").generate(ids, lens, gp)
    paged = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=4, max_seq=256, kv_pages=9, kv_dtype="fp8")
    got = paged.generate(ids, lens, gp)
    assert torch.equal(got, want)
    eng = ContinuousLlama(paged)
    futs = [eng.submit(ids[b, : int(lens[b])].tolist(), gp) for b in range(3)]
    eng.start()  # all three admitted by the first iteration: the same [3, 90] prefill as generate()
    outs = [f.result(timeout=120) for f in futs]
    eng.stop()
    eos = set(cfg.eos_ids)
    for b in range(3):
        w = want[b].tolist()
        cut = next((i + 1 for i, t in enumerate(w) if t in eos), len(w))
        assert outs[b] == w[:cut]
    assert paged.pages.free_pages == 8
