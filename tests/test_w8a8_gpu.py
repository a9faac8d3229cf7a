"""csrc/gemm_w8a8.hip on the GPU: the activation-row quantiser (mls_quant_rows_fp8) against ``R.a8_quant`` bit
for bit, the block-scaled-MFMA GEMM (mls_gemm_w8a8) against ``ops.w8a8_reference`` -- the fp32 product of the
same codes, so no quantisation error enters -- in every launch variant, and the Llama model with
``weight_dtype="w8a8"`` on the fused backend against the reference backend."""
import pytest
import torch

from mlmicroservicetemplate_amd.ops import reference as R
from test_kv_fp8_cpu import CFG128, decode_top5_deviation
from test_w8a8_cpu import D_W8

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FUSED_VS_REF = 5e-2  # tests/test_models_gpu.py test_llama_fused_matches_reference_tiny's bound
VARIANTS = range(6)  # 0: the launcher's pick; 1-3: the large tiles; 4, 5: decode-shaped (split-K)


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def _rows(M, K, seed):
    """bf16 rows with magnitudes over three decades, an all-zero row and a row with one large outlier."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.logspace(-2, 1, M).view(M, 1)
    x[1] = 0.0
    x[2, K - 60] = 1e4
    return x.to(torch.bfloat16).to(DEV)


# ------------------------------------------------------------------------------- 1. quantiser
@pytest.mark.parametrize("M,K", [(37, 512), (3, 2176), (3, 14336), (3, 28672)])
def test_quant_rows_matches_the_rule_bit_for_bit(M, K):
    from mlmicroservicetemplate_amd import ops

    x = _rows(M, K, seed=M + K)
    want_q, want_s = R.a8_quant(x)
    q, s = ops.quant_rows_fp8(x)
    assert q.dtype == torch.uint8 and q.shape == (M, K) and s.dtype == torch.float32 and s.shape == (M,)
    assert torch.equal(q, want_q) and torch.equal(s, want_s)
    assert not q[1].any() and s[1].item() == want_s[1].item() > 0
    # h = bf16(x + delta), written back; its codes and scales by the same rule
    d = _rows(M, K, seed=M + K + 1).flip(0).contiguous()
    h = (x.float() + d.float()).to(torch.bfloat16)
    r_out = torch.full_like(x, 7.0)
    q2, s2 = ops.quant_rows_fp8(x, d, r_out)
    want_q2, want_s2 = R.a8_quant(h)
    assert torch.equal(r_out, h) and torch.equal(q2, want_q2) and torch.equal(s2, want_s2)
    # norm: the same codes, scale = hs * rstd within 4 ulp
    eps = 1e-5
    for args, hh, wq_, ws_ in (((x,), x, want_q, want_s), ((x, d), h, want_q2, want_s2)):
        qn, sn = ops.quant_rows_fp8(*args, norm=True, eps=eps)
        rstd = torch.rsqrt(hh.float().pow(2).mean(-1) + eps)
        want = ws_ * rstd
        ulps = (sn.view(torch.int32) - want.view(torch.int32)).abs().max().item()
        print(f"norm scales, M {M} K {K}: {ulps} ulp")
        assert torch.equal(qn, wq_) and ulps <= 4


def test_quant_rows_rejects_bad_arguments():
    from mlmicroservicetemplate_amd import ops

    x = _rand(4, 256)
    with pytest.raises(ValueError):
        ops.quant_rows_fp8(x.float())
    with pytest.raises(ValueError):
        ops.quant_rows_fp8(x, resid_out=torch.empty_like(x))  # resid_out needs delta
    with pytest.raises(ValueError):
        ops.quant_rows_fp8(x, _rand(4, 128))
    with pytest.raises(ValueError):
        ops.quant_rows_fp8(_rand(4, 260))


# ------------------------------------------------------------------------------- 2. GEMM
@pytest.mark.parametrize("variant", VARIANTS)
def test_operand_map_exact(variant):
    """One-hot rows against weights whose every code, scale and product is exact (small integers times powers of
    two, asymmetric in n and k): catches a transposed operand, a wrong k order inside the 128-deep step and a
    wrong scale index."""
    from mlmicroservicetemplate_amd import ops

    assert ops.W8A8_VARIANTS == ops.lib().mls_gemm_w8a8_num_variants() == len(VARIANTS)
    N, K = 32, 384
    n = torch.arange(N, device=DEV).view(N, 1)
    k = torch.arange(K, device=DEV).view(1, K)
    w = (2.0 ** ((n + k // 128) % 5) * (((n * K + k) % 15) - 7)).to(torch.bfloat16)
    wq, ws = ops.pack_w8(w)
    codes = ops.unpack_w8_reference(wq, N, K)
    assert torch.equal(R.w8_dequant(codes, ws), w.float())  # the format holds w exactly
    ks = [0, 1, 31, 32, 127, 128, 200, 383]
    x = torch.zeros(len(ks), K, device=DEV, dtype=torch.bfloat16)
    for r, kk in enumerate(ks):
        x[r, kk] = 1.0
    want = w[:, ks].T.contiguous()
    # codes of 1.0 with unit row scales: nothing rounds anywhere
    xq = x.to(torch.float8_e4m3fn).view(torch.uint8)
    ones = torch.ones(len(ks), device=DEV)
    assert torch.equal(ops.gemm_w8a8(xq, ones, wq, ws, N, variant=variant), want)
    assert torch.equal(ops.w8a8_reference(xq, ones, codes, ws).to(torch.bfloat16), want)
    # through the quantiser: code 448, scale fl(1 / 448); the bf16 rounding of the output absorbs its last bit
    assert torch.equal(ops.gemm_w8a8(*ops.quant_rows_fp8(x), wq, ws, N, variant=variant), want)


RAN = set()


@pytest.mark.parametrize("N,K", [(n, k) for n in (16, 48, 272) for k in (128, 384, 2176)])
def test_random_shapes_cross_every_tile_edge(N, K):
    """M 1 .. 257 crosses the 16-row fragment, the 32 / 64 / 128 / 256-row tiles; N 16 .. 272 the 32-column pair,
    the 128- and 256-column tiles.  Every variant takes every shape (none is clamped)."""
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(N + K)
    w = _rand(N, K, scale=K**-0.5)
    wq, ws = ops.pack_w8(w)
    codes = ops.unpack_w8_reference(wq, N, K)
    for M in (1, 5, 17, 33, 130, 257):
        xq, xs = ops.quant_rows_fp8(_rand(M, K))
        ref = ops.w8a8_reference(xq, xs, codes, ws)
        for variant in VARIANTS:
            out = ops.gemm_w8a8(xq, xs, wq, ws, N, variant=variant)
            err = rel_err(out, ref)
            RAN.add(variant)
            assert out.shape == (M, N) and err < 1e-2, (M, N, K, variant, err)
    assert RAN == set(VARIANTS)


@pytest.mark.parametrize("variant,splitk", [(3, 2), (3, 4), (4, 2), (4, 8), (5, 4), (5, 8), (1, 2), (2, 2)])
def test_split_k_is_deterministic(variant, splitk):
    """K = 1024 = 8 k-steps in 2 / 4 / 8 splits; the reduce sums the slabs in split order, so launches repeat bit
    for bit."""
    from mlmicroservicetemplate_amd import ops

    M, N, K = 40, 272, 1024
    torch.manual_seed(variant * 10 + splitk)
    wq, ws = ops.pack_w8(_rand(N, K, scale=K**-0.5))
    xq, xs = ops.quant_rows_fp8(_rand(M, K))
    ref = ops.w8a8_reference(xq, xs, ops.unpack_w8_reference(wq, N, K), ws)
    work = torch.zeros(4 << 20, device=DEV, dtype=torch.float32)  # its own workspace, so its own counters
    first = ops.gemm_w8a8(xq, xs, wq, ws, N, variant=variant, splitk=splitk, workspace=work)
    assert rel_err(first, ref) < 1e-2
    for _ in range(3):
        assert torch.equal(ops.gemm_w8a8(xq, xs, wq, ws, N, variant=variant, splitk=splitk, workspace=work), first)
    torch.cuda.synchronize()
    assert int(ops.split_counters(work).abs().sum().item()) == 0  # every tile's reducer reset its counter


@pytest.mark.parametrize("variant,K,splitk", [(5, 256, 1), (4, 512, 2)])
def test_blocks_walk_more_than_one_unit(variant, K, splitk):
    """270 tiles of 32 x 128 / 150 tiles of 64 x 128 in 2 K splits (300 units of 2 k-steps) on a persistent grid
    of one block per CU: blocks walk two units, so the ring runs across a unit boundary and a unit's epilogue (or
    its split-K arrive) overlaps the next unit's DMA.  M = 257 leaves a one-row last tile."""
    from mlmicroservicetemplate_amd import ops

    M, N = 257, 3840
    bm, bn = ops.W8A8_CFGS[variant]
    units = -(-M // bm) * -(-N // bn) * splitk
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    if units <= cus:
        pytest.skip(f"{units} units on {cus} CUs: no block walks two units")
    torch.manual_seed(variant)
    wq, ws = ops.pack_w8(_rand(N, K, scale=K**-0.5))
    xq, xs = ops.quant_rows_fp8(_rand(M, K))
    ref = ops.w8a8_reference(xq, xs, ops.unpack_w8_reference(wq, N, K), ws)
    first = ops.gemm_w8a8(xq, xs, wq, ws, N, variant=variant, splitk=splitk)
    assert first.shape == (M, N) and rel_err(first, ref) < 1e-2
    assert torch.equal(ops.gemm_w8a8(xq, xs, wq, ws, N, variant=variant, splitk=splitk), first)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M", [4, 40, 257])
def test_epilogues(variant, M):
    """M = 257 (with K = 256): all eight 16-row blocks of the 256-row tiles hold valid rows under every epilogue,
    and a second, one-row tile follows."""
    from mlmicroservicetemplate_amd import ops

    K, N = (256 if M == 257 else 512), 272
    torch.manual_seed(10 * variant + M)
    wq, ws = ops.pack_w8(_rand(N, K, scale=K**-0.5))
    codes = ops.unpack_w8_reference(wq, N, K)
    xq, xs = ops.quant_rows_fp8(_rand(M, K))
    b, res = torch.randn(N, device=DEV) * 0.1, _rand(M, N)
    ref = ops.w8a8_reference(xq, xs, codes, ws)
    assert rel_err(ops.gemm_w8a8(xq, xs, wq, ws, N, bias=b, variant=variant), ref + b) < 1e-2
    assert rel_err(ops.gemm_w8a8(xq, xs, wq, ws, N, residual=res, variant=variant), ref + res.float()) < 1e-2
    out = torch.full((M, N), 9.0, device=DEV, dtype=torch.bfloat16)
    assert ops.gemm_w8a8(xq, xs, wq, ws, N, bias=b, residual=res, out=out, variant=variant) is out
    assert rel_err(out, ref + b + res.float()) < 1e-2
    # SiLU-mul on gate / up interleaved in groups of 8: the bound test_w4_gpu.py uses for this epilogue
    y = ref + b
    g, u = y.view(M, N // 16, 2, 8)[:, :, 0].reshape(M, -1), y.view(M, N // 16, 2, 8)[:, :, 1].reshape(M, -1)
    sm = ops.gemm_w8a8(xq, xs, wq, ws, N, bias=b, act="silu_mul", variant=variant)
    assert sm.shape == (M, N // 2) and rel_err(sm, torch.nn.functional.silu(g) * u) < 2e-2


def test_gemm_rejects_bad_arguments():
    from mlmicroservicetemplate_amd import ops

    N, K, M = 64, 256, 2
    wq, ws = ops.pack_w8(_rand(N, K))
    xq, xs = ops.quant_rows_fp8(_rand(M, K))
    ops.gemm_w8a8(xq, xs, wq, ws, N)
    bad = [
        dict(a=(xq[:, :192].contiguous(), xs, wq[: N * 192], ws, N)),  # K % 128
        dict(a=(xq, xs, wq[: 40 * K], ws[:40], 40)),  # N % 16
        dict(a=(xq, xs, wq, ws, 48)),  # wq size
        dict(a=(xq, xs, wq, ws[:-1], N)),  # ws size
        dict(a=(xq, xs[:1], wq, ws, N)),  # xs size
        dict(a=(xq.to(torch.int8), xs, wq, ws, N)),  # dtypes
        dict(a=(xq, xs.double(), wq, ws, N)),
        dict(a=(xq, xs, wq.to(torch.int8), ws, N)),
        dict(a=(xq, xs, wq, ws.to(torch.bfloat16), N)),
        dict(a=(xq, xs, wq, ws, N), variant=6),
        dict(a=(xq, xs, wq, ws, N), variant=-1),
        dict(a=(xq, xs, wq, ws, N), residual=_rand(M, 32)),
        dict(a=(xq, xs, wq, ws, N), residual=_rand(M, N).float()),
        dict(a=(xq, xs, wq, ws, N), bias=torch.zeros(N, device=DEV, dtype=torch.bfloat16)),
        dict(a=(xq, xs, wq, ws, N), act="silu_mul", residual=_rand(M, N)),
        dict(a=(xq, xs, wq, ws, N), act="gelu"),
        dict(a=(xq, xs, wq, ws, N), out=torch.empty(M, 32, device=DEV, dtype=torch.bfloat16)),
        dict(a=(xq, xs, wq, ws, N), variant=5, splitk=4),  # K / 128 = 2 k-steps
    ]
    for kw in bad:
        a = kw.pop("a")
        with pytest.raises(ValueError):
            ops.gemm_w8a8(*a, **kw)
    with pytest.raises(ValueError):
        ops.pack_w8(_rand(64, 200))


def test_graph_replay_matches_eager():
    """quant -> gate_up (SiLU-mul) -> quant -> down (+ residual), the layer's MLP chain, captured once.  4 rows of
    K = 1024: the launcher picks the 32-row tile and splits K four ways in both GEMMs, so an equal replay also shows
    the in-launch reduce is deterministic."""
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(0)
    M, H, I = 4, 1024, 1024
    gu = ops.pack_w8(ops.interleave_gate_up(_rand(I, H, scale=H**-0.5), _rand(I, H, scale=H**-0.5)))
    dn = ops.pack_w8(_rand(H, I, scale=I**-0.5))

    def chain(x, d):
        r = torch.empty_like(x)
        h = ops.gemm_w8a8(*ops.quant_rows_fp8(x, d, r, norm=True), *gu, 2 * I, act="silu_mul")
        return ops.gemm_w8a8(*ops.quant_rows_fp8(h), *dn, H, residual=r)

    xs, ds = _rand(M, H), _rand(M, H)
    chain(xs, ds)  # warm-up outside the capture (the split-K workspace and counters are allocated here)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s_out = chain(xs, ds)
    for seed in (1, 2):
        torch.manual_seed(seed)
        x, d = _rand(M, H), _rand(M, H)
        want = chain(x, d)
        xs.copy_(x)
        ds.copy_(d)
        g.replay()
        assert torch.equal(s_out, want)


# ------------------------------------------------------------------------------- 3. model
@pytest.fixture(scope="module")
def tiny():
    from mlmicroservicetemplate_amd.models.llama import init_llama_shard, tiny_config

    cfg = tiny_config(**CFG128)
    return cfg, init_llama_shard(cfg, 1, 0, seed=5, device=DEV)


def _llama(tiny, backend, **kw):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    kw = dict(dict(max_batch=2, max_seq=64, weight_dtype="w8a8"), **kw)
    return LlamaTP(p, cfg, backend=backend, device=DEV, **kw)


@pytest.fixture(scope="module")
def fused8(tiny):
    return _llama(tiny, "fused")


def _prompts():
    ids = torch.randint(3, 2000, (2, 20), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(DEV)
    return ids, torch.tensor([20, 20], dtype=torch.int32, device=DEV)


def test_model_fused_vs_reference(tiny, fused8):
    """A 40-row prefill and a 2-row decode step."""
    ids, lens = _prompts()
    ref = _llama(tiny, "reference")
    pos = torch.arange(20, device=DEV, dtype=torch.int32).unsqueeze(0).expand(2, 20).contiguous()
    rv, _ = ref.step(ids, pos, lens, decode=False, k=5)
    fv, _ = fused8.step(ids, pos, lens, decode=False, k=5)
    print("prefill, fused w8a8 vs reference w8a8:", rel_err(fv, rv))
    assert rel_err(fv, rv) < FUSED_VS_REF
    tok = torch.full((2, 1), 7, dtype=torch.int32, device=DEV)
    rv2, _ = ref.step(tok, lens.view(2, 1).clone(), lens + 1, decode=True, k=5)
    fv2, _ = fused8.step(tok, lens.view(2, 1).clone(), lens + 1, decode=True, k=5)
    print("decode, fused w8a8 vs reference w8a8:", rel_err(fv2, rv2))
    assert rel_err(fv2, rv2) < FUSED_VS_REF


def test_model_26_row_decode_step(tiny):
    B = 26
    ids = torch.randint(3, 2000, (B, 4), generator=torch.Generator().manual_seed(6)).to(torch.int32).to(DEV)
    lens = torch.full((B,), 4, dtype=torch.int32, device=DEV)
    ref = _llama(tiny, "reference", max_batch=B, max_seq=16)
    fus = _llama(tiny, "fused", max_batch=B, max_seq=16)
    dev = decode_top5_deviation(fus, ref, ids, lens)
    print("26-row decode, fused w8a8 vs reference w8a8:", dev)
    assert dev < FUSED_VS_REF


def test_model_fused_w8a8_vs_fused_bf16(tiny, fused8):
    ids, lens = _prompts()
    b16 = _llama(tiny, "fused", weight_dtype="bf16")
    assert not b16.w8 and b16.weight_dtype == "bf16"
    dev = decode_top5_deviation(fused8, b16, ids, lens)
    print("fused w8a8 vs fused bf16:", dev)
    assert dev <= 2 * D_W8 + FUSED_VS_REF


def test_model_holds_codes_only_and_runs_no_bf16_layer_kernel(tiny, fused8, monkeypatch):
    from mlmicroservicetemplate_amd import ops

    cfg, p = tiny
    m = fused8
    names = {f"l{i}.{n}" for i in range(cfg.layers) for n in ("qkv", "o", "gate_up", "down")}
    assert set(m.w8) == names and not m.w4 and not m.fp8
    assert not [n for n in m.p if n.split(".")[-1] in ("qkv", "o", "gate", "up", "gate_up", "down")]
    assert set(m.packed) <= {"lm_head"}
    shapes = {"qkv": (m.qkv_width, cfg.hidden), "o": (cfg.hidden, cfg.heads * cfg.head_dim),
              "gate_up": (2 * cfg.intermediate, cfg.hidden), "down": (cfg.hidden, cfg.intermediate)}
    assert m.layer_weight_bytes() == cfg.layers * sum(N * K + 4 * N for N, K in shapes.values())
    for name, (wq, ws, N) in m.w8.items():
        assert (N, wq.numel() // N) == shapes[name.split(".")[-1]] and wq.dtype == torch.uint8 and ws.shape == (N,)

    graphs, m.use_graphs = m.use_graphs, False  # eager decode so the counters see the calls
    calls = {"w8": 0, "bf16_layer": 0, "bf16_head": 0}
    real = {n: getattr(ops, n) for n in ("linear", "gemm_rmsnorm", "skinny_packed", "gemm_w8a8")}

    def spy16(name):
        def run(x, w, *a, **k):
            head = w is m.p["lm_head"] or w is m.packed.get("lm_head")
            calls["bf16_head" if head else "bf16_layer"] += 1
            return real[name](x, w, *a, **k)
        return run

    def spy8(*a, **k):
        calls["w8"] += 1
        return real["gemm_w8a8"](*a, **k)

    for n in ("linear", "gemm_rmsnorm", "skinny_packed"):
        monkeypatch.setattr(ops, n, spy16(n))
    monkeypatch.setattr(ops, "gemm_w8a8", spy8)
    try:
        ids, lens = _prompts()
        pos = torch.arange(20, device=DEV, dtype=torch.int32).unsqueeze(0).expand(2, 20).contiguous()
        m.step(ids, pos, lens, decode=False, k=5)  # 40 rows
        assert calls == {"w8": 4 * cfg.layers, "bf16_layer": 0, "bf16_head": 1}
        tok = torch.tensor([[7], [9]], device=DEV, dtype=torch.int32)
        m.decode_step(tok, lens.view(2, 1).clone(), 5, max_ctx=21)
        assert calls == {"w8": 8 * cfg.layers, "bf16_layer": 0, "bf16_head": 2}
    finally:
        m.use_graphs = graphs


@pytest.mark.parametrize("device_pick", ["1", "0"])
def test_model_generate_graphs_match_eager(tiny, monkeypatch, device_pick):
    from mlmicroservicetemplate_amd.models.llama import GenParams

    monkeypatch.setenv("MLS_DEVICE_PICK", device_pick)
    ids, lens = _prompts()
    gp = GenParams(max_new_tokens=8)
    eager = _llama(tiny, "fused")
    eager.use_graphs = False
    want = eager.generate(ids, lens, gp)
    graphed = _llama(tiny, "fused")
    assert graphed.use_graphs
    got = graphed.generate(ids, lens, gp)
    assert torch.equal(got, want)
    assert graphed._graphs or graphed._dev_graphs  # the decode steps were captured


def test_model_chunked_generate_against_the_reference(tiny):
    """generate(prefill_chunk=8): every emitted token, teacher-forced through the reference backend with w8a8, is
    among its top-8 within tests/test_kv_prefill_cache_gpu.py's bound."""
    from mlmicroservicetemplate_amd.models.llama import GenParams
    from test_kv_prefill_cache_gpu import _check_tokens

    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 2000, (3, 30), generator=g).to(torch.int32).to(DEV)
    lens = torch.tensor([30, 17, 5], dtype=torch.int32, device=DEV)
    ref = _llama(tiny, "reference", max_batch=4, max_seq=64)
    m = _llama(tiny, "fused", max_batch=4, max_seq=64)
    out = m.generate(ids, lens, GenParams(max_new_tokens=6), prefill_chunk=8).cpu()
    assert out.shape == (3, 6)
    for b in range(3):
        _check_tokens(ref, ids[b, : int(lens[b])].tolist(), out[b].tolist())


def test_model_refuses_bad_geometry(tiny):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP, init_llama_shard, tiny_config

    cfg192 = tiny_config(layers=1, hidden=192, heads=2, kv_heads=1, head_dim=128, intermediate=512)
    with pytest.raises(ValueError, match="128"):
        LlamaTP(init_llama_shard(cfg192, 1, 0, seed=1, device=DEV), cfg192, backend="fused", device=DEV, max_batch=2,
                max_seq=64, weight_dtype="w8a8")
