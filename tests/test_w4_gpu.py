"""csrc/skinny_w4.hip, the W4A16 decode GEMM (mls_skinny_w4), vs ``ops.w4_reference`` -- the fp32 product
with the same dequantised weights, so no quantisation error enters -- every launch variant, and the
Llama model with ``weight_dtype="int4"`` on the fused backend vs the reference backend."""
import pytest
import torch

from test_kv_fp8_cpu import CFG128, decode_top5_deviation
from test_w4_cpu import D_W4

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FUSED_VS_REF = 5e-2  # tests/test_models_gpu.py test_llama_fused_matches_reference_tiny's bound


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


# ------------------------------------------------------------------------------- 1. kernel
@pytest.mark.parametrize("M,N,K", [(1, 16, 128), (3, 48, 384), (4, 64, 2176), (5, 32, 1024), (16, 64, 512),
                                   (17, 32, 256), (24, 96, 2048), (2, 64, 14336), (1, 256, 4096)])
def test_w4_plain(M, N, K):
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(M + N + K)
    x, w = _rand(M, K), _rand(N, K, scale=K**-0.5)
    b, res = torch.randn(N, device=DEV) * 0.1, _rand(M, N)
    wq, sc = ops.pack_skinny_w4(w)
    ref = ops.w4_reference(x, w)
    assert rel_err(ops.skinny_w4(x, wq, sc, N), ref) < 1e-2
    out = ops.skinny_w4(x, wq, sc, N, bias=b, residual=res)
    assert rel_err(out, ref + b + res.float()) < 1e-2


@pytest.mark.parametrize("variant", range(13))
@pytest.mark.parametrize("M", [1, 8, 24])
def test_w4_variants(variant, M):
    """Every launch shape the launcher accepts (a shape the call cannot take falls to the nearest
    one it can); N = 192 tiles by 1, 2 and 4, 17 granules over 8 / 16 waves."""
    from mlmicroservicetemplate_amd import ops

    assert ops.W4_VARIANTS == ops.lib().mls_skinny_w4_num_variants() == 13
    N, K = 192, 2176
    torch.manual_seed(variant + M)
    x, w = _rand(M, K), _rand(N, K, scale=K**-0.5)
    b, res = torch.randn(N, device=DEV) * 0.1, _rand(M, N)
    wq, sc = ops.pack_skinny_w4(w)
    out = ops.skinny_w4(x, wq, sc, N, bias=b, residual=res, variant=variant)
    assert rel_err(out, ops.w4_reference(x, w) + b + res.float()) < 1e-2


@pytest.mark.parametrize("variant", [0, 4, 11, 12])
def test_w4_exact_one_hot(variant):
    """One-hot rows against weights whose every value, scale and product is exact in bf16: catches the
    nibble order, a transposed operand map and a wrong scale index."""
    from mlmicroservicetemplate_amd import ops

    N, K = 32, 512
    n = torch.arange(N, device=DEV).view(N, 1)
    k = torch.arange(K, device=DEV).view(1, K)
    w = (2.0 ** ((n + k // 128) % 5) * (((n * K + k) % 15) - 7)).to(torch.bfloat16)
    wq, sc = ops.pack_skinny_w4(w)
    q, s = ops.unpack_skinny_w4_reference(wq, sc, N, K)
    assert torch.equal(q.float() * s.float().repeat_interleave(128, dim=1), w.float())  # the format holds w exactly
    for ks in ([0, 1, 9, 127], [128, 200, 301, 383], [384, 450, 510, 511]):  # first, a middle, the last group
        x = torch.zeros(len(ks), K, device=DEV, dtype=torch.bfloat16)
        for r, kk in enumerate(ks):
            x[r, kk] = 1.0
        out = ops.skinny_w4(x, wq, sc, N, variant=variant)
        assert torch.equal(out, w[:, ks].T.contiguous()), ks


@pytest.mark.parametrize("variant", [0, 3, 6, 10, 11, 12])
@pytest.mark.parametrize("M", [1, 4, 8, 17])
def test_w4_add_norm_silu_mul(variant, M):
    """The decode gate_up form: RMSNorm(x + delta) with the gain folded into W, SiLU-mul epilogue,
    x + delta written back to the residual stream."""
    from mlmicroservicetemplate_amd import ops

    K, N = 512, 256
    torch.manual_seed(10 * variant + M)
    x, d = _rand(M, K), _rand(M, K)
    gain = torch.rand(K, device=DEV) + 0.5
    w = ops.interleave_gate_up(_rand(N // 2, K, scale=K**-0.5), _rand(N // 2, K, scale=K**-0.5))
    wf = ops.fold_norm(w, gain)
    wq, sc = ops.pack_skinny_w4(wf)
    r_out = torch.empty_like(x)
    out = ops.skinny_w4(x, wq, sc, N, delta=d, resid_out=r_out, norm=True, act="silu_mul", variant=variant)
    h = (x.float() + d.float()).to(torch.bfloat16)
    assert torch.equal(r_out, h)
    rstd = torch.rsqrt(h.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    y = ops.w4_reference(h, wf) * rstd
    g, u = y.view(M, N // 16, 2, 8)[:, :, 0].reshape(M, -1), y.view(M, N // 16, 2, 8)[:, :, 1].reshape(M, -1)
    assert rel_err(out, torch.nn.functional.silu(g) * u) < 2e-2
    # norm without delta: the same rows, nothing written back
    out2 = ops.skinny_w4(h, wq, sc, N, norm=True, act="silu_mul", variant=variant)
    assert rel_err(out2, torch.nn.functional.silu(g) * u) < 2e-2


def test_w4_rejects_bad_arguments():
    from mlmicroservicetemplate_amd import ops

    wq, sc = ops.pack_skinny_w4(_rand(64, 256))
    x = _rand(2, 256)
    with pytest.raises(ValueError):
        ops.skinny_w4(_rand(33, 256), wq, sc, 64)  # M > 32
    with pytest.raises(ValueError):
        ops.skinny_w4(x, wq, sc, 48)  # wq size mismatch
    with pytest.raises(ValueError):
        ops.skinny_w4(x, wq, sc[:-16], 64)  # scales size mismatch
    with pytest.raises(ValueError):
        ops.skinny_w4(_rand(2, 192), wq[: 64 * 96], sc[:96], 64)  # K % 128
    with pytest.raises(ValueError):
        ops.skinny_w4(x, wq, sc, 64, delta=_rand(2, 256))  # delta only with norm
    with pytest.raises(ValueError):
        ops.skinny_w4(x, wq, sc, 64, norm=True, resid_out=torch.empty_like(x))  # resid_out needs delta
    with pytest.raises(ValueError):
        ops.skinny_w4(x, wq, sc, 64, residual=_rand(2, 32))
    with pytest.raises(ValueError):
        ops.skinny_w4(x, wq, sc, 64, variant=13)
    with pytest.raises(ValueError):
        ops.skinny_w4(x, wq, sc, 64, out=torch.empty(2, 32, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.pack_skinny_w4(_rand(64, 200))


def test_w4_graph_replay_matches_eager():
    """Three consecutive calls (norm + add-norm + plain with residual, the decode layer's chain) captured once."""
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(0)
    M, K, N = 4, 512, 256
    w1, w2 = _rand(N, K, scale=K**-0.5), _rand(K, N // 2, scale=N**-0.5)
    p1, p2 = ops.pack_skinny_w4(w1), ops.pack_skinny_w4(_rand(K, K, scale=K**-0.5))
    p3 = ops.pack_skinny_w4(w2)

    def chain(x, d):
        h = ops.skinny_w4(x, *p2, K, norm=True)
        r = torch.empty_like(x)
        gu = ops.skinny_w4(h, *p1, N, delta=d, resid_out=r, norm=True, act="silu_mul")
        return ops.skinny_w4(gu, *p3, K, residual=r)

    xs, ds = _rand(M, K), _rand(M, K)
    chain(xs, ds)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s_out = chain(xs, ds)
    for seed in (1, 2):
        torch.manual_seed(seed)
        x, d = _rand(M, K), _rand(M, K)
        want = chain(x, d)
        xs.copy_(x)
        ds.copy_(d)
        g.replay()
        assert torch.equal(s_out, want)


# ------------------------------------------------------------------------------- 2. model
@pytest.fixture(scope="module")
def tiny():
    from mlmicroservicetemplate_amd.models.llama import init_llama_shard, tiny_config

    cfg = tiny_config(**CFG128)
    return cfg, init_llama_shard(cfg, 1, 0, seed=5, device=DEV)


@pytest.fixture(scope="module")
def fused4(tiny):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    return LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, weight_dtype="int4")


def _prompts():
    ids = torch.randint(3, 2000, (2, 20), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(DEV)
    return ids, torch.tensor([20, 20], dtype=torch.int32, device=DEV)


def test_model_fused_int4_vs_reference_int4(tiny, fused4):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    ids, lens = _prompts()
    ref = LlamaTP(p, cfg, backend="reference", device=DEV, max_batch=2, max_seq=64, weight_dtype="int4")
    pos = torch.arange(20, device=DEV, dtype=torch.int32).unsqueeze(0).expand(2, 20).contiguous()
    rv, _ = ref.step(ids, pos, lens, decode=False, k=5)
    fv, _ = fused4.step(ids, pos, lens, decode=False, k=5)
    print("prefill, fused int4 vs reference int4:", rel_err(fv, rv))
    assert rel_err(fv, rv) < FUSED_VS_REF
    tok = torch.full((2, 1), 7, dtype=torch.int32, device=DEV)
    rv2, _ = ref.step(tok, lens.view(2, 1).clone(), lens + 1, decode=True, k=5)
    fv2, _ = fused4.step(tok, lens.view(2, 1).clone(), lens + 1, decode=True, k=5)
    print("decode, fused int4 vs reference int4:", rel_err(fv2, rv2))
    assert rel_err(fv2, rv2) < FUSED_VS_REF


def test_model_26_row_decode_step(tiny):
    """Above 24 rows: two 16-row A fragments per granule, and the lm_head route without a packed copy."""
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    B = 26
    ids = torch.randint(3, 2000, (B, 4), generator=torch.Generator().manual_seed(6)).to(torch.int32).to(DEV)
    lens = torch.full((B,), 4, dtype=torch.int32, device=DEV)
    ref = LlamaTP(p, cfg, backend="reference", device=DEV, max_batch=B, max_seq=16, weight_dtype="int4")
    fus = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=B, max_seq=16, weight_dtype="int4")
    dev = decode_top5_deviation(fus, ref, ids, lens)
    print("26-row decode, fused int4 vs reference int4:", dev)
    assert dev < FUSED_VS_REF


def test_model_fused_int4_vs_fused_bf16(tiny, fused4):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    ids, lens = _prompts()
    b16 = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64)
    assert not b16.w4 and b16.weight_dtype == "bf16"
    dev = decode_top5_deviation(fused4, b16, ids, lens)
    print("fused int4 vs fused bf16:", dev)
    assert dev <= 2 * D_W4 + FUSED_VS_REF


def test_model_decode_runs_the_w4_kernel(tiny, fused4, monkeypatch):
    from mlmicroservicetemplate_amd import ops

    cfg, p = tiny
    m = fused4
    assert m.w4_max_rows == 32
    graphs, m.use_graphs = m.use_graphs, False  # eager decode so the counters see the calls
    layer_packed = {id(w) for n, w in m.packed.items() if n != "lm_head"}
    assert not layer_packed and set(m.w4) == {f"l{i}.{n}" for i in range(cfg.layers)
                                              for n in ("qkv", "o", "gate_up", "down")}
    calls = {"w4": 0, "packed_layer": 0, "packed_head": 0}
    real4, real16 = ops.skinny_w4, ops.skinny_packed

    def spy4(*a, **k):
        calls["w4"] += 1
        return real4(*a, **k)

    def spy16(x, wp, *a, **k):
        calls["packed_head" if wp is m.packed["lm_head"] else "packed_layer"] += 1
        return real16(x, wp, *a, **k)

    monkeypatch.setattr(ops, "skinny_w4", spy4)
    monkeypatch.setattr(ops, "skinny_packed", spy16)
    try:
        ids, lens = _prompts()
        pos = torch.arange(20, device=DEV, dtype=torch.int32).unsqueeze(0).expand(2, 20).contiguous()
        m.step(ids, pos, lens, decode=False, k=5)  # 40 rows: the bf16 rounding of the same weights
        assert calls["w4"] == 0 and calls["packed_layer"] == 0
        tok = torch.tensor([[7], [9]], device=DEV, dtype=torch.int32)
        m.decode_step(tok, lens.view(2, 1).clone(), 5, max_ctx=21)
        # lm_head (2 rows in both steps) stays on the packed bf16 kernel
        assert calls == {"w4": 4 * cfg.layers, "packed_layer": 0, "packed_head": 2}
    finally:
        m.use_graphs = graphs


@pytest.mark.parametrize("device_pick", ["1", "0"])
def test_model_generate_graphs_match_eager(tiny, monkeypatch, device_pick):
    """The captured decode step (device-resident loop, and the host loop over a step graph) needs no
    change for int4: same tokens as the eager loop."""
    from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP

    monkeypatch.setenv("MLS_DEVICE_PICK", device_pick)
    cfg, p = tiny
    ids, lens = _prompts()
    gp = GenParams(max_new_tokens=8)
    eager = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, weight_dtype="int4")
    eager.use_graphs = False
    want = eager.generate(ids, lens, gp)
    graphed = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, weight_dtype="int4")
    assert graphed.use_graphs
    got = graphed.generate(ids, lens, gp)
    assert torch.equal(got, want)
    assert graphed._graphs or graphed._dev_graphs  # the decode steps were captured


def test_model_int4_bytes(tiny, fused4):
    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    nbytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)  # noqa: E731
    for i in range(cfg.layers):
        names = [f"l{i}.{n}" for n in ("qkv", "o", "gate_up", "down")]
        bf16 = nbytes(fused4.p[n] for n in names)
        int4 = nbytes(t for n in names for t in fused4.w4[n])
        assert int4 * 16 * 128 == bf16 * (4 * 128 + 16)  # (4 + 16/128) / 16
    b16 = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64)
    assert fused4.layer_weight_bytes() * 16 * 128 == b16.layer_weight_bytes() * (4 * 128 + 16)
    # the bf16 copy prefill and the > 32-row steps read is the RNE rounding of the dequantised codes
    q, s = ops.unpack_skinny_w4_reference(*fused4.w4["l0.o"], *fused4.p["l0.o"].shape)
    assert torch.equal(fused4.p["l0.o"], (q.float() * s.float().repeat_interleave(128, dim=1)).to(torch.bfloat16))


def test_model_refuses_bad_geometry(tiny):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP, init_llama_shard, tiny_config

    cfg, p = tiny
    with pytest.raises(ValueError):
        LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=2, max_seq=64, weight_dtype="int8")
    cfg64 = tiny_config(layers=1, hidden=192, heads=2, kv_heads=1, head_dim=128, intermediate=512)
    with pytest.raises(ValueError):
        LlamaTP(init_llama_shard(cfg64, 1, 0, seed=1, device=DEV), cfg64, backend="fused", device=DEV, max_batch=2,
                max_seq=64, weight_dtype="int4")
