"""End-to-end model numerics on MI355X: fused (HIP kernels) vs fp32 PyTorch reference."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def test_gemm_silu_mul():
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(0)
    M, I, K = 37, 256, 512
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    g = (torch.randn(I, K, device=DEV) / K**0.5).to(torch.bfloat16)
    u = (torch.randn(I, K, device=DEV) / K**0.5).to(torch.bfloat16)
    w = ops.interleave_gate_up(g, u)
    ref = torch.nn.functional.silu(x.float() @ g.float().T) * (x.float() @ u.float().T)
    ws = torch.empty(8 << 20, device=DEV, dtype=torch.float32)
    for cfg, sk in ((0, 0), (1, 1), (4, 1), (4, 4), (2, 2), (13, 1), (15, 2)):
        out = ops.gemm(x, w, act="silu_mul", workspace=ws, cfg=cfg, splitk=sk)
        assert out.shape == (M, I)
        assert rel(out, ref) < 2e-2, (cfg, sk)


@pytest.mark.parametrize("M", [1, 3, 4, 5, 16, 17, 32])
@pytest.mark.parametrize("nsplit", [0, 1, 3])
def test_skinny_gemm(M, nsplit):
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(M)
    N, K = 1024, 1000
    a = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K**0.5).to(torch.bfloat16)
    b = torch.randn(N, device=DEV)
    r = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    ws = torch.empty(4 << 20, device=DEV, dtype=torch.float32)
    y = a.float() @ w.float().T + b
    for act, ref in ((0, y + r.float()), (2, torch.nn.functional.gelu(y + r.float()))):
        out = ops.gemm(a, w, b, residual=r, act=act, workspace=ws, splitk=nsplit)
        assert rel(out, ref) < 2e-2
    g = w[:512].contiguous()
    u = w[512:].contiguous()
    wi = ops.interleave_gate_up(g, u)
    out = ops.gemm(a, wi, act="silu_mul", workspace=ws, splitk=nsplit)
    ref = torch.nn.functional.silu(a.float() @ g.float().T) * (a.float() @ u.float().T)
    assert out.shape == (M, 512) and rel(out, ref) < 2e-2


@pytest.mark.parametrize("M", [1, 2, 4, 7, 16, 32])
@pytest.mark.parametrize("nsplit", [0, 1, 4])
def test_gemm_rmsnorm_fused(M, nsplit):
    """Skinny GEMM with the residual add + RMSNorm prologue vs fp32 (gain folded into W)."""
    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.ops import reference as R

    torch.manual_seed(10 + M)
    N, K = 768, 1024
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    d = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    gain = (torch.rand(K, device=DEV) + 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K**0.5).to(torch.bfloat16)
    ws = torch.empty(4 << 20, device=DEV, dtype=torch.float32)
    wf = ops.fold_norm(w, gain)
    xn, hs = R.layernorm(x, gain, None, residual=d, eps=1e-5, rms=True)
    r_out = torch.empty_like(x)
    y = ops.gemm_rmsnorm(x, wf, d, r_out, eps=1e-5, workspace=ws, splitk=nsplit)
    assert rel(y, xn.float() @ w.float().T) < 2e-2
    assert rel(r_out, hs) < 1e-2
    y0 = ops.gemm_rmsnorm(x, wf, eps=1e-5, workspace=ws, splitk=nsplit)  # no residual update
    xn0 = R.layernorm(x, gain, None, eps=1e-5, rms=True)[0]
    assert rel(y0, xn0.float() @ w.float().T) < 2e-2
    g, u = w[:384].contiguous(), w[384:].contiguous()
    wi = ops.fold_norm(ops.interleave_gate_up(g, u), gain)
    out = ops.gemm_rmsnorm(x, wi, d, None, act="silu_mul", eps=1e-5, workspace=ws, splitk=nsplit)
    ref = torch.nn.functional.silu(xn.float() @ g.float().T) * (xn.float() @ u.float().T)
    assert out.shape == (M, 384) and rel(out, ref) < 2e-2


@pytest.mark.parametrize("M", [3, 16])
def test_skinny_gemm_ragged_k(M):
    """K % 32 == 8: the row-major kernel's k tail (the last k-step holds one 8-wide slice), which K % 32
    also keeps off the LDS kernel at M <= 4."""
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(30 + M)
    N, K = 48, 104
    a = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K**0.5).to(torch.bfloat16)
    b = torch.randn(N, device=DEV)
    r = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    out = ops.gemm(a, w, b, residual=r, splitk=1)
    assert rel(out, a.float() @ w.float().T + b + r.float()) < 2e-2


@pytest.mark.parametrize("nsplit", [1, 2])
def test_gemm_rmsnorm_two_row_tiles_ragged_k(nsplit):
    """M = 17: two 16-row A fragments per k-step, with the ragged K and, at nsplit = 2, the partial
    square sums that ride behind the slabs to the finishing kernel."""
    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.ops import reference as R

    torch.manual_seed(40 + nsplit)
    M, N, K = 17, 48, 104
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    d = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    gain = (torch.rand(K, device=DEV) + 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K**0.5).to(torch.bfloat16)
    ws = torch.empty(nsplit * M * (N + 1), device=DEV, dtype=torch.float32)
    r_out = torch.empty_like(x)
    y = ops.gemm_rmsnorm(x, ops.fold_norm(w, gain), d, r_out, eps=1e-5, workspace=ws, splitk=nsplit)
    assert torch.equal(r_out, (x.float() + d.float()).to(torch.bfloat16))
    xn = R.layernorm(x, gain, None, residual=d, eps=1e-5, rms=True)[0]
    assert rel(y, xn.float() @ w.float().T) < 2e-2


@pytest.mark.parametrize("M", [1, 3, 4])
@pytest.mark.parametrize("fused", [False, True])
def test_skinny_lds_wide_n(M, fused):
    """The few-row LDS-staged skinny kernel with NT = 2 / 4 column tiles per block (N >= 24576)."""
    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.ops import reference as R

    torch.manual_seed(20 + M)
    N, K = 24576 + 1024, 512
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    d = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K**0.5).to(torch.bfloat16)
    ws = torch.empty(8 << 20, device=DEV, dtype=torch.float32)
    if fused:
        gain = (torch.rand(K, device=DEV) + 0.5).to(torch.bfloat16)
        r_out = torch.empty_like(x)
        y = ops.gemm_rmsnorm(x, ops.fold_norm(w, gain), d, r_out, eps=1e-5, workspace=ws, splitk=1)
        xn, hs = R.layernorm(x, gain, None, residual=d, eps=1e-5, rms=True)
        assert rel(y, xn.float() @ w.float().T) < 2e-2 and rel(r_out, hs) < 1e-2
    else:
        y = ops.gemm(x, w, workspace=ws, splitk=1)
        assert rel(y, x.float() @ w.float().T) < 2e-2
    g, u = w[: N // 2].contiguous(), w[N // 2:].contiguous()
    out = ops.gemm(x, ops.interleave_gate_up(g, u), act="silu_mul", workspace=ws, splitk=1)
    ref = torch.nn.functional.silu(x.float() @ g.float().T) * (x.float() @ u.float().T)
    assert rel(out, ref) < 2e-2


@pytest.mark.parametrize("impl", ["blas", "native", "tile", "auto"])
def test_linear_dispatch(impl):
    """ops.linear: the native paths (conv_gemm tiles, the LDS-DMA tile kernel, the default routing)
    and the hipBLASLt A/B reference agree with fp32."""
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(7)
    M, N, K = 640, 512, 384
    a = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / K**0.5).to(torch.bfloat16)
    b = torch.randn(N, device=DEV)
    r = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    ws = torch.empty(4 << 20, device=DEV, dtype=torch.float32)
    y = a.float() @ w.float().T + b
    assert rel(ops.linear(a, w, b, impl=impl, workspace=ws), y) < 2e-2
    assert rel(ops.linear(a, w, b, residual=r, impl=impl, workspace=ws), y + r.float()) < 2e-2
    assert rel(ops.linear(a, w, None, residual=r, impl=impl, workspace=ws), y - b + r.float()) < 2e-2
    assert rel(ops.linear(a, w, b, act="gelu", impl=impl, workspace=ws), torch.nn.functional.gelu(y)) < 2e-2
    g, u = w[:256].contiguous(), w[256:].contiguous()
    out = ops.linear(a, ops.interleave_gate_up(g, u), act="silu_mul", impl=impl, workspace=ws)
    ref = torch.nn.functional.silu(a.float() @ g.float().T) * (a.float() @ u.float().T)
    assert out.shape == (M, 256) and rel(out, ref) < 2e-2


def test_topk_large():
    from mlmicroservicetemplate_amd import ops

    x = torch.randn(3, 128256, device=DEV).to(torch.bfloat16)
    v, i = ops.topk_large(x, 8)
    rv, ri = torch.topk(x.float(), 8, dim=-1)
    assert torch.allclose(v, rv) and torch.allclose(x.float().gather(1, i.long()), rv)


@pytest.mark.parametrize("N,k,lo,valid", [(128256, 1, 0, 128256), (128256, 50, 0, 128256), (16032, 5, 112224, 16032),
                                          (16032, 4, 120240, 8016), (16032, 3, 128256, 0), (30000, 2, 7, 29990)])
def test_topk_large_shard_offset_and_tail(N, k, lo, valid):
    """Native two-launch path: shard offset added and the padded tail never wins (vs torch.topk
    over the valid columns)."""
    from mlmicroservicetemplate_amd import ops

    torch.manual_seed(k)
    x = torch.randn(2, N, device=DEV).to(torch.bfloat16)
    x[:, valid:] = 100.0  # the padded tail would win if it were not masked
    v, i = ops.topk_large(x, k, lo=lo, valid=valid)
    if valid == 0:
        assert torch.isinf(v).all() and (v < 0).all()
        return
    rv, _ = torch.topk(x[:, :valid].float(), k, dim=-1)
    assert torch.allclose(v, rv)
    local = i.long() - lo
    assert (local >= 0).all() and (local < valid).all()
    assert torch.allclose(x.float().gather(1, local), rv)


# 256 tokens: conv_gemm tiles; 1024 / 4096 (the benchmark shape): the LDS-DMA tile GEMM
@pytest.mark.parametrize("B,S", [(4, 64), (16, 64), (32, 128)])
def test_bert_fused_matches_reference(B, S):
    from mlmicroservicetemplate_amd.models import bert

    cfg = bert.BertConfig(num_labels=3)
    p = bert.init_bert(cfg, 0)
    torch.manual_seed(1)
    ids = torch.randint(1000, cfg.vocab, (B, S), device=DEV, dtype=torch.int32)
    tt = torch.zeros_like(ids)
    lens = torch.tensor(([64, 33, 10, 1] * (B // 4)), device=DEV, dtype=torch.int32)
    ref = bert.bert_reference({k: v.to(DEV) for k, v in p.items()}, ids, tt, lens, cfg)
    fused = bert.BertFused(p, DEV, cfg)
    out = fused(ids, tt, lens)[:, :3].float()
    assert rel(out, ref) < 3e-2  # bf16 activations through 12 layers: 2.1-2.2 % measured
    vals, idx = fused.classify(ids, tt, lens, k=3)
    top2 = ref.topk(2, dim=-1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * (out - ref).abs().max()
    assert torch.equal(idx[:, 0].long()[sure], ref.argmax(-1)[sure])
    eager = bert.BertEager(p, DEV, cfg)
    assert rel(eager(ids, tt, lens).float(), ref) < 5e-2


def test_llama_fused_matches_reference_tiny():
    from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config

    cfg = tiny_config(layers=3, hidden=512, heads=8, kv_heads=2, head_dim=64, intermediate=1024)
    cfg.head_dim = 128  # the fused kernels' Llama head size
    cfg.heads, cfg.kv_heads = 4, 1
    p = init_llama_shard(cfg, 1, 0, seed=3, device=DEV)
    ref = LlamaTP(p, cfg, backend="reference", device=DEV, max_batch=4, max_seq=512)
    fus = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=4, max_seq=512)
    torch.manual_seed(2)
    ids = torch.randint(3, cfg.vocab - 1, (3, 70), device=DEV, dtype=torch.int32)
    lens = torch.tensor([70, 41, 5], device=DEV, dtype=torch.int32)
    pos = torch.arange(70, device=DEV, dtype=torch.int32).unsqueeze(0).expand(3, 70).contiguous()
    rv, ri = ref.step(ids, pos, lens, decode=False, k=8)
    fv, fi = fus.step(ids, pos, lens, decode=False, k=8)
    assert rel(fv, rv) < 5e-2
    assert (fi[:, 0] == ri[:, 0]).float().mean() >= 2 / 3
    # decode step over the caches each backend filled
    tok = ri[:, 0].view(3, 1)
    rv2, ri2 = ref.step(tok, lens.view(3, 1), lens + 1, decode=True, k=8)
    fv2, fi2 = fus.step(tok, lens.view(3, 1), lens + 1, decode=True, k=8)
    assert rel(fv2, rv2) < 5e-2
    out = fus.generate(ids, lens, GenParams(max_new_tokens=8))
    assert out.shape == (3, 8)


@pytest.mark.slow
def test_llama3_8b_tp1_generate_smoke():
    """Full Llama-3-8B shapes on one MI355X (TP=1, 16 GB of bf16 weights)."""
    import time

    from mlmicroservicetemplate_amd.models.llama import LLAMA3_8B, GenParams, LlamaTP, init_llama_shard

    p = init_llama_shard(LLAMA3_8B, 1, 0, seed=0, device=DEV)
    m = LlamaTP(p, LLAMA3_8B, backend="fused", device=DEV, max_batch=4, max_seq=1024)
    ids = torch.randint(1000, 100000, (2, 128), device=DEV, dtype=torch.int32)
    lens = torch.tensor([128, 77], device=DEV, dtype=torch.int32)
    t0 = time.time()
    out = m.generate(ids, lens, GenParams(max_new_tokens=8))
    torch.cuda.synchronize()
    assert out.shape == (2, 8) and int(out.min()) >= 0 and int(out.max()) < LLAMA3_8B.vocab
    print(f"8B generate 8 tokens: {time.time() - t0:.2f}s")


def test_continuous_batching_fused():
    """Continuous batching over the fused decode graph (max_batch rows, idle slots included)."""
    import time

    from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    cfg = tiny_config(layers=2, hidden=512, heads=8, kv_heads=2, head_dim=128, intermediate=1024)
    p = init_llama_shard(cfg, 1, 0, seed=5, device=DEV)
    m = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=4, max_seq=256)
    eng = ContinuousLlama(m).start()
    g = torch.Generator().manual_seed(1)
    reqs = [(torch.randint(3, 2000, (int(n),), generator=g).tolist(), GenParams(max_new_tokens=int(t)))
            for n, t in zip(torch.randint(2, 40, (9,), generator=g), torch.randint(2, 12, (9,), generator=g))]
    futs = []
    for ids, gp in reqs:
        futs.append(eng.submit(ids, gp))
        time.sleep(0.005)
    outs = [f.result(timeout=120) for f in futs]
    eng.stop()
    single = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=1, max_seq=256)
    agree = total = 0
    for (ids, gp), got in zip(reqs, outs):
        want = single.generate(torch.tensor([ids]), torch.tensor([len(ids)]), gp)[0].tolist()[: len(got)]
        assert got[0] == want[0]  # the prefill token
        agree += sum(a == b for a, b in zip(got, want))
        total += len(got)
    assert agree / total >= 0.9, (agree, total)  # bf16: different row counts may flip late near-ties
