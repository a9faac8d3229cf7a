"""csrc/gemm_w4.hip (ops.gemm_w4a16) vs ``ops.w4_reference`` in every tile variant, and the fused Llama with
``weight_dtype="int4", w4_rows="all"`` vs the reference int4 backend.  Metric and bounds: tests/test_w4_gpu.py's."""
import pytest
import torch

from mlmicroservicetemplate_amd import ops
from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
from test_kv_fp8_cpu import CFG128, decode_top5_deviation
from test_w4_gpu import FUSED_VS_REF, _prompts, _rand, rel_err

pytestmark = pytest.mark.gpu
DEV, VARIANTS = "cuda:0", range(6)


@pytest.fixture(scope="module")
def weights():
    torch.manual_seed(0)
    ws = {(N, K): _rand(N, K, scale=K**-0.5) for N in (16, 48, 272) for K in (128, 384, 2176)}
    return {nk: (w, *ops.pack_skinny_w4(w)) for nk, w in ws.items()}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", [128, 384, 2176])
@pytest.mark.parametrize("M", [1, 16, 17, 33, 64, 65, 129, 257])
def test_gemm_w4_plain(weights, M, K, variant):
    torch.manual_seed(M + K)
    x = _rand(M, K)
    for N in (16, 48, 272):
        w, wq, sc = weights[N, K]
        b, res = torch.randn(N, device=DEV) * 0.1, _rand(M, N)
        ref = ops.w4_reference(x, w)
        assert rel_err(ops.gemm_w4a16(x, wq, sc, N, variant=variant), ref) < 1e-2, N
        out = ops.gemm_w4a16(x, wq, sc, N, bias=b, residual=res, variant=variant)
        assert rel_err(out, ref + b + res.float()) < 1e-2, N


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_w4_exact_one_hot(variant):
    N, K, M = 32, 512, 40
    n, k = torch.arange(N, device=DEV).view(N, 1), torch.arange(K, device=DEV).view(1, K)
    w = (2.0 ** ((n + k // 128) % 5) * (((n * K + k) % 15) - 7)).to(torch.bfloat16)
    x = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    want = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    for r, kk in {0: 1, 5: 127, 17: 200, 31: 301, 32: 384, 39: 511}.items():
        x[r, kk] = 1.0
        want[r] = w[:, kk]
    assert torch.equal(ops.gemm_w4a16(x, *ops.pack_skinny_w4(w), N, variant=variant), want)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M", [40, 257])
def test_gemm_w4_silu_mul_and_residual(variant, M):
    N, K = 272, 256
    torch.manual_seed(M + variant)
    x, res = _rand(M, K), _rand(M, N)
    w = ops.interleave_gate_up(_rand(N // 2, K, scale=K**-0.5), _rand(N // 2, K, scale=K**-0.5))
    wq, sc = ops.pack_skinny_w4(w)
    y = ops.w4_reference(x, w)
    v = y.view(M, N // 16, 2, 8)
    want = torch.nn.functional.silu(v[:, :, 0].reshape(M, -1)) * v[:, :, 1].reshape(M, -1)
    out = ops.gemm_w4a16(x, wq, sc, N, act="silu_mul", variant=variant)
    assert out.shape == (M, N // 2) and rel_err(out, want) < 1e-2
    assert rel_err(ops.gemm_w4a16(x, wq, sc, N, residual=res, variant=variant), y + res.float()) < 1e-2


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("splitk", [2, 3, 4])
def test_gemm_w4_forced_splitk(weights, variant, splitk):
    M, N, K = 65, 272, 2176
    w, wq, sc = weights[N, K]
    torch.manual_seed(splitk)
    x = _rand(M, K)
    ws = torch.full((1 << 20,), float("nan"), device=DEV)
    one = ops.gemm_w4a16(x, wq, sc, N, variant=variant, splitk=1)
    a = ops.gemm_w4a16(x, wq, sc, N, variant=variant, splitk=splitk, workspace=ws)
    assert torch.equal(a, ops.gemm_w4a16(x, wq, sc, N, variant=variant, splitk=splitk, workspace=ws))
    assert rel_err(a, one) < 1e-2 and rel_err(a, ops.w4_reference(x, w)) < 1e-2
    assert not ops.split_counters(ws).any()


def test_gemm_w4_row_blocks_past_2_gib():
    K, N = 16384, 16
    cut = ((1 << 31) - 1) // (K * 2) // 256 * 256
    x = torch.randn(cut + 20, 1, device=DEV).to(torch.bfloat16).expand(-1, K).contiguous()
    w = _rand(N, K, scale=K**-0.5)
    out = ops.gemm_w4a16(x, *ops.pack_skinny_w4(w), N)
    for rows in (slice(0, 40), slice(cut - 20, cut + 20)):
        assert rel_err(out[rows], ops.w4_reference(x[rows], w)) < 1e-2


def test_gemm_w4_graph_replay_matches_eager():
    torch.manual_seed(0)
    M, K, N = 40, 512, 256
    p1 = ops.pack_skinny_w4(ops.interleave_gate_up(_rand(N // 2, K, scale=K**-0.5), _rand(N // 2, K, scale=K**-0.5)))
    p2 = ops.pack_skinny_w4(_rand(K, N // 2, scale=N**-0.5))
    ones = torch.ones(K, device=DEV, dtype=torch.bfloat16)
    def chain(x):
        return ops.gemm_w4a16(ops.gemm_w4a16(ops.rmsnorm(x, ones), *p1, N, act="silu_mul"), *p2, K, residual=x)

    xs = _rand(M, K)
    chain(xs)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s_out = chain(xs)
    for seed in (1, 2, 3):
        torch.manual_seed(seed)
        x = _rand(M, K)
        want = chain(x)
        xs.copy_(x)
        g.replay()
        assert torch.equal(s_out, want)


def test_gemm_w4_rejects_bad_arguments():
    wq, sc = ops.pack_skinny_w4(_rand(64, 256))
    x = _rand(40, 256)
    for call in (lambda: ops.gemm_w4a16(x.float(), wq, sc, 64),  # dtype
                 lambda: ops.gemm_w4a16(_rand(40, 192), wq[: 64 * 96], sc[:96], 64),  # K % 128
                 lambda: ops.gemm_w4a16(x, wq[: 40 * 128], sc[: 40 * 2], 40),  # N % 16
                 lambda: ops.gemm_w4a16(x, wq, sc, 48),  # code count
                 lambda: ops.gemm_w4a16(x, wq, sc, 64, variant=1, splitk=2, workspace=torch.empty(1024, device=DEV))):
        with pytest.raises(ValueError):
            call()


@pytest.fixture(scope="module")
def tiny():
    cfg = tiny_config(**CFG128)
    return cfg, init_llama_shard(cfg, 1, 0, seed=5, device=DEV)


def _llama(tiny, backend, **kw):
    kw = dict(dict(max_batch=2, max_seq=64, weight_dtype="int4", w4_rows="all"), **kw)
    return LlamaTP(tiny[1], tiny[0], backend=backend, device=DEV, **kw)


def _prefill40(m):
    ids, lens = _prompts()
    pos = torch.arange(20, device=DEV, dtype=torch.int32).unsqueeze(0).expand(2, 20).contiguous()
    return m.step(ids, pos, lens, decode=False, k=5)[0], lens


def test_model_fused_all_vs_reference(tiny):
    ref, fus = _llama(tiny, "reference"), _llama(tiny, "fused")
    (rv, lens), (fv, _) = _prefill40(ref), _prefill40(fus)
    assert rel_err(fv, rv) < FUSED_VS_REF
    tok = torch.full((2, 1), 7, dtype=torch.int32, device=DEV)
    rv2, _ = ref.step(tok, lens.view(2, 1).clone(), lens + 1, decode=True, k=5)
    fv2, _ = fus.step(tok, lens.view(2, 1).clone(), lens + 1, decode=True, k=5)
    assert rel_err(fv2, rv2) < FUSED_VS_REF
    for B in (26, 40):  # decode steps on skinny_w4 and on the tiled GEMM
        ids = torch.randint(3, 2000, (B, 4), generator=torch.Generator().manual_seed(6)).to(torch.int32).to(DEV)
        lens = torch.full((B,), 4, dtype=torch.int32, device=DEV)
        ref, fus = (_llama(tiny, b, max_batch=B, max_seq=16) for b in ("reference", "fused"))
        assert decode_top5_deviation(fus, ref, ids, lens) < FUSED_VS_REF


def _spied(m, monkeypatch, run):
    calls = {"w4": 0, "w4g": 0, "linear_layer": 0, "linear_head": 0}
    real = {n: getattr(ops, n) for n in ("linear", "skinny_w4", "gemm_w4a16")}

    def spy(name, key):
        def f(*a, **k):
            calls[key(a) if callable(key) else key] += 1
            return real[name](*a, **k)
        return f

    monkeypatch.setattr(ops, "linear", spy("linear", lambda a: "linear_head" if a[1] is m.p["lm_head"] else "linear_layer"))
    monkeypatch.setattr(ops, "skinny_w4", spy("skinny_w4", "w4"))
    monkeypatch.setattr(ops, "gemm_w4a16", spy("gemm_w4a16", "w4g"))
    m.use_graphs = False  # eager steps so the counters see the calls
    run()
    return calls


def test_model_holds_codes_only_and_routes_by_rows(tiny, monkeypatch):
    cfg = tiny[0]
    m, d = _llama(tiny, "fused", max_batch=26), _llama(tiny, "fused", w4_rows="decode")
    layer = {f"l{i}.{n}" for i in range(cfg.layers) for n in ("qkv", "o", "gate_up", "down")}
    assert set(m.w4) == layer and not layer & set(m.p) and layer <= set(d.p)
    assert m.layer_weight_bytes() == d.layer_weight_bytes() > 0
    calls = _spied(m, monkeypatch, lambda: _prefill40(m))  # 40 rows: tiled, ops.linear sees the lm_head only
    assert calls == {"w4": 0, "w4g": 4 * cfg.layers, "linear_layer": 0, "linear_head": calls["linear_head"]}
    ids, lens = torch.full((26, 1), 7, dtype=torch.int32, device=DEV), torch.ones(26, dtype=torch.int32, device=DEV)
    calls = _spied(m, monkeypatch, lambda: m.step(ids, torch.zeros_like(ids), lens, decode=False, k=5))  # 26 rows
    assert (calls["w4"], calls["w4g"], calls["linear_layer"]) == (4 * cfg.layers, 0, 0)
    calls = _spied(d, monkeypatch, lambda: _prefill40(d))  # the default int4 model: its bf16 copy, never the new op
    assert (calls["w4"], calls["w4g"]) == (0, 0)


def test_model_generate_graphs_and_chunks(tiny):
    from test_kv_prefill_cache_gpu import _check_tokens
    ids, lens = _prompts()
    eager, graphed = _llama(tiny, "fused"), _llama(tiny, "fused")
    eager.use_graphs = False
    assert torch.equal(graphed.generate(ids, lens, GenParams(max_new_tokens=8)), eager.generate(ids, lens, GenParams(max_new_tokens=8)))
    assert graphed._graphs or graphed._dev_graphs  # the decode steps were captured
    ids = torch.randint(3, 2000, (6, 30), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
    lens = torch.tensor([30, 17, 5, 30, 29, 22], dtype=torch.int32, device=DEV)
    ref, m = (_llama(tiny, b, max_batch=6, max_seq=64) for b in ("reference", "fused"))
    out = m.generate(ids, lens, GenParams(max_new_tokens=4), prefill_chunk=8).cpu()
    for b in range(6):
        _check_tokens(ref, ids[b, : int(lens[b])].tolist(), out[b].tolist())
