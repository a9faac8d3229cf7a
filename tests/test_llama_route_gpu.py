"""The route of models/llama_route.py is what the fused forward runs: per-op call counts of one prefill
step at row counts on both sides of the 16-row (fused-norm GEMM) and 24-row (packed copies) thresholds,
on a tiny bf16 model at TP = 1 that holds a packed copy of every projection."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPIED = ("skinny_packed", "gemm_rmsnorm", "linear_add_rmsnorm", "linear", "rmsnorm")
SHAPES = {2: (2, 1), 16: (2, 8), 17: (1, 17), 24: (2, 12), 25: (1, 25), 40: (2, 20)}  # rows -> (B, S)


def implied(rt, layers):
    """Calls of one one-shot prefill at TP = 1 on a model with every projection packed and a residual
    stream narrower than ops.linear_add_rmsnorm takes (2048): per layer qkv, o, gate_up, down; the
    lm_head sees <= 2 rows, so it streams its packed copy."""
    want = dict.fromkeys(SPIED, 0)
    want["skinny_packed"] = 1
    if rt.packed:  # all four through the packed copies, norms and residual adds inside (before the
        # fused-norm GEMM on the ladder: ops.gemm_rmsnorm never runs on this model)
        want["skinny_packed"] += 4 * layers
    else:
        assert not rt.fuse  # 16 < 24: no row count of this model is fused-norm but not packed
        want["rmsnorm"] = 2 * layers
        want["linear"] = 4 * layers
    if rt.fuse_rn:  # layer 0's o_proj asks, is refused (narrow rows) and leaves a delta: nobody asks again
        want["linear_add_rmsnorm"] = 1
    return want


def test_prefill_runs_what_the_route_says(monkeypatch):
    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.models.llama import LlamaTP, init_llama_shard, tiny_config

    # head_dim 128: the prefill attention's; every matrix then keeps N % 16 == 0 and K % 32 == 0 (packable)
    cfg = tiny_config(heads=4, kv_heads=2, head_dim=128)
    m = LlamaTP(init_llama_shard(cfg, 1, 0, seed=3, device=DEV), cfg, backend="fused", device=DEV, max_batch=2,
                max_seq=64)
    m.use_graphs = False
    assert set(m.packed) == {f"l{i}.{n}" for i in range(cfg.layers) for n in ("qkv", "o", "gate_up", "down")} | {"lm_head"}
    assert cfg.hidden < 2048 and not m.w4 and not m.fp8
    calls = dict.fromkeys(SPIED, 0)

    def spy(name):
        real = getattr(ops, name)

        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)

        return f

    for name in SPIED:
        monkeypatch.setattr(ops, name, spy(name))
    g = torch.Generator().manual_seed(1)
    for rows, (B, S) in SHAPES.items():
        rt = m._route(B, S, False, False, False)
        # the rules themselves (tests/test_llama_route_cpu.py), at this model's dimensions
        assert (rt.packed, rt.fuse, rt.fold, rt.fuse_rn) == (rows <= 24, rows <= 16, rows <= 24, rows > 24), rows
        assert not (rt.w4 or rt.fp8 or rt.overlap or rt.multi or rt.ar_fuse or rt.fuse_combine), rows
        ids = torch.randint(3, cfg.vocab - 1, (B, S), generator=g).to(torch.int32).to(DEV)
        lens = torch.full((B,), S, device=DEV, dtype=torch.int32)
        pos = torch.arange(S, device=DEV, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
        for name in SPIED:
            calls[name] = 0
        vals, idx = m.step(ids, pos, lens, decode=False, k=4)
        torch.cuda.synchronize()
        assert vals.shape == (B, 4) and bool(torch.isfinite(vals.float()).all())
        assert calls == implied(rt, cfg.layers), rows
    assert m.add_norm_fused == 0 and m.ar_fused_calls == 0
