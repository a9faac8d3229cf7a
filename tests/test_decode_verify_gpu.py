"""Speculative decoding on the GPU: the multi-token verify attention (ops/csrc/decode_verify.hip,
``ops.decode_attention_multi``) vs the fp32 oracle ``ops.reference.attention_ctx`` on the same bf16 cache
contents, per-slot and paged; and the fused ``LlamaTP.verify_step`` / ``generate(speculate=)`` /
``ContinuousLlama(speculate=)`` against the reference backend.

Tolerances: 2e-2 of the largest output magnitude for the kernel (the bound tests/test_flash_ctx_gpu.py
holds its kernel to, for the same reason: P is rounded to bf16 before the PV product), 3e-2 for the
model's top-k values against the reference backend (tests/test_e2e_gpu.py's bound for the Llama cut).
Two fused kernel routes may round differently, and 24.1 % of the reference's own rows on these inputs
have a top-1 / top-2 gap below 1e-2 of the largest candidate -- so tokens are never compared between the
speculative and the plain fused run; every emitted token is checked against the reference backend
teacher-forced on the run's own prefix instead."""
import pytest
import torch

import attn_cases as A
from mlmicroservicetemplate_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
MAX_SEQ = 333  # not a multiple of the split: the last split of a slot ends inside its rows
PASTS = [0, 1, 62, 63, 64, 200]  # steps that straddle the 64-row split / page boundary; a row with one visible key
UNSUPPORTED, BAD_ARG = 1002, 1001


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@pytest.fixture(scope="module")
def ops():
    from mlmicroservicetemplate_amd import ops as o

    o.lib()
    return o


def _valid_counts(T):
    """Valid queries per batch row, ragged in [1, T]; the rows at 62 and 63 keep all of theirs (they cross
    row 64)."""
    return [T, max(1, T - 1), T, T, 1, max(1, T // 2)]


def _case(Hq, Hkv, T, seed=0):
    """qkv of the step (its K / V columns poisoned: the kernel reads K / V from the cache only), a per-slot
    head-major cache and the same rows in a shuffled page pool; everything a launch must not read (unused
    slots, rows >= lens, the tail of a slot's last page) is NaN."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = len(PASTS)
    past = torch.tensor(PASTS, dtype=torch.int32, device=DEV)
    n = torch.tensor(_valid_counts(T), dtype=torch.int32, device=DEV)
    lens = past + n
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    qkv[:, Hq * D:] = float("nan")
    n_slots = B + 3
    slot_ids = torch.tensor([7, 2, 8, 0, 5, 3], dtype=torch.int32, device=DEV)  # slots 1, 4, 6 unused
    kc = torch.full((n_slots, Hkv, MAX_SEQ, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    vc = torch.full_like(kc, float("nan"))
    for b in range(B):
        L, s = int(lens[b]), int(slot_ids[b])
        kc[s, :, :L] = torch.randn(Hkv, L, D, device=DEV, generator=g).to(torch.bfloat16)
        vc[s, :, :L] = torch.randn(Hkv, L, D, device=DEV, generator=g).to(torch.bfloat16)
    pps = -(-MAX_SEQ // 64)
    pages = n_slots * pps + 1
    table = (1 + torch.randperm(pages - 1, device=DEV, generator=g)).view(n_slots, pps).to(torch.int32)
    kp = torch.full((pages, Hkv, 64, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    vp = torch.full_like(kp, float("nan"))
    for s in range(n_slots):
        for j in range(pps):
            r0, r1 = j * 64, min(MAX_SEQ, j * 64 + 64)
            kp[int(table[s, j]), :, : r1 - r0] = kc[s, :, r0:r1]
            vp[int(table[s, j]), :, : r1 - r0] = vc[s, :, r0:r1]
    return dict(B=B, S=T, past=past, n=n, lens=lens, qkv=qkv, slot_ids=slot_ids, kc=kc, vc=vc, table=table, kp=kp,
                vp=vp)


def _valid(out, c):
    """The valid rows of every batch row, concatenated (the others are unspecified)."""
    o = out.view(c["B"], c["S"], -1)
    return torch.cat([o[b, : int(c["n"][b])] for b in range(c["B"])])


@pytest.mark.parametrize("Hq,Hkv,T", [(4, 1, 4), (8, 2, 4), (8, 1, 2), (4, 2, 8), (2, 2, 16)])
def test_kernel_vs_oracle_per_slot_and_paged(ops, Hq, Hkv, T):
    c = _case(Hq, Hkv, T)
    args = (c["past"], c["lens"], c["B"], T, Hq, Hkv, D)
    ref = R.attention_ctx(c["qkv"], c["kc"], c["vc"], *args, slot_ids=c["slot_ids"], head_major=True)
    want = _valid(ref, c)
    # per (row, head) bound: 4 x the rounding model on these inputs (tests/attn_cases.py)
    tol = A.tolerance(A.rows_ctx(c["qkv"], c["kc"], c["vc"], *args, slot_ids=c["slot_ids"]), D)
    outs = {}
    for chunk in (64, 128):
        outs[chunk] = ops.decode_attention_multi(c["qkv"], c["kc"], c["vc"], *args, slot_ids=c["slot_ids"], chunk=chunk)
    outs["paged"] = ops.decode_attention_multi(c["qkv"], c["kp"], c["vp"], *args, slot_ids=c["slot_ids"],
                                               page_table=c["table"])
    # a tight host bound on lens (two splits fewer than the cache holds) changes the grid, not the result
    outs["bound"] = ops.decode_attention_multi(c["qkv"], c["kc"], c["vc"], *args, slot_ids=c["slot_ids"],
                                               max_len=int(c["lens"].max()))
    torch.cuda.synchronize()
    for name, out in outs.items():
        got = _valid(out, c)
        assert torch.isfinite(got.float()).all(), name  # no poisoned row or column was read
        err = rel(got, want)
        print(f"Hq={Hq} Hkv={Hkv} T={T} {name}: rel {err:.4f}")
        assert err < 2e-2, name
        assert A.head_err(got, want, D).max() < tol, name
    # paged == per-slot bit for bit at 64-row splits: the same splits in the same order, only the addressing differs
    assert torch.equal(_valid(outs["paged"], c), _valid(outs[64], c))
    assert torch.equal(_valid(outs["bound"], c), _valid(outs[64], c))


@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (8, 2), (8, 8)])
def test_one_query_matches_decode_attention(ops, Hq, Hkv):
    """T = 1 is single-token decode attention: the matrix-core decode kernel on the same cache."""
    B = 5
    g = torch.Generator(device=DEV).manual_seed(3)
    lens = torch.tensor([1, 64, 65, 200, 333], dtype=torch.int32, device=DEV)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    kc = torch.randn(B, Hkv, MAX_SEQ, D, device=DEV, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, MAX_SEQ, D, device=DEV, generator=g).to(torch.bfloat16)
    one = ops.decode_attention(qkv, kc, vc, lens, Hq, Hkv, D, chunk=64, head_major=True, impl="mfma")
    out = torch.full((B, Hq * D), float("nan"), device=DEV, dtype=torch.bfloat16)
    ret = ops.decode_attention_multi(qkv, kc, vc, lens - 1, lens, B, 1, Hq, Hkv, D, out=out)  # slot_ids=None: slot b
    assert ret.data_ptr() == out.data_ptr()
    err = rel(out, one)
    print(f"Hq={Hq} Hkv={Hkv}: T=1 vs decode_attention rel {err:.4f}")
    assert torch.isfinite(out.float()).all() and err < 2e-2
    rows = A.rows_decode(qkv, kc, vc, lens, Hq, Hkv, D, head_major=True)
    assert A.head_err(out, one, D).max() < 2 * A.tolerance(rows, D)  # two kernels, each within tol of the oracle


def test_empty_rows_are_finite(ops):
    """lens == past (a captured step's warm-up) and lens == 0: nothing valid, nothing read, finite rows."""
    Hq, Hkv, T, B = 8, 2, 4, 3
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    kc = torch.full((B, Hkv, 256, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    kc[1, :, :100] = 1.0
    past = torch.tensor([0, 100, 0], dtype=torch.int32, device=DEV)
    out = ops.decode_attention_multi(qkv, kc, kc, past, past.clone(), B, T, Hq, Hkv, D)
    assert torch.isfinite(out.float()).all() and not out.any()


def test_bad_geometry_is_refused(ops):
    Hq, Hkv, T, B = 4, 2, 4, 1
    qkv = torch.zeros(B * T, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)
    past = torch.zeros(B, dtype=torch.int32, device=DEV)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    hm = torch.zeros(2, Hkv, 64, D, device=DEV, dtype=torch.bfloat16)
    ops.decode_attention_multi(qkv, hm, hm, past, lens, B, T, Hq, Hkv, D)  # the supported layout launches
    rm = torch.zeros(2, 64, Hkv, D, device=DEV, dtype=torch.bfloat16)  # row-major [slots, rows, Hkv, D]
    with pytest.raises(ValueError, match="head-major"):
        ops.decode_attention_multi(qkv, rm, rm, past, lens, B, T, Hq, Hkv, D)
    q64 = torch.zeros(B * T, (Hq + 2 * Hkv) * 64, device=DEV, dtype=torch.bfloat16)
    c64 = torch.zeros(2, Hkv, 64, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="head_dim"):
        ops.decode_attention_multi(q64, c64, c64, past, lens, B, T, Hq, Hkv, 64)
    q16 = torch.zeros(B * 16, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)  # T * G = 32
    with pytest.raises(ValueError, match="<= 16"):
        ops.decode_attention_multi(q16, hm, hm, past, lens, B, 16, Hq, Hkv, D)
    p32 = torch.zeros(4, Hkv, 32, D, device=DEV, dtype=torch.bfloat16)  # pages of 32 rows
    table = torch.tensor([[1, 2]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="64 rows"):
        ops.decode_attention_multi(qkv, p32, p32, past, lens, B, T, Hq, Hkv, D, page_table=table)
    with pytest.raises(TypeError):
        ops.decode_attention_multi(qkv, hm, hm, past.long(), lens, B, T, Hq, Hkv, D)
    # the host entry refuses the same geometries itself (nothing is launched: the output keeps its NaNs)
    lib = ops.lib()
    out = torch.full((16 * B, Hq * D), float("nan"), device=DEV, dtype=torch.bfloat16)
    ws = torch.zeros(1 << 16, device=DEV, dtype=torch.float32)

    def entry(q, cache, pt, pps, t, d, hm_rows, q_stride=None, chunk=64):
        return lib.mls_decode_attention_multi(q.data_ptr(), cache.data_ptr(), cache.data_ptr(), out.data_ptr(),
                                              ws.data_ptr(), ws[1 << 15:].data_ptr(), q_stride or q.shape[1],
                                              Hq * d, past.data_ptr(), lens.data_ptr(), None, pt, pps,
                                              1 if pt else cache.shape[0], B, t, Hq, Hkv, d, cache.shape[0], hm_rows,
                                              64, chunk, 1.0, ops.stream_ptr(torch.device(DEV)))

    assert entry(qkv, rm, None, 0, T, D, 0) == UNSUPPORTED            # row-major cache
    assert entry(q64, c64, None, 0, T, 64, 64) == UNSUPPORTED         # D = 64
    assert entry(q16, hm, None, 0, 16, D, 64) == UNSUPPORTED          # T * G = 32
    assert entry(qkv, p32, table.data_ptr(), 2, T, D, 32) == UNSUPPORTED  # page rows != 64
    assert entry(qkv, hm, None, 0, T, D, 64, q_stride=qkv.shape[1] + 4) == BAD_ARG  # misaligned stride
    assert entry(qkv, hm, None, 0, T, D, 64, chunk=32) == BAD_ARG     # splits of 64 or 128 rows
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()
    assert entry(qkv, hm, None, 0, T, D, 64) == 0                      # and the supported call goes through it
    torch.cuda.synchronize()
    assert torch.isfinite(out[:T].float()).all()


# ------------------------------------------------------------------ the fused model
CFG128 = dict(vocab=2048, layers=2, hidden=512, heads=8, kv_heads=2, head_dim=128, intermediate=1024)
K = 3
NEW = 40


@pytest.fixture(scope="module")
def tiny():
    from mlmicroservicetemplate_amd.models.llama import init_llama_shard, tiny_config

    cfg = tiny_config(**CFG128)
    return cfg, init_llama_shard(cfg, 1, 0, seed=5, device=DEV)


def _prompts():
    ids = torch.randint(3, 2000, (3, 150), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(DEV)
    return ids, torch.tensor([150, 131, 17], dtype=torch.int32, device=DEV)


def _llama(tiny, backend, kv_pages=0):
    from mlmicroservicetemplate_amd.models.llama import LlamaTP

    cfg, p = tiny
    return LlamaTP(p, cfg, backend=backend, device=DEV, max_batch=4, max_seq=512, kv_pages=kv_pages)


@pytest.fixture(scope="module")
def ref_model(tiny):
    """The reference backend every model test compares against (its cache is rewritten by each use)."""
    return _llama(tiny, "reference")


def _check_tokens(ref, prompt, out):
    """Every emitted token, teacher-forced through the reference backend on the run's own prefix, is among
    the reference's top-8 with a value within 3e-2 of the largest |value| of the reference's top-1.  Every
    token is checked, none is left out."""
    full = torch.tensor(list(prompt) + list(out), dtype=torch.int32, device=DEV).unsqueeze(0)
    S = full.shape[1]
    pos = torch.arange(S, dtype=torch.int32, device=DEV).unsqueeze(0)
    v, i = ref.step(full, pos, torch.tensor([S], dtype=torch.int32, device=DEV), decode=False, k=8,
                    past=torch.zeros(1, dtype=torch.int32, device=DEV), all_rows=True)
    L = len(prompt)
    v, i = v[L - 1: S - 1].float().cpu(), i[L - 1: S - 1].cpu()  # row p: the candidates of the token at p + 1
    bound = 3e-2 * float(v.abs().max())
    worst = 0.0
    for t, tok in enumerate(out):
        hit = (i[t] == int(tok)).nonzero()
        assert hit.numel(), f"token {t} ({tok}) is not among the reference's top-8"
        worst = max(worst, float(v[t, 0] - v[t, int(hit[0, 0])]))
    assert worst <= bound, (worst, bound)
    return worst / bound


@pytest.mark.parametrize("kv_pages", [0, 24])
def test_fused_verify_step_vs_reference_backend(tiny, ref_model, kv_pages):
    from mlmicroservicetemplate_amd.models.llama import GenParams

    ids, lens = _prompts()
    B, S = ids.shape
    T, STEPS = 4, 9
    ref, fus = _llama(tiny, "reference", kv_pages), _llama(tiny, "fused", kv_pages)
    cont = ref_model.generate(ids, lens, GenParams(max_new_tokens=NEW)).to(DEV)  # the reference's own greedy run
    if kv_pages:
        for m in (ref, fus):
            for b in range(B):
                m.pages.assign(b, 256)
    pos = torch.arange(S, device=DEV, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
    for m in (ref, fus):
        m.step(ids, pos, lens, decode=False, k=8)
    n = torch.full((B,), T, dtype=torch.int32, device=DEV)
    rv, ri, fv, fi = [], [], [], []
    for s in range(STEPS):  # teacher-forced: both backends are fed the reference's tokens
        feed = cont[:, T * s: T * s + T].to(torch.int32)
        past = lens + T * s
        v, i = ref.verify_step(feed, past, n, 8)
        rv.append(v.reshape(B * T, -1).clone()), ri.append(i.reshape(B * T, -1).clone())
        v, i = fus.verify_step(feed, past, n, 8, max_ctx=S + T * s + T)
        fv.append(v.reshape(B * T, -1).clone()), fi.append(i.reshape(B * T, -1).clone())
    rv, ri, fv, fi = torch.cat(rv).float(), torch.cat(ri), torch.cat(fv).float(), torch.cat(fi)
    assert rv.shape[0] == 108
    # the reference's rows reproduce its own plain run (verification through the chunk path is exact there)
    want = torch.stack([cont[:, T * s + t + 1] for s in range(STEPS) for t in range(T)], 0)  # [36, B]
    got = ri[:, 0].view(STEPS, B, T).permute(0, 2, 1).reshape(STEPS * T, B)
    assert torch.equal(got.to(torch.int32), want.to(torch.int32))
    err = rel(fv, rv)
    gap = (rv[:, 0] - rv[:, 1]) / rv.abs().max()
    keep = gap > 1e-2
    left_out = 1.0 - float(keep.float().mean())
    print(f"kv_pages={kv_pages}: fused verify vs reference top-k values rel {err:.4f}; gap filter leaves out "
          f"{100 * left_out:.1f} % of {rv.shape[0]} rows")
    assert err <= 3e-2
    assert left_out <= 0.35
    assert torch.equal(fi[:, 0][keep], ri[:, 0][keep])
    if fus.use_graphs:
        assert len(fus._ver_graphs) >= 1  # the step ran as a captured graph


def _oracle_drafter(prompts, conts):
    """Right drafts for every sequence of a recorded run (distinct prompts): the tokens that followed."""
    prompts = [list(p) for p in prompts]

    def draft(tokens, n):
        toks = list(tokens)
        for p, c in zip(prompts, conts):
            e = len(toks) - len(p)
            if e > 0 and toks[: len(p)] == p and toks[len(p):] == list(c[:e]):
                return list(c[e: e + n])
        return [toks[-1]] * n

    return draft


@pytest.mark.parametrize("kv_pages", [0, 24])
def test_fused_generate_speculative(tiny, ref_model, kv_pages):
    from mlmicroservicetemplate_amd.models.llama import GenParams

    ids, lens = _prompts()
    gp = GenParams(max_new_tokens=NEW)
    plain = _llama(tiny, "fused", kv_pages).generate(ids, lens, gp).cpu()
    prompts = [ids[b, : int(lens[b])].tolist() for b in range(3)]
    oracle = _oracle_drafter(prompts, plain.tolist())  # drafts = the plain fused run's continuation
    m = _llama(tiny, "fused", kv_pages)
    got = m.generate(ids, lens, gp, speculate=K, drafter=oracle).cpu()
    st = dict(m.spec_stats)
    assert got.shape == plain.shape
    for b in range(3):
        frac = _check_tokens(ref_model, prompts[b], got[b].tolist())
        print(f"kv_pages={kv_pages} row {b}: worst top-1 distance {frac:.3f} of the bound; "
              f"{int((got[b] == plain[b]).sum())}/{NEW} tokens equal the plain fused run")
    print(f"kv_pages={kv_pages}: {st}")
    assert st["accepted"] > 0 and st["steps"] < NEW - 1
    if kv_pages:
        assert m.pages.free_pages == kv_pages - 1
    again = m.generate(ids, lens, gp, speculate=K, drafter=oracle).cpu()  # over the first run's stale cache rows
    assert torch.equal(again, got)
    if kv_pages:
        assert m.pages.free_pages == kv_pages - 1


@pytest.mark.parametrize("kv_pages", [0, 24])
def test_fused_serving_speculative(tiny, ref_model, kv_pages):
    from mlmicroservicetemplate_amd.models.llama import GenParams
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    g = torch.Generator().manual_seed(5)
    mk = lambda n: torch.randint(3, 2000, (n,), generator=g).tolist()  # noqa: E731
    loop = mk(12)
    reqs = [(mk(150), GenParams(max_new_tokens=9)), (loop * 4, GenParams(max_new_tokens=12)),  # a prompt that repeats
            (mk(70), GenParams(max_new_tokens=10)), (mk(3), GenParams(max_new_tokens=7))]
    model = _llama(tiny, "fused", kv_pages)
    eng = ContinuousLlama(model, speculate=K)
    futs = [eng.submit(*reqs[0])]
    eng.run_iteration(eng._leader_admissions())
    futs += [eng.submit(ids, gp) for ids, gp in reqs[1:]]
    for _ in range(100):
        if all(f.done() for f in futs):
            break
        eng.run_iteration(eng._leader_admissions())
    outs = [f.result(timeout=0) for f in futs]
    assert not eng.dev_mode and eng.failures == 0
    for (prompt, gp), out in zip(reqs, outs):
        assert 1 <= len(out) <= gp.max_new_tokens
        assert len(out) == gp.max_new_tokens or out[-1] in eng.eos
        _check_tokens(ref_model, prompt, out)
    st = eng.stats()
    print(f"kv_pages={kv_pages}: {st}")
    assert st["active"] == 0 and st["queued"] == 0 and all(s is None for s in eng.slots)
    assert st["spec_steps"] >= 1 and st["tokens"] == sum(len(o) for o in outs)
    if model.use_graphs:
        # 1 -> 4 -> fewer decoding sequences: several captured steps, replayed after larger ones were captured --
        # each holds the split-KV workspace its launches were captured with
        ws = [g[-1] for g in model._ver_graphs.values()]
        assert len(ws) >= 2 and all(w.numel() > 0 for w in ws) and len({w.data_ptr() for w in ws}) == len(ws)
    if kv_pages:
        assert st["kv_pages_free"] == kv_pages - 1


def test_fused_refusals(tiny, monkeypatch):
    from mlmicroservicetemplate_amd.models.llama import GenParams, LlamaTP, init_llama_shard, tiny_config
    from mlmicroservicetemplate_amd.models.llama_serving import ContinuousLlama

    cfg, p = tiny
    ids, lens = _prompts()
    m = _llama(tiny, "fused")
    with pytest.raises(ValueError, match="<= 16"):  # G = 4: at most 4 positions per step
        m.generate(ids, lens, GenParams(2), speculate=4)
    with pytest.raises(ValueError, match="<= 16"):
        ContinuousLlama(m, speculate=4)
    m8 = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=4, max_seq=256, kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        m8.generate(ids, lens, GenParams(2), speculate=K)
    monkeypatch.setenv("MLS_KV_HEAD_MAJOR", "0")
    rm = LlamaTP(p, cfg, backend="fused", device=DEV, max_batch=4, max_seq=256)
    with pytest.raises(ValueError, match="head-major"):
        rm.generate(ids, lens, GenParams(2), speculate=K)
    monkeypatch.delenv("MLS_KV_HEAD_MAJOR")
    cfg32 = tiny_config()  # head_dim 32
    m32 = LlamaTP(init_llama_shard(cfg32, 1, 0, seed=1, device=DEV), cfg32, backend="fused", device=DEV, max_batch=2,
                  max_seq=64)
    with pytest.raises(ValueError, match="head_dim"):
        m32.check_speculate(K)


def test_verify_attention_routes_agree(tiny, monkeypatch):
    """MLS_VERIFY_ATTN=ctx (the A/B arm) runs the same verify step through the chunk kernel."""
    ids, lens = _prompts()
    B, S = ids.shape
    pos = torch.arange(S, device=DEV, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
    feed = torch.randint(3, 2000, (B, 4), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(DEV)
    n = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    res = []
    for arm in ("multi", "ctx"):
        monkeypatch.setenv("MLS_VERIFY_ATTN", arm)
        m = _llama(tiny, "fused")
        assert m.verify_attn == arm
        m.step(ids, pos, lens, decode=False, k=8)
        v, i = m.verify_step(feed, lens, n, 8, max_ctx=S + 4)
        res.append(torch.cat([v[b, : int(n[b])] for b in range(B)]).float().clone())
    err = rel(res[0], res[1])
    print(f"verify step, multi vs ctx attention: top-k values rel {err:.4f}")
    assert err <= 3e-2
