"""The LoRA oracle, its error bound and its inputs (tests/lora_cases.py), on the CPU: the oracle equals the
merged-weight product, a bf16 rounding model of the kernels stays inside the bound, and every mutant a kernel
could plausibly be misses the oracle by at least 3 bounds on these inputs."""
import pytest
import torch

import lora_cases as L
from mlmicroservicetemplate_amd import ops
from mlmicroservicetemplate_amd.ops import reference as R


def test_ops_exports_the_oracle():
    assert ops.lora_reference is R.lora_qkv


def test_oracle_equals_merged_weights():
    """``qkv + s B (A xn)`` is ``xn (W + s B A)^T``: against an fp64 merged product."""
    c = L.Case(256, (16, 16, 16), "2x17")
    g = torch.Generator().manual_seed(5)
    W = torch.randn(L.N, c.K, generator=g, dtype=torch.float64) * 0.05
    x = c.x.double()
    xn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + L.EPS) * c.gain.double().view(1, -1)
    got = R.lora_qkv((xn @ W.T).float(), c.x, c.gain, c.adapters, c.lora_slot, c.B, c.S, L.WIDTHS, eps=L.EPS)
    for b in range(c.B):
        a = c.adapter_of(b)
        Wm = W.clone()
        if a >= 0:
            c0 = 0
            for j, p in enumerate(R.LORA_MODULES):
                if p in c.adapters[a]:
                    A, Bm, s = c.adapters[a][p]
                    Wm[c0: c0 + L.WIDTHS[j]] += s * (Bm.double() @ A.double())
                c0 += L.WIDTHS[j]
        rows = slice(b * c.S, (b + 1) * c.S)
        want = xn[rows] @ Wm.T
        # fp32 products of 256 terms against fp64: 256 * 2^-24 of the magnitudes, with room
        assert (got[rows].double() - want).abs().max() <= 1e-4 * want.abs().max()


@pytest.mark.parametrize("rows", sorted(L.ROWS))
def test_base_rows_are_bit_identical(rows):
    c = L.Case(256, (8, 0, 16), rows)
    ref = c.reference()
    for b in range(c.B):
        sl = slice(b * c.S, (b + 1) * c.S)
        if c.adapter_of(b) < 0:
            assert torch.equal(ref[sl], c.qkv[sl])
        else:
            assert not torch.equal(ref[sl], c.qkv[sl])


@pytest.mark.parametrize("generic_a", [False, True])
@pytest.mark.parametrize("ranks", L.RANKS)
@pytest.mark.parametrize("K", [256, 4096])
def test_rounding_model_is_inside_the_bound(K, ranks, generic_a):
    """What the kernels round -- A' = bf16(A gain), t to bf16, the sum to bf16 -- stays under the bound; with a
    plain fp32 A (the fold really rounds) under the bound plus the load quantisation's term."""
    c = L.Case(K, ranks, "2x17", generic_a=generic_a)
    ref = c.reference()
    if generic_a:
        assert not torch.equal((c.adapters[0]["q"][0] * c.gain).to(torch.bfloat16).float(), c.adapters[0]["q"][0] * c.gain)
    bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    ads = [{p: (bf(A * c.gain.view(1, -1)), Bm, s) for p, (A, Bm, s) in ad.items()} for ad in c.adapters]
    out = c.qkv.clone()
    rstd = torch.rsqrt(c.x.pow(2).mean(-1, keepdim=True) + L.EPS)
    starts = (0, L.WIDTHS[0], L.WIDTHS[0] + L.WIDTHS[1])
    for b in range(c.B):
        a = c.adapter_of(b)
        if a < 0:
            continue
        sl = slice(b * c.S, (b + 1) * c.S)
        for p, (A, Bm, s) in ads[a].items():
            j = R.LORA_MODULES.index(p)
            out[sl, starts[j]: starts[j] + L.WIDTHS[j]] += (bf(c.x[sl] @ A.T) @ Bm.T) * (s * rstd[sl])
    w = L.worst(bf(out), ref, c.bound(ref, a_quant=generic_a))
    print(f"K={K} ranks={ranks} generic_a={generic_a}: rounding model at {w:.3f} of the bound")
    assert w <= 1.0


def test_every_mutant_is_at_least_three_bounds_away():
    c = L.Case(256, (16, 16, 16), "3x17_slot_ids")
    ref = c.reference()
    bound = c.bound(ref)
    muts = L.mutants(c)
    assert set(muts) == {"neighbour_adapter", "slot_ids_ignored", "k_delta_in_v", "rstd_omitted", "scale_omitted",
                         "gain_not_folded", "last_k_split_dropped", "row16_next_sequence", "base_row_modified"}
    for name, m in muts.items():
        w = L.worst(m, ref, bound)
        print(f"{name}: {w:.1f} bounds")
        assert w >= 3.0, name


def test_inputs_are_what_the_issue_asks():
    c = L.Case(256, (4, 0, 12), "2x17")
    assert float(c.gain.min()) < 0.5 and float(c.gain.max()) > 2.0
    for ad in c.adapters:
        assert set(ad) == {"q", "v"}
        assert all(abs(s - 1.0) > 0.1 for _, _, s in ad.values())
    a0, a1 = c.adapters[0]["q"], c.adapters[1]["q"]
    assert (a0[1] - a1[1]).abs().max() > 0.1
    assert R.lora_scale(8, 16) == 0.5 and R.lora_scale(8, 16, use_rslora=True) == 2.0
