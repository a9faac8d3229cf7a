"""SHA-256 of every output of the skinny-GEMM family on seeded inputs, one JSON line per call: the
before / after record of a refactor of csrc/skinny_gemm.hip, skinny_w4.hip and skinny_tiles.h that must
not move a bit.

Covers ops.gemm / ops.gemm_rmsnorm (row-major and LDS kernels, splitk 0 / 1 / 4), ops.skinny_packed
(the variant list of test_packed_plain), ops.skinny_packed_combine (the lens lists of
test_packed_combine_matches_attention_then_gemm, both variants), ops.skinny_fp8 (variants 0-2) and
ops.skinny_w4 (variants 0-12); prologue plain / norm / add-norm (resid_out hashed too), epilogue none /
bias + residual / silu_mul.  ops.gemm has no norm prologue and ops.gemm_rmsnorm no bias / residual, so
the row-major family takes the modes each entry point offers.  Inputs come from a CPU generator, so they
do not depend on the library.  Two libraries compute the same thing iff their files are identical:

    python tools/probe/skinny_dump.py --out new.jsonl
    MLS_LIB_OVERRIDE=/path/to/parent/libmls_kernels.so python tools/probe/skinny_dump.py --out parent.jsonl
    cmp parent.jsonl new.jsonl

``--summary`` also writes the record that is small enough to keep: one line per (op, N, K, M) with the number
of calls and tensors and the SHA-256 over that group's lines of the per-call file
(``--summarize-only`` makes it from an existing per-call file, without a GPU).
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

DEV = "cuda:0"
PROLOGUES = ("plain", "norm", "add_norm")
EPILOGUES = ("none", "bias_res", "silu_mul")
PACKED_VARIANTS = list(range(14)) + [17, 25, 26, 27, 28, 29]
COMBINE_LENS = ([300], [1, 64, 65, 700], [129, 20])


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


class Inputs:
    """One seeded set per (M, N, K): x, delta, W (gate/up rows are what they are: silu_mul only needs
    N % 16 == 0), bias, residual."""

    def __init__(self, M, N, K, seed):
        g = torch.Generator().manual_seed(seed)
        bf = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16).to(DEV)
        self.x, self.d = bf(M, K), bf(M, K)
        self.w = bf(N, K, scale=K**-0.5)
        self.bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
        self.res = bf(M, N)


def epilogue_kw(inp, epi):
    if epi == "bias_res":
        return dict(bias=inp.bias, residual=inp.res)
    return dict(act="silu_mul") if epi == "silu_mul" else {}


def prologue_kw(inp, pro):
    """-> (keyword arguments of the packed-style entry points, resid_out or None)"""
    if pro == "add_norm":
        r = torch.zeros_like(inp.x)
        return dict(delta=inp.d, resid_out=r, norm=True), r
    return (dict(norm=True) if pro == "norm" else {}), None


def record(rows, op, case, out, resid):
    row = {"op": op, **case, "out": sha(out)}
    if resid is not None:
        row["resid_out"] = sha(resid)
    rows.append(row)


def dump_gemm(ops, rows):
    ws = torch.empty(4 * 32 * (25600 + 1), device=DEV, dtype=torch.float32)
    for N, K in ((768, 1024), (48, 104), (25600, 512)):
        for M in (1, 4, 5, 16, 17, 32):
            inp = Inputs(M, N, K, 1000 + M + N)
            for splitk in (0, 1, 4):
                case = dict(M=M, N=N, K=K, splitk=splitk)
                if M <= 16:  # ops.gemm routes M <= 16 to the skinny kernels
                    for epi in EPILOGUES:
                        out = ops.gemm(inp.x, inp.w, workspace=ws, splitk=splitk, **epilogue_kw(inp, epi))
                        record(rows, "gemm", dict(case, pro="plain", epi=epi), out, None)
                for pro in ("norm", "add_norm"):
                    for epi in ("none", "silu_mul"):
                        r = torch.zeros_like(inp.x) if pro == "add_norm" else None
                        out = ops.gemm_rmsnorm(inp.x, inp.w, inp.d if r is not None else None, r, workspace=ws,
                                               splitk=splitk, **epilogue_kw(inp, epi))
                        record(rows, "gemm_rmsnorm", dict(case, pro=pro, epi=epi), out, r)


def dump_family(ops, rows, name, call, pack, variants, Ms, NKs):
    for N, K in NKs:
        for M in Ms:
            inp = Inputs(M, N, K, 2000 + M + N)
            packed = pack(inp.w)
            for variant in variants:
                for pro in PROLOGUES:
                    for epi in EPILOGUES:
                        kw, r = prologue_kw(inp, pro)
                        out = call(inp.x, packed, N, variant=variant, **kw, **epilogue_kw(inp, epi))
                        record(rows, name, dict(M=M, N=N, K=K, variant=variant, pro=pro, epi=epi), out, r)


def dump_combine(ops, rows):
    for lens_list in COMBINE_LENS:
        g = torch.Generator().manual_seed(len(lens_list))
        B, Hq, Hkv, D, L, N = len(lens_list), 32, 8, 128, 1024, 4096
        bf = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16).to(DEV)
        kc, vc, q = bf(B, L, Hkv, D), bf(B, L, Hkv, D), bf(B, (Hq + 2 * Hkv) * D)
        wp, res = ops.pack_skinny(bf(N, Hq * D, scale=(Hq * D) ** -0.5)), bf(B, N)
        lens = torch.tensor(lens_list, device=DEV, dtype=torch.int32)
        a, parts = ops.decode_attention(q, kc, vc, lens, Hq, Hkv, D, max_len=L, combine=False)
        for variant in (1, 9):
            out = ops.skinny_packed_combine(a, parts, wp, N, residual=res, variant=variant)
            record(rows, "skinny_packed_combine", dict(lens=lens_list, variant=variant, attn=sha(a)), out, None)


def line(row):
    return json.dumps(row, sort_keys=True, separators=(",", ":")) + "\n"


def summarize(rows, path):
    groups = {}
    for row in rows:
        key = (row["op"], row.get("N"), row.get("K"), row.get("M"), json.dumps(row.get("lens")))
        g = groups.setdefault(key, {"calls": 0, "tensors": 0, "h": hashlib.sha256()})
        g["calls"] += 1
        g["tensors"] += 1 + ("resid_out" in row)
        g["h"].update(line(row).encode())
    with open(path, "w") as f:
        for (op, N, K, M, lens), g in groups.items():
            f.write(line({"op": op, "N": N, "K": K, "M": M, "lens": json.loads(lens), "calls": g["calls"],
                          "tensors": g["tensors"], "sha256": g["h"].hexdigest()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--summary", help="also write the per-(op, shape) digest file")
    ap.add_argument("--summarize-only", action="store_true", help="--out exists: only write --summary from it")
    ap.add_argument("--only", default="gemm,packed,combine,fp8,w4")
    a = ap.parse_args()
    if a.summarize_only:
        with open(a.out) as f:
            summarize([json.loads(ln) for ln in f], a.summary)
        return
    from mlmicroservicetemplate_amd import ops

    rows, only = [], a.only.split(",")
    if "gemm" in only:
        dump_gemm(ops, rows)
    if "packed" in only:
        dump_family(ops, rows, "skinny_packed", ops.skinny_packed, lambda w: ops.pack_skinny(w), PACKED_VARIANTS,
                    (1, 3, 4, 5, 16, 17, 32), ((256, 512), (48, 96), (64, 14336), (6144, 256)))
    if "combine" in only:
        dump_combine(ops, rows)
    if "fp8" in only:
        dump_family(ops, rows, "skinny_fp8", lambda x, p, N, **kw: ops.skinny_fp8(x, p[0], p[1], N, **kw),
                    ops.pack_skinny_fp8, (0, 1, 2), (1, 4), ((48, 128), (256, 4096)))
    if "w4" in only:
        dump_family(ops, rows, "skinny_w4", lambda x, p, N, **kw: ops.skinny_w4(x, p[0], p[1], N, **kw),
                    ops.pack_skinny_w4, range(13), (1, 4, 5, 17, 32), ((64, 128), (256, 4096), (16384, 512)))
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        for row in rows:
            f.write(line(row))
    if a.summary:
        summarize(rows, a.summary)
    print(f"{len(rows)} calls -> {a.out}", flush=True)


if __name__ == "__main__":
    main()
