"""SHA-256 of every output of the tiled GEMMs on seeded inputs, one JSON line per call: the before / after
record of a refactor of csrc/gemm_ring.h, gemm_tile.hip and gemm_w8a8.hip that must not move a bit.

Covers ops.gemm_tile over the cfgs and shapes of test_gemm_tile_epilogues and the split-K cases of
test_gemm_tile_splitk with every epilogue kind (bias, GELU, residual, bias + residual, SiLU-mul), ops.gemm_tile_ln
at the shapes of tests/test_ln_fold_gpu.py (folded projection none / GELU; residual projection with and without
a LayerNorm'd residual, with and without row partials, the partials hashed too), and ops.gemm_w8a8 over every
variant x {plain, bias + residual, silu_mul} at the shapes of tests/test_w8a8_gpu.py (the split-K pairs
included).  Inputs come from a CPU generator, so they do not depend on the library.  Two libraries compute
the same thing iff their files are identical:

    python tools/probe/gemm_tile_dump.py --out new.jsonl
    MLS_LIB_OVERRIDE=/path/to/parent/libmls_kernels.so python tools/probe/gemm_tile_dump.py --out parent.jsonl
    cmp parent.jsonl new.jsonl

``--summary`` also writes the record that is small enough to keep: one line per (op, M, N, K) with the number of
calls and tensors and the SHA-256 over that group's lines of the per-call file (``--summarize-only`` makes it
from an existing per-call file, without a GPU).
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

DEV = "cuda:0"
TILE_CFGS = (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 15, 16, 21, 22)
TILE_SHAPES = ((300, 528, 192, 0), (1024, 1280, 512, 3), (4096, 768, 768, 0))  # M, N, K, grid_cap
SPLITK_CFGS = (1, 2, 15, 16)
SPLITK_SHAPES = ((300, 528, 256, 2), (4096, 768, 3072, 3), (1024, 1280, 1536, 4))  # M, N, K, S
LN_FOLDED = ((4096, 2304, 768, 0), (1000, 3072, 768, 0), (4096, 768, 768, 16), (512, 768, 768, 5),
             (300, 512, 768, 4), (777, 2304, 768, 15))
LN_RESIDUAL = ((4096, 768, 3072, 0), (4096, 768, 768, 2), (333, 768, 3072, 15), (4096, 768, 3072, 10),
               (1000, 1024, 768, 4), (700, 768, 768, 5))
W8_SHAPES = tuple((M, N, K) for N in (16, 48, 272) for K in (128, 384, 2176) for M in (1, 5, 17, 33, 130, 257)) \
    + ((4, 272, 512), (40, 272, 512), (257, 272, 256))
W8_SPLITK = ((3, 2), (3, 4), (4, 2), (4, 8), (5, 4), (5, 8), (1, 2), (2, 2))  # variant, splitk at M 40, N 272, K 1024
W8_WALK = ((5, 257, 3840, 256, 1), (4, 257, 3840, 512, 2))  # variant, M, N, K, splitk: blocks walk two units


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    bf = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16).to(DEV)
    f32 = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, generator=g) * scale + shift).to(DEV)
    return bf, f32


def partials(t):
    tf = t.float().view(t.shape[0], t.shape[1] // 128, 128)
    return torch.stack([tf.sum(2), (tf * tf).sum(2)], 2).reshape(-1).contiguous()


def tile_epilogues(ops, rows, a, w, b, r, case, **kw):
    """every epilogue kind of ops.gemm_tile on one (a, w)"""
    N = w.shape[0]
    half = N // 2 // 16 * 16
    gu = ops.interleave_gate_up(w[:half].contiguous(), w[N - half:].contiguous())
    for epi, call in (("bias", lambda: ops.gemm_tile(a, w, b, **kw)),
                      ("gelu", lambda: ops.gemm_tile(a, w, b, act=ops.ACT_GELU, **kw)),
                      ("res", lambda: ops.gemm_tile(a, w, None, residual=r, **kw)),
                      ("bias_res", lambda: ops.gemm_tile(a, w, b, residual=r, **kw)),
                      ("silu_mul", lambda: ops.gemm_tile(a, gu, None, act=ops.ACT_SILU_MUL, **kw))):
        rows.append({"op": "gemm_tile", **case, "epi": epi, "out": sha(call())})


def dump_tile(ops, rows):
    for M, N, K, cap in TILE_SHAPES:
        bf, f32 = gen(100 + M + N)
        a, w, b, r = bf(M, K), bf(N, K, scale=K**-0.5), f32(N, scale=0.1), bf(M, N)
        for cfg in TILE_CFGS:
            tile_epilogues(ops, rows, a, w, b, r, dict(M=M, N=N, K=K, cfg=cfg, cap=cap, splitk=1), cfg=cfg, grid_cap=cap)
    ws = torch.zeros(16 << 20, device=DEV, dtype=torch.float32)
    for M, N, K, S in SPLITK_SHAPES:
        bf, f32 = gen(200 + M + N)
        a, w, b, r = bf(M, K), bf(N, K, scale=K**-0.5), f32(N, scale=0.1), bf(M, N)
        for cfg in SPLITK_CFGS:
            tile_epilogues(ops, rows, a, w, b, r, dict(M=M, N=N, K=K, cfg=cfg, cap=0, splitk=S), cfg=cfg, splitk=S,
                           workspace=ws)
    torch.cuda.synchronize()
    assert int(ops.split_counters(ws).abs().sum().item()) == 0


def dump_ln(ops, rows):
    for M, N, K, cfg in LN_FOLDED:
        bf, f32 = gen(300 + M + N)
        h, w, b = bf(M, K) + bf(M, 1, scale=0.3), bf(N, K, scale=K**-0.5), f32(N, scale=0.1)
        gam, bet = f32(K, scale=0.2, shift=1.0), f32(K, scale=0.1)
        w2, c, b2 = ops.fold_layernorm(w, b, gam, bet)
        for act in ("none", "gelu"):
            out = ops.gemm_tile_ln(h, w2, b2, act=act, fold_c=c, ln_part=partials(h), cfg=cfg)
            rows.append({"op": "gemm_tile_ln", "form": "folded", "M": M, "N": N, "K": K, "cfg": cfg, "act": act,
                         "out": sha(out)})
    for M, N, K, cfg in LN_RESIDUAL:
        bf, f32 = gen(400 + M + K)
        a, w, b, r = bf(M, K), bf(N, K, scale=K**-0.5), f32(N, scale=0.1), bf(M, N) + bf(M, 1, scale=0.3)
        gam = f32(N, scale=0.2, shift=1.0)
        for ln_res in (False, True):
            kw = dict(ln_part=partials(r), ln_g=gam) if ln_res else {}
            for stats in (False, True):
                part = ops.ln_partials(M, N, DEV).fill_(float("nan")) if stats else None
                out = ops.gemm_tile_ln(a, w, b, residual=r, stats_part=part, cfg=cfg, **kw)
                row = {"op": "gemm_tile_ln", "form": "residual", "M": M, "N": N, "K": K, "cfg": cfg, "ln_res": ln_res,
                       "out": sha(out)}
                if stats:
                    row["stats_part"] = sha(part)
                rows.append(row)


def w8_epilogues(ops, rows, xq, xs, wq, ws, b, r, N, case, **kw):
    for epi, ekw in (("none", {}), ("bias_res", dict(bias=b, residual=r)), ("silu_mul", dict(bias=b, act="silu_mul"))):
        rows.append({"op": "gemm_w8a8", **case, "epi": epi, "out": sha(ops.gemm_w8a8(xq, xs, wq, ws, N, **ekw, **kw))})


def dump_w8(ops, rows):
    def operands(M, N, K, seed):
        bf, f32 = gen(seed)
        wq, ws = ops.pack_w8(bf(N, K, scale=K**-0.5))
        xq, xs = ops.quant_rows_fp8(bf(M, K))
        return xq, xs, wq, ws, f32(N, scale=0.1), bf(M, N)

    for M, N, K in W8_SHAPES:
        args = operands(M, N, K, 500 + M + N + K)
        for variant in range(ops.W8A8_VARIANTS):
            w8_epilogues(ops, rows, *args, N, dict(M=M, N=N, K=K, variant=variant, splitk=0), variant=variant)
    work = torch.zeros(4 << 20, device=DEV, dtype=torch.float32)
    args = operands(40, 272, 1024, 600)
    for variant, splitk in W8_SPLITK:
        w8_epilogues(ops, rows, *args, 272, dict(M=40, N=272, K=1024, variant=variant, splitk=splitk), variant=variant,
                     splitk=splitk, workspace=work)
    for variant, M, N, K, splitk in W8_WALK:
        args = operands(M, N, K, 700 + K)
        w8_epilogues(ops, rows, *args, N, dict(M=M, N=N, K=K, variant=variant, splitk=splitk), variant=variant,
                     splitk=splitk, workspace=work)
    torch.cuda.synchronize()
    assert int(ops.split_counters(work).abs().sum().item()) == 0


def line(row):
    return json.dumps(row, sort_keys=True, separators=(",", ":")) + "\n"


def summarize(rows, path):
    groups = {}
    for row in rows:
        g = groups.setdefault((row["op"], row["M"], row["N"], row["K"]), {"calls": 0, "tensors": 0, "h": hashlib.sha256()})
        g["calls"] += 1
        g["tensors"] += 1 + ("stats_part" in row)
        g["h"].update(line(row).encode())
    with open(path, "w") as f:
        for (op, M, N, K), g in groups.items():
            f.write(line({"op": op, "M": M, "N": N, "K": K, "calls": g["calls"], "tensors": g["tensors"],
                          "sha256": g["h"].hexdigest()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--summary", help="also write the per-(op, shape) digest file")
    ap.add_argument("--summarize-only", action="store_true", help="--out exists: only write --summary from it")
    ap.add_argument("--only", default="tile,ln,w8")
    a = ap.parse_args()
    if a.summarize_only:
        with open(a.out) as f:
            summarize([json.loads(ln) for ln in f], a.summary)
        return
    from mlmicroservicetemplate_amd import ops

    rows, only = [], a.only.split(",")
    if "tile" in only:
        dump_tile(ops, rows)
    if "ln" in only:
        dump_ln(ops, rows)
    if "w8" in only:
        dump_w8(ops, rows)
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        for row in rows:
            f.write(line(row))
    if a.summary:
        summarize(rows, a.summary)
    print(f"{len(rows)} calls -> {a.out}", flush=True)


if __name__ == "__main__":
    main()
