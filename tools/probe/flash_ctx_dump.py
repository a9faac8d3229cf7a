"""SHA-256 (its first 64 bits) of every output of the context-attention kernels on seeded inputs: the
before / after record of a refactor of csrc/flash_ctx.hip that must not move a bit.  One JSON line per
(shape, cache type, layout) with the hashes of its calls, one per split count, in lists.

Covers ops.flash_attention_ctx and ops.flash_attention_ctx_fp8 at the shapes of tests/test_flash_ctx_gpu.py,
test_flash_ctx_split_gpu.py and test_flash_ctx_fp8_gpu.py: (Hq, Hkv) in (8, 2), (4, 1), (8, 1); S in 1,
16, 63, 64, 65, 130; ``past`` ragged in one batch (0, 1, 63, 64, 65, 200), 333 rows per slot, some rows
with fewer valid queries than S, shuffled slot_ids; the per-slot cache and the same rows in a page pool
behind a shuffled table; splits 1 (the unsplit launch), 2, 3 and 8 (over at most 6 key tiles: empty
splits); and the 18-tile batch (lens 1005 / 41) at 4 and 16 splits.  Everything a launch must not read is
NaN.  The valid rows (query i < lens[b] - past[b]) and the padding rows of an output are hashed
separately, and ``padding_zero`` says whether the padding rows are all zero.  Inputs come from a CPU
generator and the e4m3 caches from ops.reference.kv_quant_fp8 of the bf16 rows, so they do not depend on
the library.  Two libraries compute the same thing iff their files are identical:

    python tools/probe/flash_ctx_dump.py --out new.jsonl
    MLS_LIB_OVERRIDE=/path/to/parent/libmls_kernels.so python tools/probe/flash_ctx_dump.py --out parent.jsonl
    python tools/probe/flash_ctx_dump.py --compare parent.jsonl new.jsonl

``--compare`` needs no GPU: it prints the calls whose hashes differ and a count per (kv_dtype, splits).
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

DEV = "cuda:0"
D = 128
PASTS = [0, 1, 63, 64, 65, 200]
SLOT_IDS = (7, 2, 8, 0, 5, 3)


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def valid_counts(S, B):
    return [S, max(1, S - 1), max(1, S // 2), S, max(1, S - 7), S][:B]


def paged(src, table, pps, poison):
    """The rows of a per-slot cache [slots, Hkv, max_seq(, D)] in a page pool [pages, Hkv, 64(, D)]"""
    n_slots, Hkv, max_seq = src.shape[:3]
    tail = tuple(src.shape[3:])
    pad = pps * 64 - max_seq
    rows = torch.nn.functional.pad(src, (0, 0) * len(tail) + (0, pad), value=poison)
    dst = torch.full((n_slots * pps + 1, Hkv, 64) + tail, poison, dtype=src.dtype)
    perm = (0, 2, 1, 3) + ((4,) if tail else ())
    dst[table.long().flatten()] = rows.view(n_slots, Hkv, pps, 64, *tail).permute(*perm).reshape(
        n_slots * pps, Hkv, 64, *tail)
    return dst


def make_case(R, Hq, Hkv, S, seed, pasts=PASTS, max_seq=333, slot_ids=SLOT_IDS):
    g = torch.Generator().manual_seed(seed)
    B = len(pasts)
    past = torch.tensor(pasts, dtype=torch.int32)
    n = torch.tensor(valid_counts(S, B), dtype=torch.int32)
    lens = past + n
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    qkv[:, Hq * D:] = float("nan")
    n_slots = B + 3
    slots = torch.tensor(list(slot_ids[:B]), dtype=torch.int32)
    nan8 = 0x7F
    c16 = [torch.full((n_slots, Hkv, max_seq, D), float("nan"), dtype=torch.bfloat16) for _ in range(2)]
    c8 = [torch.full((n_slots, Hkv, max_seq, D), nan8, dtype=torch.uint8) for _ in range(2)]
    sc = [torch.full((n_slots, Hkv, max_seq), float("nan"), dtype=torch.float32) for _ in range(2)]
    for b in range(B):
        L, s = int(lens[b]), int(slots[b])
        for i in range(2):  # rows of different magnitude, so the per-row scales matter
            rows = torch.randn(Hkv, L, D, generator=g) * (0.25 + 2 * torch.rand(Hkv, L, 1, generator=g))
            rows = rows.to(torch.bfloat16)
            c16[i][s, :, :L] = rows
            c8[i][s, :, :L], sc[i][s, :, :L] = R.kv_quant_fp8(rows)
    pps = -(-max_seq // 64)
    table = (1 + torch.randperm(n_slots * pps, generator=g)).view(n_slots, pps).to(torch.int32)
    to = lambda ts: tuple(t.to(DEV) for t in ts)
    return dict(
        B=B, S=S, Hq=Hq, Hkv=Hkv, n=n.tolist(), max_ctx=int(lens.max()), qkv=qkv.to(DEV), past=past.to(DEV),
        lens=lens.to(DEV), slot_ids=slots.to(DEV), table=table.to(DEV),
        caches={("bf16", False): to(c16), ("fp8", False): to(c8 + sc),
                ("bf16", True): to([paged(t, table, pps, float("nan")) for t in c16]),
                ("fp8", True): to([paged(t, table, pps, nan8) for t in c8]
                                  + [paged(t, table, pps, float("nan")) for t in sc])})


def dump_case(ops, rows, c, name, splits_list):
    B, S, Hq = c["B"], c["S"], c["Hq"]
    for (kv_dtype, is_paged), caches in c["caches"].items():
        fn = ops.flash_attention_ctx if kv_dtype == "bf16" else ops.flash_attention_ctx_fp8
        for splits in splits_list:
            out = torch.full((B * S, Hq * D), float("nan"), device=DEV, dtype=torch.bfloat16)
            kw = dict(splits=splits, max_ctx=c["max_ctx"]) if splits > 1 else {}
            fn(c["qkv"], *caches, c["past"], c["lens"], B, S, Hq, c["Hkv"], D, slot_ids=c["slot_ids"],
               page_table=c["table"] if is_paged else None, out=out, **kw)
            o = out.view(B, S, -1).cpu()
            valid = torch.cat([o[b, : c["n"][b]] for b in range(B)])
            padding = torch.cat([o[b, c["n"][b]:] for b in range(B)])
            rows.append({"case": name, "Hq": Hq, "Hkv": c["Hkv"], "S": S, "kv_dtype": kv_dtype, "paged": is_paged,
                         "splits": splits, "valid": sha(valid), "padding": sha(padding),
                         "padding_rows": padding.shape[0], "padding_zero": not bool(padding.view(torch.int16).any())})


GROUP = ("case", "Hq", "Hkv", "S", "kv_dtype", "paged", "padding_rows")
PER_CALL = ("splits", "valid", "padding", "padding_zero")


def write(rows, path):
    """One line per group of calls that differ in ``splits`` only (PER_CALL values as lists)."""
    groups = {}
    for row in rows:
        g = groups.setdefault(tuple(row[k] for k in GROUP), {k: [] for k in PER_CALL})
        for k in PER_CALL:
            g[k].append(row[k])
    with open(path, "w") as f:
        for key, g in groups.items():
            f.write(json.dumps({**dict(zip(GROUP, key)), **g}, separators=(",", ":")) + "\n")


def read(path):
    with open(path) as f:
        lines = [json.loads(ln) for ln in f]
    return [{**{k: ln[k] for k in GROUP}, **dict(zip(PER_CALL, call))}
            for ln in lines for call in zip(*(ln[k] for k in PER_CALL))]


def compare(a_path, b_path):
    a, b = read(a_path), read(b_path)
    key = lambda r: tuple(r[k] for k in ("case", "Hq", "Hkv", "S", "kv_dtype", "paged", "splits"))
    assert [key(r) for r in a] == [key(r) for r in b], "the two files list different calls"
    groups = {}
    for ra, rb in zip(a, b):
        g = groups.setdefault((ra["kv_dtype"], "unsplit" if ra["splits"] == 1 else "split"),
                              dict(calls=0, valid_differ=0, padding_differ=0, with_padding=0, a_zero=0, b_zero=0))
        g["calls"] += 1
        g["valid_differ"] += ra["valid"] != rb["valid"]
        g["padding_differ"] += ra["padding"] != rb["padding"]
        g["with_padding"] += ra["padding_rows"] > 0
        g["a_zero"] += ra["padding_zero"]
        g["b_zero"] += rb["padding_zero"]
        if ra["valid"] != rb["valid"]:
            print("valid rows differ:", key(ra))
    for (kv_dtype, route), g in groups.items():
        print(json.dumps({"kv_dtype": kv_dtype, "route": route, **g}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare)
        return
    from mlmicroservicetemplate_amd import ops
    from mlmicroservicetemplate_amd.ops import reference as R

    if not torch.cuda.is_available():
        raise SystemExit("flash_ctx_dump: needs the GPU")
    rows = []
    for Hq, Hkv in ((8, 2), (4, 1), (8, 1)):
        for S in (1, 16, 63, 64, 65, 130):
            dump_case(ops, rows, make_case(R, Hq, Hkv, S, seed=1000 * Hq + 10 * Hkv + S), "tests", (1, 2, 3, 8))
    dump_case(ops, rows, make_case(R, 8, 2, 5, seed=3, pasts=[1000, 37], max_seq=1100, slot_ids=(3, 1)), "deep",
              (4, 16))
    torch.cuda.synchronize()
    write(rows, a.out)
    print(f"{len(rows)} calls, {2 * len(rows)} hashed tensors -> {a.out}", flush=True)


if __name__ == "__main__":
    main()
