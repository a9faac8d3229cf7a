"""Perplexity of a token file under a MODEL_CONFIG: the quality A/B of the numerics-changing options.

    python tools/score.py --model-config '{"weight_dtype": "int4"}' --ids tokens.npy [--weights f] [--window 512]

``tokens.npy``: one 1-D integer array of token ids.  It is cut into windows of ``--window`` tokens (the last one
shorter), each scored from its own start by ``LlamaTP.score`` -- so a window's first token is not scored and the
perplexity is that of ``tokens`` scored positions -- ``--batch`` windows per forward.  Prints one JSON line:
``{"tokens", "nll", "perplexity", ...}``.  Without ``--weights`` the model is the seeded random init
(``"config": "tiny"`` or the 8B shape): a smoke run, not a quality number.  Run it once per MODEL_CONFIG and compare.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_model(extra: dict, weights: str, window: int, batch: int, backend: str, device: str, seed: int = 0):
    from mlmicroservicetemplate_amd.models import llama
    from mlmicroservicetemplate_amd.plugins.llm import LlamaPlugin as P

    wd = P.parse_weight_dtype(extra)
    kv_dtype, kv_prefill = str(extra.get("kv_dtype", "bf16")), str(extra.get("kv_prefill", "rows"))
    cfg = llama.LLAMA3_8B if extra.get("config", "8b") == "8b" else llama.tiny_config(**extra.get("overrides", {}))
    source = llama.CheckpointSource(weights, device=device) if weights else None
    params = llama.init_llama_shard(cfg, 1, 0, seed, device=device, source=source)
    return llama.LlamaTP(params, cfg, backend=backend, device=device, max_batch=batch, max_seq=window,
                         kv_dtype=kv_dtype, weight_dtype=wd, kv_prefill=kv_prefill, w4_rows=P.parse_w4_rows(extra, wd),
                         w8_decode=P.parse_w8_decode(extra, wd),
                         verify_fp8=P.parse_verify_fp8(extra, kv_dtype, kv_prefill))


def score_tokens(model, tokens: np.ndarray, window: int, batch: int):
    """(scored positions, summed negative log-likelihood in nats) of ``tokens`` in windows of ``window``."""
    wins = [tokens[i: i + window] for i in range(0, len(tokens), window)]
    wins = [w for w in wins if len(w) >= 2]
    n, nll = 0, 0.0
    for b0 in range(0, len(wins), batch):
        grp = wins[b0: b0 + batch]
        S = max(len(w) for w in grp)
        ids = torch.zeros(len(grp), S, dtype=torch.int32)
        for i, w in enumerate(grp):
            ids[i, : len(w)] = torch.from_numpy(np.asarray(w, dtype=np.int32))
        lens = torch.tensor([len(w) for w in grp], dtype=torch.int32)
        lp = model.score(ids, lens).double().cpu()
        nll -= float(lp.sum())
        n += int(lens.sum()) - len(grp)
    return n, nll


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model-config", default="{}", help="MODEL_CONFIG as JSON (weight_dtype, kv_dtype, config ...)")
    ap.add_argument("--ids", required=True, help=".npy file: 1-D integer token ids")
    ap.add_argument("--weights", default="", help="checkpoint (safetensors directory / file); default: seeded init")
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--backend", default="fused", choices=("fused", "reference"))
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args(argv)
    extra = json.loads(args.model_config)
    tokens = np.load(args.ids).reshape(-1)
    if len(tokens) < 2 or args.window < 2:
        raise SystemExit("need at least two tokens and a window of at least two")
    backend = args.backend if args.device != "cpu" else "reference"
    model = build_model(extra, args.weights, args.window, args.batch, backend, args.device)
    if int(tokens.max()) >= model.cfg.vocab or int(tokens.min()) < 0:
        raise SystemExit(f"token ids outside [0, {model.cfg.vocab})")
    n, nll = score_tokens(model, tokens, args.window, args.batch)
    print(json.dumps({"tokens": n, "nll": nll, "perplexity": math.exp(nll / max(n, 1)), "window": args.window,
                      "backend": backend, "model_config": extra, "weights": args.weights or None}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
