"""Per-call A/B of the chain calls of the bs=32 ResNet-50 forward, in one process on one build:
variant 1 (conv_chain_kernel everywhere -- the kernel every boundary ran before the ring kernel
existed) against variant 2 (conv_chain_ring_kernel wherever it is instantiated), arms alternating,
REPS repeats (default 4), graph-timed alone (c1) and with 4 copies co-running (c4) as
component_costs.py times them.  One JSON line per (call, variant, repeat); TB/s counts every bf16
tensor of the call read or written once, weights excluded."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from component_costs import Recorder  # noqa: E402

from mlmicroservicetemplate_amd import ops  # noqa: E402
from mlmicroservicetemplate_amd.models import resnet  # noqa: E402
from mlmicroservicetemplate_amd.ops import autotune  # noqa: E402


def main():
    reps = int(os.environ.get("REPS", "4"))
    dev = torch.device("cuda:0")
    model = resnet.ResNet50Fused(resnet.init_resnet50(0), dev, max_batch=32,
                                 tuning=autotune.load_tuning("resnet50", 32))
    imgs = torch.randint(0, 256, (32, 224, 224, 3), dtype=torch.uint8, device=dev)
    calls = [c for c in Recorder(model).run(imgs) if c[0] == "conv1x1_chain"]
    lib = ops.lib()
    for i, (_, fn, a, k) in enumerate(calls):
        a1, w3, w1 = a[0], a[1], a[3]
        M = a1.shape[0] * a1.shape[1] * a1.shape[2]
        N1, N2 = w3.shape[0], w1.shape[0]
        a2 = k.get("a2")
        nbytes = a1.numel() * 2 + (M * a2.shape[3] * 2 if a2 is not None else 0) \
            + (M * N1 * 2 if k.get("residual") is not None else 0) + M * N1 * 2 + M * N2 * 2
        kk = {x: v for x, v in k.items() if x not in ("y_out", "t1_out")}
        for rep in range(reps):
            for variant in (1, 2):
                row = {"call": i, "K": w3.shape[1], "N1": N1, "N2": N2, "variant": variant, "rep": rep,
                       "MB": round(nbytes / 1e6, 1)}
                try:
                    lib.mls_chain_set_variant(variant)
                    for conc in (1, 4):
                        t = autotune._time_multi([(lambda: fn(*a, **kk)) for _ in range(conc)], 20) * 1e3
                        row[f"c{conc}_us"] = round(t, 2)
                        row[f"c{conc}_TBs"] = round(nbytes / t / 1e6, 2)
                finally:
                    lib.mls_chain_set_variant(0)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
