"""Per-call A/B of the three layer1 boundaries of the bs=32 ResNet-50 forward, in one process on one
build: the two launches (conv2 as the tuning table runs it, then ops.conv1x1_chain on its output)
against the one fused launch (ops.conv3x3_chain), arms alternating, REPS repeats (default 4),
graph-timed alone (c1) and with 4 copies co-running (c4) as component_costs.py times them.  Each
repeat runs the two-launch arm twice ("two", "two_again"): an A/A control for the order bias the c4
column carries.  One JSON line per (boundary, arm, repeat); MB counts every bf16 tensor the arm
reads or writes once, weights excluded (the two-launch arm's includes t2 written and read back)."""
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
    model.chain_conv2 = False  # record the two launches
    imgs = torch.randint(0, 256, (32, 224, 224, 3), dtype=torch.uint8, device=dev)
    calls = Recorder(model).run(imgs)
    pairs = [(calls[i - 1], c) for i, c in enumerate(calls)
             if c[0] == "conv1x1_chain" and calls[i - 1][0] == "conv2d_nhwc" and calls[i - 1][3].get("kernel") == 3]
    for i, ((_, conv, ca, ck), (_, chain, a, k)) in enumerate(pairs[:3]):
        t1, w2, b2 = ca[0], ca[1], ca[2]
        t2, w3, b3, w1, b1 = a
        M = t2.shape[0] * t2.shape[1] * t2.shape[2]
        N1, N2 = w3.shape[0], w1.shape[0]
        a2 = k.get("a2")
        base = t1.numel() * 2 + (a2.numel() * 2 if a2 is not None else 0) \
            + (M * N1 * 2 if k.get("residual") is not None else 0) + M * N1 * 2 + M * N2 * 2
        kk = {x: v for x, v in k.items() if x not in ("y_out", "t1_out")}
        ckk = {x: v for x, v in ck.items() if x != "out"}

        def two():
            return chain(conv(*ca, **ckk), w3, b3, w1, b1, **kk)

        def fused():
            return ops.conv3x3_chain(t1, w2, b2, w3, b3, w1, b1, **kk)

        arms = (("two", two, base + 2 * t2.numel() * 2), ("fused", fused, base), ("two_again", two, base + 2 * t2.numel() * 2))
        for rep in range(reps):
            for arm, fn, nbytes in arms:
                row = {"boundary": i, "K": w3.shape[1], "N1": N1, "N2": N2, "arm": arm, "rep": rep,
                       "MB": round(nbytes / 1e6, 1)}
                for conc in (1, 4):
                    t = autotune._time_multi([fn for _ in range(conc)], 20) * 1e3
                    row[f"c{conc}_us"] = round(t, 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
