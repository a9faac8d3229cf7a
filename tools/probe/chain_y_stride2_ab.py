"""Per-call A/B of the two stride-2 stage boundaries of the bs=32 ResNet-50 forward (layer1.2 ->
layer2.0 and layer2.3 -> layer3.0), in one process on one build: the full y store against the
compact one (``y_stride2=True``: only the pixels (2i, 2j) are written), arms alternating full /
compact / full again (the A/A control), REPS repeats (default 4), graph-timed alone (c1) and with 4
copies co-running (c4) as component_costs.py times them.  MLS_CHAIN_VARIANT picks the kernel form
as in the model (2: the ring form at layer2.3 -> layer3.0).  One JSON line per (boundary, arm,
repeat); MB counts every bf16 tensor the arm reads or writes once, weights excluded."""
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
    model.chain_y_stride2 = False  # record the full-store calls
    model.chain_conv2 = False  # every boundary as ops.conv1x1_chain (the default at these two anyway)
    imgs = torch.randint(0, 256, (32, 224, 224, 3), dtype=torch.uint8, device=dev)
    calls = [c for c in Recorder(model).run(imgs) if c[0] == "conv1x1_chain"
             and (c[2][1].shape[1], c[2][1].shape[0], c[2][3].shape[0]) in ops.CHAIN_Y_STRIDE2_SHAPES]
    for i, (_, fn, a, k) in enumerate(calls):
        a1, w3, w1 = a[0], a[1], a[3]
        M = a1.shape[0] * a1.shape[1] * a1.shape[2]
        N1, N2 = w3.shape[0], w1.shape[0]
        base = a1.numel() * 2 + (M * N1 * 2 if k.get("residual") is not None else 0) + M * N2 * 2
        kk = {x: v for x, v in k.items() if x not in ("y_out", "t1_out", "y_stride2")}

        def full():
            return fn(*a, **kk)

        def compact():
            return fn(*a, y_stride2=True, **kk)

        arms = (("full", full, base + M * N1 * 2), ("compact", compact, base + M * N1 // 2),
                ("full_again", full, base + M * N1 * 2))
        for rep in range(reps):
            for arm, f, nbytes in arms:
                row = {"boundary": i, "K": w3.shape[1], "N1": N1, "N2": N2, "arm": arm, "rep": rep,
                       "MB": round(nbytes / 1e6, 1)}
                for conc in (1, 4):
                    t = autotune._time_multi([f for _ in range(conc)], 20) * 1e3
                    row[f"c{conc}_us"] = round(t, 2)
                    row[f"c{conc}_TBs"] = round(nbytes / t / 1e6, 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
