"""Run by test_flash_ctx_gpu.py in a child process with MLS_DEBUG=1 HIP_LAUNCH_BLOCKING=1: legal
ops.flash_attention_ctx calls pass the bounds checks of the debug build; lens past a slot's rows, a slot
outside the cache and a page id outside the pool are reported (the kernel's own guards keep every
access in bounds: such a row reads as an empty or clamped context)."""
import sys

import torch

from mlmicroservicetemplate_amd import ops
from mlmicroservicetemplate_amd.ops import _lib

assert _lib.DEBUG and "debug" in ops.lib()._name, ops.lib()._name
dev = "cuda:0"
Hq, Hkv, D, B, S, ROWS = 4, 1, 128, 2, 16, 100
qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
kc = torch.randn(3, Hkv, ROWS, D, device=dev).to(torch.bfloat16)
vc = torch.randn_like(kc)
kp = torch.randn(5, Hkv, 64, D, device=dev).to(torch.bfloat16)
vp = torch.randn_like(kp)
table = torch.tensor([[1, 2], [3, 4]], device=dev, dtype=torch.int32)


def i32(*v):
    return torch.tensor(v, device=dev, dtype=torch.int32)


def call(past, lens, slot_ids=None, paged=False, tab=table):
    if paged:
        return ops.flash_attention_ctx(qkv, kp, vp, past, lens, B, S, Hq, Hkv, D, slot_ids=slot_ids, page_table=tab)
    return ops.flash_attention_ctx(qkv, kc, vc, past, lens, B, S, Hq, Hkv, D, slot_ids=slot_ids)


# legal
assert torch.isfinite(call(i32(84, 0), i32(100, 7), i32(2, 0)).float()).all()
assert torch.isfinite(call(i32(60, 0), i32(70, 16), paged=True).float()).all()
caught = []
for code, fn in (("311", lambda: call(i32(84, 0), i32(10 * ROWS, 7))),          # lens past the slot's rows
                 ("311", lambda: call(i32(9, 0), i32(5, 7))),                    # past > lens
                 ("312", lambda: call(i32(0, 0), i32(16, 7), i32(0, 99))),       # slot outside the cache
                 ("313", lambda: call(i32(60, 0), i32(70, 16), paged=True, tab=i32(1, 10 ** 6, 3, 4).view(2, 2)))):
    try:
        fn()
    except _lib.NativeError as e:
        assert f"[{code}]" in str(e), (code, str(e))
        caught.append(code)
print(caught)
assert caught == ["311", "311", "312", "313"], caught
# and the check state is clean afterwards
call(i32(84, 0), i32(100, 7), i32(2, 0))
print("FLASH-CTX-DEBUG-OK")
sys.exit(0)
