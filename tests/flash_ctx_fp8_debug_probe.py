"""Run by test_flash_ctx_fp8_gpu.py in a child process with MLS_DEBUG=1 HIP_LAUNCH_BLOCKING=1: legal
ops.flash_attention_ctx_fp8 calls pass the bounds checks of the debug build, unsplit and split; a page id
outside the pool, lens past a slot's rows and a slot outside the cache are reported (the kernel's own
guards keep every access in bounds: a tile whose page id is bad gets descriptors of zero valid bytes)."""
import sys

import torch

from mlmicroservicetemplate_amd import ops
from mlmicroservicetemplate_amd.ops import _lib
from mlmicroservicetemplate_amd.ops import reference as R

assert _lib.DEBUG and "debug" in ops.lib()._name, ops.lib()._name
dev = "cuda:0"
Hq, Hkv, D, B, S = 4, 1, 128, 2, 16
qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=dev).to(torch.bfloat16)
kp, ksp = R.kv_quant_fp8(torch.randn(5, Hkv, 64, D, device=dev).to(torch.bfloat16))
vp, vsp = R.kv_quant_fp8(torch.randn(5, Hkv, 64, D, device=dev).to(torch.bfloat16))
table = torch.tensor([[1, 2], [3, 4]], device=dev, dtype=torch.int32)


def i32(*v):
    return torch.tensor(v, device=dev, dtype=torch.int32)


def call(past, lens, slot_ids=None, tab=table, **kw):
    return ops.flash_attention_ctx_fp8(qkv, kp, vp, ksp, vsp, past, lens, B, S, Hq, Hkv, D, slot_ids=slot_ids,
                                       page_table=tab, **kw)


split = dict(splits=2, max_ctx=128)
# legal
assert torch.isfinite(call(i32(60, 0), i32(70, 16)).float()).all()
assert torch.isfinite(call(i32(60, 0), i32(70, 16), **split).float()).all()
bad_table = i32(1, 10 ** 6, 3, 4).view(2, 2)
caught = []
for code, fn in (("313", lambda: call(i32(60, 0), i32(70, 16), tab=bad_table)),       # page id outside the pool
                 ("313", lambda: call(i32(60, 0), i32(70, 16), tab=bad_table, **split)),
                 ("311", lambda: call(i32(60, 0), i32(1000, 16))),                     # lens past the slot's pages
                 ("312", lambda: call(i32(0, 0), i32(16, 7), i32(0, 99)))):            # slot outside the table
    try:
        fn()
    except _lib.NativeError as e:
        assert f"[{code}]" in str(e), (code, str(e))
        caught.append(code)
print(caught)
assert caught == ["313", "313", "311", "312"], caught
# and the check state is clean afterwards
call(i32(60, 0), i32(70, 16))
print("FLASH-CTX-FP8-DEBUG-OK")
sys.exit(0)
