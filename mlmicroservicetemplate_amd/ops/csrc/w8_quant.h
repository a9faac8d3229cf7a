// The one W8A8 activation-row rule on the device (ops/reference.py a8_quant): scale = max(max|h|, 2^-40) / 448
// with a true division, q = e4m3fn_rne(h * (1 / scale)).  quant_rows_fp8_kernel (gemm_w8a8.hip) and the fused
// prologue of skinny_w8_kernel (skinny_w8.hip) both convert through here, so their codes agree bit for bit.
#pragma once
#include "common.h"

constexpr float W8_FP8_MAX = 448.f;
constexpr float W8_AMAX_FLOOR = 9.094947017729282e-13f;  // 2^-40
constexpr int W8_E8M0_ONE = 0x7F7F7F7F;                  // block scale 2^0 in every byte

MLS_DEV float w8_row_scale(float amax) { return fmaxf(amax, W8_AMAX_FLOOR) / W8_FP8_MAX; }

// eight bf16 values of a row -> their eight e4m3 codes, inv = 1 / w8_row_scale(max|row|)
MLS_DEV int2 w8_codes8(uint4 h, float inv) {
  float f[8];
  unpack8(h, f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * inv, f[5] * inv, 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * inv, f[7] * inv, hi, true);
  return int2{lo, hi};
}
