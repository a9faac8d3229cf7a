// Shared device helpers for the MI355X (gfx950 / CDNA4) kernels of mlmicroservicetemplate_amd.
// Wave64 everywhere; bf16 storage, fp32 accumulate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_sched.h"

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define MLS_DEV __device__ __forceinline__

// error codes returned by every launcher (0 = launched)
enum MlsStatus : int {
  MLS_OK = 0,
  MLS_BAD_ARG = 1001,
  MLS_UNSUPPORTED = 1002,
};

MLS_DEV float bf2f(bf16 x) { return (float)x; }
MLS_DEV bf16 f2bf(float x) { return (bf16)x; }

// ---- bounds-checked debug builds: `MLS_DEBUG=1` loads a variant compiled with
// -DMLS_DEBUG in which MLS_CHECK records the first violated data-dependent bound (code, block,
// thread) in a per-translation-unit device word instead of letting the access fault the GPU;
// the kernels keep their guards in release builds too, MLS_CHECK only adds the report.  The host
// reads / clears the words through mls_debug_read_<tu> after synchronising (ops._lib.check).
#ifdef MLS_DEBUG
static __device__ int g_mls_dbg[4];
#define MLS_CHECK(cond, code)                                              \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (atomicCAS(&g_mls_dbg[0], 0, (code)) == 0) {                      \
        g_mls_dbg[1] = (int)blockIdx.x;                                    \
        g_mls_dbg[2] = (int)blockIdx.y;                                    \
        g_mls_dbg[3] = (int)threadIdx.x;                                   \
      }                                                                    \
    }                                                                      \
  } while (0)
#define MLS_DEBUG_EXPORT(tu)                                               \
  extern "C" int mls_debug_read_##tu(int* out) {                           \
    int zero[4] = {0, 0, 0, 0};                                            \
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mls_dbg), 16);    \
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_mls_dbg), zero, 16); \
    return (int)e;                                                         \
  }
#else
#define MLS_CHECK(cond, code) ((void)0)
#define MLS_DEBUG_EXPORT(tu)
#endif

// ---- buffer (SRD) loads: hardware range check returns 0 for an out-of-range offset, which is
// how the implicit-GEMM gather zero-fills conv padding without branches or pointer selects.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr int OOB = (int)0x80000000;  // any offset >= num_records reads as zero
MLS_DEV rsrc_t make_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
MLS_DEV uint4 bload16(rsrc_t r, int byte_off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
MLS_DEV uint2 bload8(rsrc_t r, int byte_off) {
  return __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0));
}
// write-through (sc1) 4-byte store / L1-bypassing (sc1) load: an in-launch hand-off between
// workgroups with no release fence (whose L2 write-back serialises per XCD) and no acquire --
// cdna_hip_programming.md §6 Guideline 16, R1
MLS_DEV void bstore_f32_sc1(rsrc_t r, int byte_off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, byte_off, 0, 16);
}
MLS_DEV float bload_f32_sc1(rsrc_t r, int byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 16));
}
MLS_DEV uint32_t clamp_bytes(size_t n) { return n > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)n; }

MLS_DEV uint4 ld16(const void* p) { return *reinterpret_cast<const uint4*>(p); }
MLS_DEV void st16(void* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }

MLS_DEV void unpack8(uint4 v, float (&f)[8]) {
  bf16x8 b = __builtin_bit_cast(bf16x8, v);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = (float)b[i];
}
MLS_DEV uint4 pack8(const float (&f)[8]) {
  bf16x8 b;
#pragma unroll
  for (int i = 0; i < 8; ++i) b[i] = (bf16)f[i];
  return __builtin_bit_cast(uint4, b);
}

// ---- cross-lane exchange on the VALU (DPP / v_permlane*_swap), not the LDS pipe ----
// __shfl_xor compiles to ds_bpermute_b32: an LDS round trip (~100+ cycles) per step, which makes a
// dependent reduction chain latency-bound.  These stay on the VALU.
template <int CTRL>
MLS_DEV float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// value held by lane (lane ^ 16) / (lane ^ 32)
MLS_DEV float xor16_f(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __builtin_bit_cast(float, ((threadIdx.x >> 4) & 1) ? r[0] : r[1]);
}
MLS_DEV float xor32_f(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, ((threadIdx.x >> 5) & 1) ? r[0] : r[1]);
}
// value held by lane (lane ^ 8) (rotate by 8 inside a 16-lane row)
MLS_DEV float xor8_f(float v) { return dpp_f<0x128>(v); }
// sum over aligned groups of N lanes (N = 4, 8, 16), every lane gets its group's sum
template <int N>
MLS_DEV float group_sum(float v) {
  static_assert(N == 4 || N == 8 || N == 16, "group");
  v += dpp_f<0xB1>(v);                      // quad_perm [1,0,3,2]: lane ^ 1
  v += dpp_f<0x4E>(v);                      // quad_perm [2,3,0,1]: lane ^ 2
  if constexpr (N >= 8) v += dpp_f<0x141>(v);   // row_half_mirror: the other quad of the 8
  if constexpr (N >= 16) v += dpp_f<0x140>(v);  // row_mirror: the other half of the 16
  return v;
}

// ---- wave64 reductions ----
MLS_DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
MLS_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// block-wide sum for blockDim.x <= 1024 (multiple of 64); `red` needs >= 16 floats of LDS.
MLS_DEV float block_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  float t = lane < nw ? red[lane] : 0.f;
  return wave_sum(t);
}
MLS_DEV float block_max(float v, float* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_max(v);
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  float t = lane < nw ? red[lane] : -INFINITY;
  return wave_max(t);
}

// Bijective XCD-aware remap (cdna_hip_programming.md §5 "XCD swizzle must be bijective"):
// blocks b, b+8, b+16 ... share an XCD; give each XCD a contiguous range of logical tiles so
// neighbouring tiles (which share operand panels) hit the same L2.
// (the arithmetic lives in chain_sched.h, which also compiles for the host and is checked there)
MLS_DEV int xcd_remap(int bid, int nwg) { return chain_logical_block(bid, nwg); }

// CUs of the current device, for the grids of the persistent kernels (256 if the query fails)
static inline int mls_num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

MLS_DEV float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
MLS_DEV float silu(float x) { return x / (1.f + __expf(-x)); }
// GEMM-epilogue forms: no IEEE divide sequence, no ocml erff branches.  erf by Abramowitz & Stegun
// 7.1.26 (|error| <= 1.5e-7, far below the bf16 output's half-ulp), one v_rcp + one v_exp each.
MLS_DEV float erf_fast(float x) {
  const float a = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, a, 1.f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float y = fmaf(-p * t, __expf(-a * a), 1.f);
  return copysignf(y, x);
}
// GEMM-epilogue GELU: the tanh form as x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3), in 7
// instructions (one v_exp, one v_rcp) -- half the issue cost of 0.5 x (1 + erf_fast(x / sqrt 2)),
// which made the FFN-up epilogue VALU-bound (12k vs 5.5k cycles per 256 x 256 tile).  It differs from
// the erf form by <= 4.7e-4 (at x = 2.70, where a bf16 ulp is 7.8e-3).
// Built with -DMLS_GELU_ERF (MLS_GELU_ERF=1 at ops.build time) every epilogue computes the exact erf
// form instead (the reference BERT's GELU; tests/test_gelu_epilogue_gpu.py bounds the difference).
MLS_DEV float gelu_fast(float x) {
#ifdef MLS_GELU_ERF
  return 0.5f * x * (1.f + erf_fast(x * 0.70710678118654752f));
#else
  constexpr float k0 = -2.f * 0.7978845608028654f * 1.4426950408889634f;  // -2 sqrt(2/pi) log2(e)
  constexpr float k1 = k0 * 0.044715f;
  const float z = fmaf(x * x, k1, k0) * x;  // -2u log2(e)
  return x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(z));
#endif
}
MLS_DEV float silu_fast(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_TANH = 3, ACT_SILU = 4, ACT_SILU_MUL = 5 };
MLS_DEV float apply_act(float v, int act) {
  switch (act) {
    case ACT_RELU: return fmaxf(v, 0.f);
    case ACT_GELU: return gelu_erf(v);
    case ACT_TANH: return tanhf(v);
    case ACT_SILU: return silu(v);
    default: return v;
  }
}
MLS_DEV float apply_act_fast(float v, int act) {
  switch (act) {
    case ACT_RELU: return fmaxf(v, 0.f);
    case ACT_GELU: return gelu_fast(v);
    case ACT_TANH: return tanhf(v);
    case ACT_SILU: return silu_fast(v);
    default: return v;
  }
}
