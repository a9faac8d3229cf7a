// The pieces the skinny-GEMM kernels share (skinny_gemm.hip, skinny_w4.hip): the fusion modes, the
// epilogue behind the cross-wave reduction, the split-KV merge of the FUSE_COMBINE prologue, and on
// the host the argument rules and the dispatch over the fusion mode.  The k loops (load_trip, the
// register double buffer, the MFMA bodies) stay in the kernels: they are the measured part of each and
// they do differ.  So does the LDS staging of A: shared as a closure it cost skinny_packed_kernel,
// skinny_fp8_kernel and skinny_w4_kernel<ALDS> 0.05-0.1 us per launch each (docs/PERF_NOTES.md,
// "csrc/skinny_tiles.h"), and each kernel has its own again.
//
// SkEpi sits in the argument structs where its fields sat before: the kernels' first scalar loads
// fetch what the first weight trip needs, and with the epilogue's fields moved to the front
// skinny_w4_kernel measured 2-4 % slower at 8 and 32 rows.
#pragma once
#include <type_traits>

#include "common.h"
#include "fastdiv.h"

// fusion modes of the A prologue (template parameter, so the unrolled k loop has no runtime
// branches -- a branch there makes hipcc drain vmcnt(0) per k-step, cdna_hip_programming.md item 4c).
// FUSE_COMBINE: skinny_packed_kernel only.
enum { FUSE_NONE = 0, FUSE_NORM = 1, FUSE_ADD_NORM = 2, FUSE_COMBINE = 3 };

MLS_DEV uint4 add_round(uint4 a, uint4 b) {  // bf16 + bf16 -> bf16 (the residual stream's precision)
  float x[8], y[8];
  unpack8(a, x);
  unpack8(b, y);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] += y[e];
  return pack8(x);
}

MLS_DEV float sumsq8(uint4 v) {
  float x[8];
  unpack8(v, x);
  float r = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) r += x[e] * x[e];
  return r;
}

// wave64 sum on the VALU (DPP + permlane swaps): the staging prologue is a latency chain every block
// pays before its first MFMA, and four ds_bpermute reductions there cost more than the weight stream
MLS_DEV float wave_sum_valu(float v) {
  v = group_sum<16>(v);
  v += xor16_f(v);
  return v + xor32_f(v);
}

// NTL: non-temporal cache policy (a weight stream is read exactly once per call)
template <int NTL>
MLS_DEV uint4 bload16_pol(rsrc_t r, int byte_off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, NTL ? 2 : 0));
}

// ------------------------------------------------------------------------------------ epilogue
// what the epilogue reads; every kernel's argument struct holds one (`e`)
struct SkEpi {
  const float* bias;
  const bf16* res;  // [M][N]
  bf16* out;        // [M][ldo]
  int M, N, K, ldo, act;
  float eps;
};

MLS_DEV float epi(float v, int n, const SkEpi& e) { return v + (e.bias ? e.bias[n] : 0.f); }

// one output element from its reduced and scaled sum: the SiLU-mul of an interleaved gate/up tile
// (8 gate + 8 up columns of 16; v = gate column n, up = column n + 8), or bias + residual + activation
MLS_DEV void sk_emit(const SkEpi& e, bool glu, int m, int n, float v, float up) {
  if (glu) {
    e.out[(size_t)m * e.ldo + (n >> 4) * 8 + (n & 7)] = (bf16)(silu(epi(v, n, e)) * epi(up, n + 8, e));
    return;
  }
  float o = epi(v, n, e);
  if (e.res) o += (float)e.res[(size_t)m * e.N + n];
  e.out[(size_t)m * e.ldo + n] = (bf16)apply_act(o, e.act);
}

MLS_DEV float sk_rstd(float ssq, const SkEpi& e) { return rsqrtf(ssq / (float)e.K + e.eps); }
// ... from the waves' partial square sums
template <int NWV, int ROWS>
MLS_DEV float sk_rstd(const float (&ssq_red)[NWV][ROWS], int m, const SkEpi& e) {
  float t2 = 0.f;
#pragma unroll
  for (int w = 0; w < NWV; ++w) t2 += ssq_red[w][m];
  return sk_rstd(t2, e);
}

struct NoColScale {};

// The block's epilogue after the barrier behind red[][][]: sum the waves' partials (w = 0..NWV-1), one
// multiply by the scale, emit.  row_scale(m): rstd (times the activation scale); col_scale(n): the
// weight's per-channel scale, NoColScale{} for none -- the product of the two is formed first.
// ALL_ROWS: walk the ROWS of red[] and skip those past M (a trip count known at compile time), instead of M rows.
template <int NWV, int ROWS, int COLS, bool ALL_ROWS = false, class RowScale, class ColScale = NoColScale>
MLS_DEV void sk_reduce_store(const float (&red)[NWV][ROWS][COLS + 1], const SkEpi& e, int n0, RowScale row_scale,
                             ColScale col_scale = {}) {
  const bool glu = e.act == ACT_SILU_MUL;
  for (int q = threadIdx.x; q < (ALL_ROWS ? ROWS : e.M) * COLS; q += NWV * 64) {
    const int m = q / COLS, c = q % COLS;
    if (ALL_ROWS && m >= e.M) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) v += red[w][m][c];
    const float rs = row_scale(m);
    const int n = n0 + c;
    if constexpr (std::is_same_v<ColScale, NoColScale>) v *= rs;
    else v *= rs * col_scale(n);
    if (glu) {
      if ((c & 15) < 8) {
        float up = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) up += red[w][m][c + 8];
        if constexpr (std::is_same_v<ColScale, NoColScale>) up *= rs;
        else up *= rs * col_scale(n + 8);
        sk_emit(e, true, m, n, v, up);
      }
      continue;
    }
    sk_emit(e, false, m, n, v, 0.f);
  }
}

// ------------------------------------------------------------------------- split-KV merge
// The decode_combine_kernel arithmetic for 8 dims d0..d0+7 of head h of row m: the online merge of the
// split-KV decode attention's ns > 1 partials (o [M][Hq][nsplit][D], (m, l) [M][Hq][nsplit][2]) in
// groups of 4 splits -- each group's (m, l, o) loads are issued together (one memory round trip per
// group, not two per split).  Returns the 8 merged values packed as bf16.
MLS_DEV uint4 splitkv_merge(int m, int h, int d0, int ns, const float* cws, const float* cml, int hq, int nsplit,
                            int hd) {
  const long rec = ((long)m * hq + h) * nsplit;
  float mx = -INFINITY, l = 0.f, o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < ns; s0 += 4) {
    float2 ml[4];
    float4 x0[4], x1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = s0 + j < ns;
      const long r = rec + (in ? s0 + j : 0);
      ml[j] = in ? *reinterpret_cast<const float2*>(cml + r * 2) : make_float2(-INFINITY, 0.f);
      x0[j] = in ? *reinterpret_cast<const float4*>(cws + r * hd + d0) : make_float4(0.f, 0.f, 0.f, 0.f);
      x1[j] = in ? *reinterpret_cast<const float4*>(cws + r * hd + d0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float gm = mx;
#pragma unroll
    for (int j = 0; j < 4; ++j) gm = fmaxf(gm, ml[j].x);
    if (gm == -INFINITY) continue;
    const float al = __builtin_amdgcn_exp2f(mx - gm);
    l *= al;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] *= al;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float w = __builtin_amdgcn_exp2f(ml[j].x - gm);
      l += ml[j].y * w;
      o[0] += x0[j].x * w; o[1] += x0[j].y * w; o[2] += x0[j].z * w; o[3] += x0[j].w * w;
      o[4] += x1[j].x * w; o[5] += x1[j].y * w; o[6] += x1[j].z * w; o[7] += x1[j].w * w;
    }
    mx = gm;
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] *= inv;
  return pack8(o);
}

// ---------------------------------------------------------------------------------- host
// the fused prologue's argument rules: A_out must not alias A / A2, and the residual add (A2, A_out)
// exists only as the norm prologue
inline int sk_check_fuse(const void* A, const void* A2, const void* A_out, int norm) {
  if (A_out && (A_out == A || A_out == A2)) return MLS_BAD_ARG;
  if ((A2 || A_out) && !norm) return MLS_UNSUPPORTED;
  return MLS_OK;
}

inline int sk_fuse_mode(const void* A2, int norm) { return A2 ? FUSE_ADD_NORM : norm ? FUSE_NORM : FUSE_NONE; }

inline SkEpi sk_epi(const float* bias, const void* res, void* out, int M, int N, int K, int act, float eps) {
  return SkEpi{bias, (const bf16*)res, (bf16*)out, M, N, K, act == ACT_SILU_MUL ? N / 2 : N, act, eps};
}

// f(std::integral_constant<int, mode>) for the three modes a launcher selects at run time
template <class F>
void with_fuse(int mode, F f) {
  switch (mode) {
    case FUSE_NONE: f(std::integral_constant<int, FUSE_NONE>{}); break;
    case FUSE_NORM: f(std::integral_constant<int, FUSE_NORM>{}); break;
    default: f(std::integral_constant<int, FUSE_ADD_NORM>{}); break;
  }
}
