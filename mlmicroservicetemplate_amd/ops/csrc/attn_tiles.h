// The pieces the attention kernels share (attention.hip, flash_ctx.hip, kv_fp8.hip): the flash tile's
// constants and v2 tile body, and the parts of the matrix-core decode kernel that do not depend on the
// cache's element type.  They take the few values they need, never a kernel's argument struct;
// MLS_CHECKs stay in the kernels, so each translation unit reports its own codes.
//
// Flash2Tile and DecodeMerge are closures written out -- a struct of references with a call operator,
// in an unnamed namespace, not force-inlined: what a local lambda of the kernel is to the compiler.
// That form compiles flash_ctx_kernel<FP8, SPLIT> and flash_fwd2_kernel to the instruction stream they had with the
// tile body as a local lambda; as a force-inlined function of the same text it took 4-8 VGPRs more and
// measured 0.6-0.8 % slower at long contexts (docs/PERF_NOTES.md).  For the same reason the kernels
// keep their own staging loop and epilogue: through helpers of either form their instruction stream moved
// (flash_ctx_kernel's four instantiations share theirs as one text with `if constexpr` in place).
#pragma once
#include "common.h"

typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define LDS_AS __attribute__((address_space(3)))

MLS_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// ------------------------------------------------------------------------------- flash tile
// 64-key K / V tiles in LDS: K rows with their 16-B chunks XOR-swizzled (chunk ^ row & (CPR-1)):
// conflict-free ds_read_b128; V rows padded by 32 B: conflict-free transposed reads.
template <int D>
struct FlashTile {
  static constexpr int BKV = 64;
  static constexpr int CPR = D / 8;         // 16-B chunks per row
  static constexpr int KK = D / 32;         // k-steps of the S^T MFMA
  static constexpr int DT = D / 16;         // 16-wide d tiles of O
  static constexpr int VST = D * 2 + 32;    // padded V row stride (bytes)
  static constexpr int K_BYTES = BKV * D * 2;
  static constexpr int V_BYTES = BKV * VST;
  static constexpr int OST = D + 8;         // v2 output tile rows (elements), padded by 16 B: the 16
                                            // query rows of one 8-B write land in different banks
  static constexpr int ni(int nt) { return BKV * CPR / nt; }  // a tile's 16-B chunks per thread of nt
};

// The v2 tile body (flash_fwd2_kernel, flash_ctx_kernel<FP8, SPLIT>): the prefill loop with the O accumulator
// transposed and the per-score VALU cut (Llama prefill, D = 128: the v1 loop issued ~450 VALU + ~170
// SALU per wave per 64-key tile against 32 MFMAs -- 193 TFLOP/s at B = 8 x 512,
// profiles/r6_flash_llama_probe.txt).  Same tiling and LDS layouts as flash_fwd_kernel; per tile and wave:
//   * O^T += V^T P^T: the PV MFMA with its operands swapped (the V fragment read by ds_read_tr16 is the
//     A operand's layout as well), so the accumulator holds O[q = lane column][d rows] and the softmax
//     rescale / final 1 / l are lane-local -- no cross-lane shuffles of alpha or 1 / l;
//   * the row sum l stays a per-lane partial over the lane's own keys (combined once, at the end);
//   * scores stay unscaled: the row max is taken raw, one FMA per score forms x * scale - m;
//     -1e30 instead of -inf for the running max removes every "no key yet" select;
//   * the key-range / causal mask runs only on the tiles that need it (`EDGE`, a wave-uniform branch),
//     where 16-key sub-tiles wholly above the diagonal also skip their MFMAs.
// One tile body with wave-uniform branches, 158 VGPRs in flash_fwd2_kernel<128> (150 in
// flash_ctx_kernel on the bf16 cache, 130 on the e4m3 cache): 3 waves per SIMD.
// (Full and edge tiles as two straight-line copies of the body took 196 VGPRs -- 2 waves per SIMD --
// and measured 71-73 vs 62 us at B = 8 x 512: profiles/r6_flash_v2_vs_v1.jsonl.)
//
// Keys kv0 + 16t + 4g + j (accumulator rows) against the query at position pw + fr (lane column);
// pw = the position of the wave's first query, L = the sequence's keys, c = scale * log2(e).
// acc_o[dt][j] = O[q = fr][d = 16dt + 4g + j] (unnormalised), m_run the running max of the scaled
// scores of query fr (log2 units, starts at -1e30), l_run this lane's partial of the row sum.
// ALWAYS_CAUSAL: the mask rule is fixed at compile time (ctx); otherwise `causal` decides per launch.
namespace {
template <int D, bool ALWAYS_CAUSAL>
struct Flash2Tile {
  using T = FlashTile<D>;
  f32x4 (&acc_o)[D / 16];
  float& m_run;
  float& l_run;
  const bf16x8 (&qf)[D / 32];
  char*& Ks;
  char*& Vs;
  const int& causal;
  const int& pw;
  const int& L;
  const float& c;
  const int& g;
  const int& fr;
  __device__ void operator()(int kv0, bool EDGE) const {
    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      // a sub-tile wholly above the wave's diagonal: no MFMAs (masked to -inf below)
      if (EDGE && (ALWAYS_CAUSAL || causal) && kv0 + 16 * t > pw + 15) continue;
      const int row = 16 * t + fr;
#pragma unroll
      for (int kk = 0; kk < T::KK; ++kk) {
        const int ch = 4 * kk + g;
        const bf16x8 kf = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(Ks + row * (D * 2) + ((ch ^ (row & (T::CPR - 1))) * 16)));
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s[t], 0, 0, 0);
      }
    }
    if (EDGE) {
      // last visible key of this query
      const int lim = (ALWAYS_CAUSAL || causal) ? min(L - 1, pw + fr) : L - 1;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (kv0 + 16 * t + 4 * g + j > lim) s[t][j] = -INFINITY;
    }
    float mt = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])),
                     fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
    mt = fmaxf(mt, fmaxf(fmaxf(fmaxf(s[2][0], s[2][1]), fmaxf(s[2][2], s[2][3])),
                         fmaxf(fmaxf(s[3][0], s[3][1]), fmaxf(s[3][2], s[3][3]))));
    mt = fmaxf(mt, xor16_f(mt));
    mt = fmaxf(mt, xor32_f(mt));
    const float m_new = fmaxf(m_run, mt * c);  // -inf * c stays -inf; m_run >= -1e30
    const float alpha = fast_exp2(m_run - m_new);
    m_run = m_new;
    const f32x2 c2 = {c, c}, nm2 = {-m_new, -m_new};
    f32x2 ls2 = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        f32x2 x = {s[t][2 * jj], s[t][2 * jj + 1]};
        x = __builtin_elementwise_fma(x, c2, nm2);
        const f32x2 p = {fast_exp2(x[0]), fast_exp2(x[1])};  // masked: exp2(-inf) = 0
        s[t][2 * jj] = p[0];
        s[t][2 * jj + 1] = p[1];
        ls2 += p;
      }
    l_run = fmaf(l_run, alpha, ls2[0] + ls2[1]);
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt) acc_o[dt] *= alpha;
    // ---- O^T += V^T P^T: two 32-key k-steps, key order permuted identically in both operands ----
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      // both sub-tiles above the diagonal
      if (EDGE && (ALWAYS_CAUSAL || causal) && kv0 + 32 * st > pw + 15) continue;
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf[j] = (bf16)s[2 * st][j];
        pf[4 + j] = (bf16)s[2 * st + 1][j];
      }
      const int qq = fr >> 2, pp = fr & 3;
      const int row0 = 32 * st + 4 * g + qq;
      const int row1 = row0 + 16;
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) {
        const int colb = (16 * dt + 4 * pp) * 2;
        const short4v r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS short4v*)(Vs + row0 * T::VST + colb));
        const short4v r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS short4v*)(Vs + row1 * T::VST + colb));
        const short8v vv = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]};
        acc_o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, acc_o[dt], 0, 0, 0);
      }
    }
  }
};
}  // namespace

// ------------------------------------------------------------------------------- matrix-core decode
// decode_attn_mfma_kernel<G, WAVES> (attention.hip, bf16 cache) and decode_attn_fp8_kernel<G, WAVES>
// (kv_fp8.hip): D = 128, WAVES waves of 32 keys, the G query heads of a KV head on the lane column.
struct DecodeDims {
  static constexpr int D = 128, KK = D / 32, DT = D / 16;
  static constexpr int VST = D * 2 + 32;      // padded V row (bytes): conflict-free transposed reads
};
template <int G, int WAVES>
struct DecodeTile : DecodeDims {
  static constexpr int NT = WAVES * 64, CHUNK = WAVES * 32;
  static constexpr int NPRO = (G + 1) * 16;   // prologue tasks: G query heads + the new K / V row, 16-B chunks
  static constexpr int PIT = (NPRO + NT - 1) / NT;
};

// a split with no key: the sequence's first split zeroes the output row of an empty sequence
template <int G, int NT>
MLS_DEV bool decode_split_empty(int start, int L, int sp, bf16* o, int o_stride, int b, int hk, int tid) {
  if (start < L) return false;
  if (L <= 0 && sp == 0)
    for (int idx = tid; idx < G * DecodeDims::D; idx += NT)
      o[(long)b * o_stride + (long)hk * G * DecodeDims::D + idx] = (bf16)0.f;
  return true;
}

// The prologue's small operands, task t = tid + it NT -> (row r = t / 16, chunk c = t % 16): chunk c of
// query head r < G, or (rope mode, r == G) of the new token's K with its V chunk in pv; in rope mode
// also the rotate-half partner chunk and the position's cos / sin for the chunk's 8 dims.  Loaded
// before the cache rows, so their vmcnt waits leave the rows in flight.
template <int G, int WAVES, int PIT>
MLS_DEV void decode_pro_load(uint4 (&px)[PIT], uint4 (&pxp)[PIT], uint4 (&pv)[PIT], float4 (&pcs)[PIT][4],
                             const bf16* qrow, bool rope, const float* cos_t, const float* sin_t, int pos, int hk,
                             int Hq, int Hkv, int tid) {
  using T = DecodeTile<G, WAVES>;
  static_assert(PIT == T::PIT, "one slot per prologue pass");
  constexpr int D = T::D;
#pragma unroll
  for (int it = 0; it < T::PIT; ++it) {
    const int t = tid + it * T::NT, r = t >> 4, c = t & 15;
    px[it] = pxp[it] = pv[it] = make_uint4(0, 0, 0, 0);
    pcs[it][0] = pcs[it][1] = pcs[it][2] = pcs[it][3] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < T::NPRO && (r < G || rope)) {
      const bf16* src = qrow + (long)(r < G ? hk * G + r : Hq + hk) * D;
      px[it] = ld16(src + c * 8);
      if (rope) {
        pxp[it] = ld16(src + ((c + 8) & 15) * 8);
        const float* cp = cos_t + (long)pos * (D / 2) + (c & 7) * 8;
        const float* sq = sin_t + (long)pos * (D / 2) + (c & 7) * 8;
        pcs[it][0] = *reinterpret_cast<const float4*>(cp);
        pcs[it][1] = *reinterpret_cast<const float4*>(cp + 4);
        pcs[it][2] = *reinterpret_cast<const float4*>(sq);
        pcs[it][3] = *reinterpret_cast<const float4*>(sq + 4);
        if (r == G) pv[it] = ld16(qrow + (long)(Hq + Hkv + hk) * D + c * 8);
      }
    }
  }
}

// O = P . V over the wave's 32 keys: pf = P packed from the S^T accumulators (heads on rows), V the
// wave's padded row-major bf16 image, keys in the same permuted order.  O rows = heads 4g + j,
// columns d = 16 dt + fr.
MLS_DEV void decode_pv(f32x4 (&o)[DecodeDims::DT], bf16x8 pf, const char* V, int g, int fr) {
  using T = DecodeDims;
  const int row0 = 4 * g + (fr >> 2), row1 = row0 + 16;
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt) {
    const int colb = (16 * dt + 4 * (fr & 3)) * 2;
    const short4v r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS short4v*)(V + row0 * T::VST + colb));
    const short4v r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS short4v*)(V + row1 * T::VST + colb));
    const short8v vv = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]};
    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, __builtin_bit_cast(bf16x8, vv), f32x4{0.f, 0.f, 0.f, 0.f}, 0,
                                                    0, 0);
  }
}

// Merge the block's waves through LDS once each has stored (mt, ls) of column fr in sm_m / sm_l and its O
// rows (columns 4g + j) in sm_o -- that store stays in the kernels: through this struct one instantiation
// paired its ds_write_b32 differently.  A sequence that fits one split (`direct`) gets its output row,
// otherwise split sp's fp32 partial (m, l, O) goes to ws / ws_ml for the combine kernels or the fused
// combine of mls_skinny_packed_combine.
// C = G (the single-token kernels): column = query head hh of the KV head, one output row per sequence.
// C > G (decode_verify_kernel): nq queries per sequence, column = query * G + head; output / partial row
// b * nq + query, so the partials of a sequence are those of nq * Hq heads of one row.
namespace {
template <int G, int WAVES, int C = G>
struct DecodeMerge {
  using T = DecodeTile<G, WAVES>;
  static constexpr int D = T::D;
  float (&sm_m)[WAVES][C];
  float (&sm_l)[WAVES][C];
  float (&sm_o)[WAVES][C][D];
  bf16* const& out;
  float* const& ws;
  float* const& ws_ml;
  const int& o_stride;
  const int& Hq;
  const int& nsplit;
  const int& b;
  const int& hk;
  const int& sp;
  const int& tid;
  __device__ void operator()(bool direct, int nq = 1) const {
    __syncthreads();
    const int cols = C == G ? G : nq * G;
    for (int idx = tid; idx < cols * D; idx += T::NT) {
      const int cc = idx / D, d = idx % D;
      const int hh = C == G ? cc : cc % G;
      const long row = C == G ? (long)b : (long)b * nq + cc / G;
      float M = -INFINITY;
#pragma unroll
      for (int p = 0; p < WAVES; ++p) M = fmaxf(M, sm_m[p][cc]);
      float Ls = 0.f, O = 0.f;
      if (M != -INFINITY) {
#pragma unroll
        for (int p = 0; p < WAVES; ++p) {
          const float w = __builtin_amdgcn_exp2f(sm_m[p][cc] - M);
          Ls += sm_l[p][cc] * w;
          O += sm_o[p][cc][d] * w;
        }
      }
      if (direct) {
        out[row * o_stride + (long)(hk * G + hh) * D + d] = (bf16)(Ls > 0.f ? O / Ls : 0.f);
      } else {
        const long base = (row * Hq + hk * G + hh) * nsplit + sp;
        ws[base * D + d] = O;
        if (d == 0) {
          ws_ml[base * 2] = M;
          ws_ml[base * 2 + 1] = Ls;
        }
      }
    }
  }
};
}  // namespace
