// W4A16 skinny GEMM for decode (M <= 32): out[M][N] = act([RMSNorm](A [+ A2]) W^T + b [+ res]) with W held
// as 4-bit codes q + 8 and one bf16 scale per (row, 128 k) -- ops.pack_skinny_w4.  Activations stay
// bf16; only the MFMA B operand is expanded from nibbles, in registers.  Same shape as the packed
// bf16 kernels of skinny_gemm.hip: a block owns NT 16-column tiles, each wave streams a contiguous run
// of 1 KiB granules ([tile][K/128][g][nr][kstep 0..3] 32-bit words: one non-temporal 16-B buffer load per
// lane = that lane's B fragments of four consecutive 32-wide k-steps = one scale group), register
// double-buffered, partial sums reduced through LDS.  A is staged once in LDS (M <= 4, M K 2 <= 64 KiB)
// or rides beside the granules in registers.
//
// Expansion: ((word >> 4p) & 0x000F000F) | 0x43004300 is the bf16 pair (128 + nib, 128 + nib') --
// 0x4300 is 128.0 and a bf16 step there is 1 -- i.e. dword p of the B operand holding 136 + q for
// the weights k = 2p, 2p + 1 (the nibble order of pack_skinny_w4): 2 VALU ops per 2 weights.  The
// MFMA sums a (136 + q) over the granule's four k-steps on top of one more MFMA chain against the
// constant -136 (products of bf16 are exact in fp32, so the offset cancels to fp32 rounding of
// 136 |a|: ~2^-18 of a product), and the group's scale, lane-local because the accumulator column is
// nr, folds it in: acc += s[n] * acc_group.  The loop body is branch-free (cdna_hip_programming.md
// item 4c: a runtime branch there drains vmcnt).
#include "skinny_tiles.h"

namespace {

struct W4Args {
  const bf16* a;   // [M][K]
  const bf16* a2;  // optional [M][K] added to a (residual-stream update)
  bf16* a_out;     // optional [M][K] <- a + a2 (written by the block of column tile 0)
  const uint8_t* w;  // packed nibbles, N K / 2 bytes
  const bf16* sc;    // [N/16][K/128][16]
  SkEpi e;           // bias, res, out, M, N, K, ldo, act, eps
  uint32_t a_bytes, w_bytes, s_bytes;
  FastDiv fd_kch;  // K / 8 chunks per row (LDS staging)
};

MLS_DEV uint32_t bload2(rsrc_t r, int byte_off) { return __builtin_amdgcn_raw_buffer_load_b16(r, byte_off, 0, 0); }

// one k-step's word -> the B fragment 136 + q (k order)
MLS_DEV bf16x8 w4_expand(uint32_t w) {
  constexpr uint32_t m = 0x000F000Fu, b = 0x43004300u;
  return __builtin_bit_cast(bf16x8, make_uint4((w & m) | b, ((w >> 4) & m) | b, ((w >> 8) & m) | b, ((w >> 12) & m) | b));
}

// the other expansion (variants 11, 12; measured slower, docs/PERF_NOTES.md "W4A16 decode"):
// (0x4300 | nib) << 16 is the fp32 128 + nib, one FMA with the group's scale gives (nib - 8) s exactly,
// rounded in pairs to bf16 -- ~3.5 VALU ops per weight, no offset MFMAs and no fold
MLS_DEV bf16x8 w4_expand_scaled(uint32_t w, float sc, float off) {
  bf16x8 b;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t t = w >> (4 * p);
    b[2 * p] = (bf16)fmaf(__builtin_bit_cast(float, ((t & 0xFu) << 16) | 0x43000000u), sc, off);
    b[2 * p + 1] = (bf16)fmaf(__builtin_bit_cast(float, (t & 0x000F0000u) | 0x43000000u), sc, off);
  }
  return b;
}

template <int TMS, int NT, int UN, int NWV, int FUSE, bool ALDS, bool SCALED = false>
__global__ __launch_bounds__(NWV * 64) void skinny_w4_kernel(const W4Args s) {
  static_assert(!ALDS || TMS == 1, "LDS staging holds <= 4 rows");
  extern __shared__ __attribute__((aligned(16))) uint4 a_lds[];  // ALDS: [M][K/8]
  __shared__ float red[NWV][16 * TMS][NT * 16 + 1];
  __shared__ float ssq_red[NWV][16 * TMS];
  constexpr int T = NWV * 64;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nr = lane & 15, g = lane >> 4;
  const int tile0 = blockIdx.x * NT, n0 = tile0 * 16;
  const int G = s.e.K >> 7;  // granules (= scale groups) per tile
  const int kch = s.e.K >> 3;
  const int gpw = (G + NWV - 1) / NWV;
  const int gb = wid * gpw, ge = min(G, gb + gpw);
  const rsrc_t wr = make_rsrc(s.w, s.w_bytes);
  const rsrc_t sr = make_rsrc(s.sc, s.s_bytes);
  const rsrc_t ar = make_rsrc(s.a, s.a_bytes);
  const rsrc_t a2r = make_rsrc(s.a2, FUSE == FUSE_ADD_NORM ? s.a_bytes : 0);
  const int wbase = tile0 * G * 1024 + lane * 16;  // tile j, granule q: + (j G + q) 1024
  const int sbase = (tile0 * G * 16 + nr) * 2;     //                    + (j G + q) 32
  int abase[TMS];
#pragma unroll
  for (int t = 0; t < TMS; ++t) abase[t] = 16 * t + nr < s.e.M ? ((16 * t + nr) * s.e.K + 8 * g) * 2 : OOB;
  const bool wr_res = FUSE == FUSE_ADD_NORM && s.a_out && blockIdx.x == 0;

  constexpr int AU = ALDS ? 1 : UN, AK = ALDS ? 1 : 4;  // register A fragments: none with LDS staging
  struct Trip {
    uint4 w[UN][NT];
    uint32_t sc[UN][NT];
    uint4 a[AU][AK][TMS], a2[AU][AK][TMS];
  };
  auto load_trip = [&](int q0, Trip& tr) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const bool in = q0 + u < ge;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        tr.w[u][j] = bload16_pol<1>(wr, in ? wbase + (j * G + q0 + u) * 1024 : OOB);
        tr.sc[u][j] = bload2(sr, in ? sbase + (j * G + q0 + u) * 32 : OOB);
      }
      if constexpr (!ALDS) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int t = 0; t < TMS; ++t) {
            const int ao = (in && abase[t] != OOB) ? abase[t] + ((q0 + u) * 4 + ks) * 64 : OOB;
            tr.a[u][ks][t] = bload16(ar, ao);
            if constexpr (FUSE == FUSE_ADD_NORM) tr.a2[u][ks][t] = bload16(a2r, ao);
          }
      }
    }
  };

  Trip nxt;
  // register path: the rows' square sums ride on the matrix core -- the A fragment is laid out as a B
  // fragment too (row / column nr, k 8g..8g+7), so mfma(a, a) accumulates A A^T, whose diagonal is the
  // sum of squares (bf16 products are exact in fp32); 8 unpacks + 8 FMAs per k-step leave the VALU
  f32x4 aat[TMS];
#pragma unroll
  for (int t = 0; t < TMS; ++t) aat[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  if constexpr (ALDS) {
    // As skinny_packed_kernel: the first QPT A (+ A2) chunks per thread are loaded BEFORE the first
    // weight trip (the vector memory counter retires in order, so consuming them does not wait for
    // the weights) and the barrier below is LDS-only.
    constexpr int QPT = 2048 / T;
    const int nq = s.e.M * kch;
    uint4 a0[QPT], a20[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
      const int q = tid + j * T;
      const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
      const int off = q < nq ? (m * s.e.K + c * 8) * 2 : OOB;
      a0[j] = bload16(ar, off);
      if constexpr (FUSE == FUSE_ADD_NORM) a20[j] = bload16(a2r, off);
    }
    load_trip(gb, nxt);  // in flight during the staging
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    auto stage = [&](int q, uint4 v, uint4 v2) {
      const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
      if constexpr (FUSE == FUSE_ADD_NORM) {
        v = add_round(v, v2);
        if (wr_res) st16(s.a_out + (size_t)m * s.e.K + c * 8, v);
      }
      a_lds[q] = v;
      if constexpr (FUSE != FUSE_NONE) {
        const float sq = sumsq8(v);
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) part[mm] += mm == m ? sq : 0.f;
      }
    };
#pragma unroll
    for (int j = 0; j < QPT; ++j)
      if (tid + j * T < nq) stage(tid + j * T, a0[j], a20[j]);
    for (int q = tid + QPT * T; q < nq; q += T) {
      const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
      stage(q, ld16(s.a + (size_t)m * s.e.K + c * 8),
            FUSE == FUSE_ADD_NORM ? ld16(s.a2 + (size_t)m * s.e.K + c * 8) : make_uint4(0, 0, 0, 0));
    }
    if constexpr (FUSE != FUSE_NONE) {
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) {
        const float t = wave_sum_valu(part[mm]);
        if (lane == 0) ssq_red[wid][mm] = t;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  } else {
    load_trip(gb, nxt);
  }

  f32x4 acc[TMS][NT];
#pragma unroll
  for (int t = 0; t < TMS; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 neg136 = __builtin_bit_cast(bf16x8, make_uint4(0xC308C308u, 0xC308C308u, 0xC308C308u, 0xC308C308u));
  const bool arow = nr < s.e.M;

  for (int q = gb; q < ge; q += UN) {
    Trip cur = nxt;
    if (q + UN < ge) load_trip(q + UN, nxt);
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      uint4 av[4][TMS];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int t = 0; t < TMS; ++t) {
          const int kstep = (q + u) * 4 + ks;
          if constexpr (ALDS) {
            av[ks][t] = (arow && q + u < ge) ? a_lds[nr * kch + kstep * 4 + g] : make_uint4(0, 0, 0, 0);
          } else {
            uint4 v = cur.a[u][ks][t];
            if constexpr (FUSE == FUSE_ADD_NORM) {
              v = add_round(v, cur.a2[u][ks][t]);
              if (wr_res && abase[t] != OOB && q + u < ge) st16(s.a_out + (16 * t + nr) * s.e.K + kstep * 32 + 8 * g, v);
            }
            if constexpr (FUSE != FUSE_NONE)
              aat[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, v), __builtin_bit_cast(bf16x8, v),
                                                               aat[t], 0, 0, 0);
            av[ks][t] = v;
          }
        }
      if constexpr (SCALED) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const uint4 wv = cur.w[u][j];
          const float sc = __builtin_bit_cast(float, cur.sc[u][j] << 16), off = -136.f * sc;
          const bf16x8 b[4] = {w4_expand_scaled(wv.x, sc, off), w4_expand_scaled(wv.y, sc, off),
                               w4_expand_scaled(wv.z, sc, off), w4_expand_scaled(wv.w, sc, off)};
#pragma unroll
          for (int t = 0; t < TMS; ++t)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
              acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[ks][t]), b[ks], acc[t][j], 0, 0, 0);
        }
        continue;
      }
      f32x4 corr[TMS];  // -136 * (the rows' sums of a over the group)
#pragma unroll
      for (int t = 0; t < TMS; ++t) {
        corr[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          corr[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[ks][t]), neg136, corr[t], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const uint4 wv = cur.w[u][j];
        const bf16x8 b[4] = {w4_expand(wv.x), w4_expand(wv.y), w4_expand(wv.z), w4_expand(wv.w)};
        const float sc = __builtin_bit_cast(float, cur.sc[u][j] << 16);
#pragma unroll
        for (int t = 0; t < TMS; ++t) {
          f32x4 ag = corr[t];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            ag = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[ks][t]), b[ks], ag, 0, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[t][j][i] = fmaf(sc, ag[i], acc[t][j][i]);
        }
      }
    }
  }

  // reduce the waves' partial sums; C layout: acc[t][j][i] = out[m = 16t + 4g + i][n = n0 + 16j + nr]
#pragma unroll
  for (int t = 0; t < TMS; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wid][16 * t + 4 * g + i][16 * j + nr] = acc[t][j][i];
  if constexpr (FUSE != FUSE_NONE && !ALDS) {
#pragma unroll
    for (int t = 0; t < TMS; ++t) {
      // aat[t][i] = (A A^T)[16t + 4g + i][16t + nr]: row nr's diagonal element sits in lane group g = nr / 4
      const int i = nr & 3;
      const float v = i == 0 ? aat[t][0] : i == 1 ? aat[t][1] : i == 2 ? aat[t][2] : aat[t][3];
      if (g == (nr >> 2)) ssq_red[wid][16 * t + nr] = v;
    }
  }
  __syncthreads();
  sk_reduce_store<NWV, 16 * TMS, NT * 16>(red, s.e, n0,
                                          [&](int m) { return FUSE != FUSE_NONE ? sk_rstd(ssq_red, m, s.e) : 1.f; });
}

// launch shapes: (A in LDS, column tiles per block, granules per trip, waves)
struct W4Shape {
  int lds, nt, un, nw;
};
constexpr W4Shape W4_SHAPES[] = {
    {0, 0, 0, 0},   // 0: the launcher's pick
    {1, 1, 2, 16},  // 1
    {1, 1, 1, 8},   // 2
    {1, 2, 1, 16},  // 3
    {0, 1, 1, 16},  // 4
    {0, 1, 1, 8},   // 5
    {0, 2, 1, 8},   // 6
    {0, 4, 1, 8},   // 7
    {0, 2, 1, 16},  // 8
    {1, 2, 1, 8},   // 9
    {1, 4, 1, 8},   // 10
    {1, 1, 1, 8},   // 11: shape 2 with the scaled expansion
    {0, 4, 1, 8},   // 12: shape 7 with the scaled expansion
};
constexpr int W4_NVARIANTS = sizeof(W4_SHAPES) / sizeof(W4_SHAPES[0]);

template <int TMS, int NT, int UN, int NWV, bool ALDS, bool SCALED = false>
void w4_launch(const W4Args& s, int mode, size_t lds, hipStream_t st) {
  const dim3 grid(s.e.N / (16 * NT)), block(NWV * 64);
  with_fuse(mode, [&](auto F) {
    hipLaunchKernelGGL((skinny_w4_kernel<TMS, NT, UN, NWV, decltype(F)::value, ALDS, SCALED>), grid, block, lds, st, s);
  });
}

}  // namespace

extern "C" {

int mls_skinny_w4_num_variants() { return W4_NVARIANTS; }

// W4A16 decode GEMM (+ optional fused add + RMSNorm prologue), M <= 32, N % 16 == 0, K % 128 == 0.
// variant: an index into W4_SHAPES; a shape the call cannot take falls to the nearest one it can
// (LDS staging needs M <= 4 and M K 2 <= 64 KiB, NT tiles per block N % (16 NT) == 0, M > 16 runs
// two 16-row A fragments per granule on 8 waves).
int mls_skinny_w4(const void* A, const void* A2, void* A_out, const void* Wq, const void* scales, const float* bias,
                  const void* res, void* out, int M, int N, int K, int act, int norm, float eps, int variant,
                  void* stream) {
  if (M <= 0 || M > 32 || N <= 0 || N % 16 || K <= 0 || K % 128) return MLS_BAD_ARG;
  if (!A || !Wq || !scales || !out) return MLS_BAD_ARG;
  if (variant < 0 || variant >= W4_NVARIANTS) return MLS_BAD_ARG;
  if (const int rc = sk_check_fuse(A, A2, A_out, norm)) return rc;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K / 2;
  if (wb >= 0x7FFFFFFFull) return MLS_UNSUPPORTED;
  W4Args s{};
  s.e = sk_epi(bias, res, out, M, N, K, act, eps);
  s.a = (const bf16*)A;
  s.a2 = (const bf16*)A2;
  s.a_out = (bf16*)A_out;
  s.w = (const uint8_t*)Wq;
  s.sc = (const bf16*)scales;
  s.a_bytes = (uint32_t)ab;
  s.w_bytes = (uint32_t)wb;
  s.s_bytes = (uint32_t)((size_t)N * K / 128 * 2);
  s.fd_kch = fastdiv_make((uint32_t)(K >> 3));
  const int mode = sk_fuse_mode(A2, norm);
  hipStream_t st = (hipStream_t)stream;
  const bool can_lds = M <= 4 && ab <= 65536;
  W4Shape sh = W4_SHAPES[variant];
  const int tiles = N / 16;
  if (variant == 0)  // measured: profiles/w4_decode_ab.jsonl
    sh = can_lds ? (tiles >= 1024 ? W4Shape{1, 4, 1, 8} : tiles >= 384 ? W4Shape{1, 2, 1, 16} : W4Shape{1, 1, 2, 16})
                 : tiles >= 1024 ? W4Shape{0, 4, 1, 8} : tiles >= 384 ? W4Shape{0, 2, 1, 16} : W4Shape{0, 1, 1, 16};
  while (sh.nt > 1 && N % (16 * sh.nt)) sh.nt >>= 1;
  const bool scaled = variant >= 11;
  if (scaled && M <= 16 && sh.lds && can_lds) {
    w4_launch<1, 1, 1, 8, true, true>(s, mode, ab, st);
  } else if (scaled && M <= 16 && sh.nt >= 4) {
    w4_launch<1, 4, 1, 8, false, true>(s, mode, 0, st);
  } else if (M > 16) {
    if (sh.nt >= 2) w4_launch<2, 2, 1, 8, false>(s, mode, 0, st);
    else w4_launch<2, 1, 1, 8, false>(s, mode, 0, st);
  } else if (sh.lds && can_lds) {
    if (sh.nt >= 4) w4_launch<1, 4, 1, 8, true>(s, mode, ab, st);
    else if (sh.nt == 2 && sh.nw == 8) w4_launch<1, 2, 1, 8, true>(s, mode, ab, st);
    else if (sh.nt == 2) w4_launch<1, 2, 1, 16, true>(s, mode, ab, st);
    else if (sh.nw == 8) w4_launch<1, 1, 1, 8, true>(s, mode, ab, st);
    else w4_launch<1, 1, 2, 16, true>(s, mode, ab, st);
  } else if (sh.nw == 16) {
    if (sh.nt >= 2) w4_launch<1, 2, 1, 16, false>(s, mode, 0, st);
    else w4_launch<1, 1, 1, 16, false>(s, mode, 0, st);
  } else {
    if (sh.nt >= 4) w4_launch<1, 4, 1, 8, false>(s, mode, 0, st);
    else if (sh.nt == 2) w4_launch<1, 2, 1, 8, false>(s, mode, 0, st);
    else w4_launch<1, 1, 1, 8, false>(s, mode, 0, st);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
