// Skinny GEMM for decode-shaped products (M = batch <= 16 rows by default dispatch): out[M][N] = act(A[M][K] W[N][K]^T + b).
// Memory-bound on W (every weight byte is read exactly once per call), so -- per
// cdna_hip_programming.md §5 "GEMV / M <= 16 decode weights" -- W goes straight to VGPRs with
// 16-B buffer loads (no LDS round trip), many loads in flight per lane (unrolled k loop), and
// the math on v_mfma_f32_16x16x32_bf16 (A = the few activation rows, padded to 16 by the
// descriptor range check; B = 16 weight rows).  Block = 8 waves on one 16-column tile, each
// wave every 8th 32-wide k-step, reduced through LDS; when N/16 tiles cannot fill the chip the grid also
// splits K across blocks (fp32 slabs + a finishing epilogue kernel).  The epilogue fuses bias,
// activation, residual and the SiLU-mul of the interleaved gate/up projection (a 16-column
// tile = 8 gate + 8 up columns).
//
// Fused pre-norm (decode): with `norm` set the kernel computes RMSNorm(a + a2) on the fly -- the
// RMSNorm gain is folded into W's columns at load time, so x_norm @ W^T = rstd[m] * ((a+a2) @ W'^T)
// and rstd only scales the epilogue.  Each block already streams every element of its rows of
// (a + a2) through registers for the MFMA, so the sum of squares costs nothing extra; blocks of
// column tile 0 also write the updated residual stream a + a2 to a_out (a separate buffer: other
// blocks still read a).  This removes the standalone RMSNorm launch (2 per layer) from decode.
#include "skinny_tiles.h"
#include "ar_protocol.h"

namespace {

struct SkArgs {
  const bf16* a;   // [M][lda]
  const bf16* a2;  // optional [M][lda] added to a (residual-stream update)
  bf16* a_out;     // optional [M][lda] <- a + a2 (written by column-tile-0 blocks)
  const bf16* w;   // [N][K]
  float* ws;       // [nsplit][M][N]
  // bias, res, out, M, N, K, ldo, act, eps.  Behind ws, so that M, N, K and a_bytes, w_bytes keep the
  // offsets they had as plain fields: with `e` in front of ws the row-major LDS kernel measured 0.1 us
  // slower at one row with its own staging and epilogue text unchanged (docs/PERF_NOTES.md)
  SkEpi e;
  int lda, nsplit, ksteps_per_split, norm;
  uint32_t a_bytes, w_bytes;
  // FUSE_COMBINE (packed LDS kernel): A = the split-KV decode attention's merged output, combined
  // here from its fp32 partials (o [M][Hq][nsplit][D], (m, l) [M][Hq][nsplit][2]); rows whose
  // sequence fit one split were written to `a` directly by the attention kernel
  const float* cws;
  const float* cml;
  const int* lens;
  int c_nsplit, c_chunk, c_hq, c_hd;
  const float* wscale;  // fp8 weights: per-output-channel dequantisation scale [N]
  // fused tensor-parallel all-reduce of `out` (ar_protocol.h; world == 0: none): the row-parallel
  // decode projections reduce their partial sums across ranks in their own epilogue
  ArFuse arf;
  // runtime divisors of the A staging loops (fastdiv.h): K / 8 chunks per row, combine head dim
  FastDiv fd_kch, fd_hd;
};

// NT 16-column tiles per block: every A fragment a wave loads feeds NT MFMAs, so the activation
// traffic from L2 (M rows x K per block) is amortised over NT weight tiles -- at M = 16 it equals
// the weight traffic when NT = 1.
template <int TMS, int UNROLL, int NWV, int FUSE, int NT>
__global__ __launch_bounds__(NWV * 64) void skinny_gemm_kernel(const SkArgs s) {
  __shared__ float red[NWV][TMS * 16][NT * 16 + 1];
  __shared__ float ssq_red[NWV][TMS * 16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  const int split = blockIdx.y;
  const int ks_beg = split * s.ksteps_per_split;
  const int ksteps = (s.e.K + 31) / 32;
  const int ks_end = min(ksteps, ks_beg + s.ksteps_per_split);
  const rsrc_t ar = make_rsrc(s.a, s.a_bytes);
  const rsrc_t wr = make_rsrc(s.w, s.w_bytes);
  const rsrc_t a2r = make_rsrc(s.a2, FUSE == FUSE_ADD_NORM ? s.a_bytes : 0);
  const bool wr_res = FUSE == FUSE_ADD_NORM && s.a_out && blockIdx.x == 0;
  int wbase[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) wbase[j] = ((n0 + 16 * j + nr) * s.e.K + 8 * g) * 2;
  int abase[TMS];
#pragma unroll
  for (int t = 0; t < TMS; ++t) {
    const int m = 16 * t + nr;
    abase[t] = m < s.e.M ? (m * s.lda + 8 * g) * 2 : OOB;
  }
  f32x4 acc[TMS][NT];
  float ssq[TMS];
#pragma unroll
  for (int t = 0; t < TMS; ++t) {
    ssq[t] = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // U k-steps per trip: issue every load first, then the math, then (tile-0 blocks) the
  // residual-stream stores
  auto body = [&](int ks0, auto U_) {
    constexpr int U = decltype(U_)::value;
    uint4 wv[U][NT], av[U][TMS], a2v[U][TMS];
    int aoff[U][TMS];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = (ks0 + NWV * u) * 32;
      const bool kin = k + 8 * g < s.e.K;
#pragma unroll
      for (int j = 0; j < NT; ++j) wv[u][j] = bload16(wr, kin ? wbase[j] + k * 2 : OOB);
#pragma unroll
      for (int t = 0; t < TMS; ++t) {
        aoff[u][t] = (kin && abase[t] != OOB) ? abase[t] + k * 2 : OOB;
        av[u][t] = bload16(ar, aoff[u][t]);
        if constexpr (FUSE == FUSE_ADD_NORM) a2v[u][t] = bload16(a2r, aoff[u][t]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < TMS; ++t) {
        if constexpr (FUSE == FUSE_ADD_NORM) av[u][t] = add_round(av[u][t], a2v[u][t]);
        if constexpr (FUSE != FUSE_NONE) ssq[t] += sumsq8(av[u][t]);
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[u][t]),
                                                              __builtin_bit_cast(bf16x8, wv[u][j]), acc[t][j], 0, 0, 0);
      }
    if constexpr (FUSE == FUSE_ADD_NORM) {
      if (wr_res) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int t = 0; t < TMS; ++t)
            if (aoff[u][t] != OOB) st16(s.a_out + aoff[u][t] / 2, av[u][t]);
      }
    }
  };
  int ks = ks_beg + wid;
  for (; ks + NWV * (UNROLL - 1) < ks_end; ks += NWV * UNROLL) body(ks, std::integral_constant<int, UNROLL>{});
  for (; ks < ks_end; ks += NWV) body(ks, std::integral_constant<int, 1>{});

  // C layout: acc[t][j][i] = out[m = 16t + 4g + i][n = n0 + 16j + nr]
#pragma unroll
  for (int t = 0; t < TMS; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wid][16 * t + 4 * g + i][16 * j + nr] = acc[t][j][i];
  if constexpr (FUSE != FUSE_NONE) {
    // lanes nr, nr+16, nr+32, nr+48 hold row nr's four 8-element k slices
#pragma unroll
    for (int t = 0; t < TMS; ++t) {
      float v = ssq[t];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (g == 0) ssq_red[wid][16 * t + nr] = v;
    }
  }
  __syncthreads();
  constexpr int COLS = NT * 16;
  if (s.nsplit > 1) {  // fp32 slabs for skinny_finish_kernel; the partial square sums ride after them
    for (int q = tid; q < TMS * 16 * COLS; q += NWV * 64) {
      const int m = q / COLS, c = q % COLS;
      if (m >= s.e.M) continue;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NWV; ++w) v += red[w][m][c];
      s.ws[((size_t)split * s.e.M + m) * s.e.N + n0 + c] = v;
      if constexpr (FUSE != FUSE_NONE) {
        if (blockIdx.x == 0 && c == 0) {
          float t2 = 0.f;
#pragma unroll
          for (int w = 0; w < NWV; ++w) t2 += ssq_red[w][m];
          s.ws[(size_t)s.nsplit * s.e.M * s.e.N + split * s.e.M + m] = t2;
        }
      }
    }
    return;
  }
  sk_reduce_store<NWV, TMS * 16, COLS, true>(red, s.e, n0,
                                             [&](int m) { return FUSE != FUSE_NONE ? sk_rstd(ssq_red, m, s.e) : 1.f; });
}

// Few-row variant (M <= 4, whole K per block): the activation rows -- with the fused prologue,
// a + a2 rounded to the bf16 residual stream -- are staged ONCE per block into LDS (M*K*2 bytes,
// dynamic) together with their square sums, so the k loop is the plain weight stream with the
// A fragments read from LDS; the block's first weight loads are issued before that prologue and
// every later trip's loads are in flight while the previous trip's MFMAs run (register double
// buffer).  Measured motivation: the register-path fused kernel streamed gate_up ~20 % slower
// than the plain one (profiles/r1_decode_cold_weight_stream_probe.jsonl).
template <int UNROLL, int NWV, int FUSE, int NT>
__global__ __launch_bounds__(NWV * 64) void skinny_lds_kernel(const SkArgs s) {
  extern __shared__ __attribute__((aligned(16))) uint4 a_lds[];  // [M][K/8]
  __shared__ float red[NWV][16][NT * 16 + 1];
  __shared__ float ssq_s[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  const int ksteps = s.e.K >> 5;
  const int kch = s.e.K >> 3;  // 16-B chunks per row
  const rsrc_t wr = make_rsrc(s.w, s.w_bytes);
  int wbase[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) wbase[j] = ((n0 + 16 * j + nr) * s.e.K + 8 * g) * 2;

  auto load_trip = [&](int ks0, uint4 (&wv)[UNROLL][NT]) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int ks = ks0 + NWV * u;
#pragma unroll
      for (int j = 0; j < NT; ++j) wv[u][j] = bload16(wr, ks < ksteps ? wbase[j] + ks * 64 : OOB);
    }
  };
  uint4 wnext[UNROLL][NT];
  int ks = wid;
  load_trip(ks, wnext);  // in flight during the prologue

  // prologue: A (+ A2) -> LDS, residual write-back (column-tile-0 blocks), square sums
  constexpr bool NORM = FUSE == FUSE_NORM || FUSE == FUSE_ADD_NORM;
  if (tid < 4) ssq_s[tid] = 0.f;
  __syncthreads();
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  const bool wr_res = FUSE == FUSE_ADD_NORM && s.a_out && blockIdx.x == 0;
  for (int q = tid; q < s.e.M * kch; q += NWV * 64) {
    const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
    uint4 v = ld16(s.a + (size_t)m * s.lda + c * 8);
    if constexpr (FUSE == FUSE_ADD_NORM) {
      v = add_round(v, ld16(s.a2 + (size_t)m * s.lda + c * 8));
      if (wr_res) st16(s.a_out + (size_t)m * s.lda + c * 8, v);
    }
    a_lds[q] = v;
    if constexpr (NORM) {
      const float sq = sumsq8(v);
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) part[mm] += mm == m ? sq : 0.f;
    }
  }
  if constexpr (NORM) {
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
      const float t = wave_sum(part[mm]);
      if (lane == 0 && mm < s.e.M) atomicAdd(&ssq_s[mm], t);
    }
  }
  __syncthreads();

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool arow = nr < s.e.M;
  for (; ks < ksteps; ks += NWV * UNROLL) {
    uint4 wv[UNROLL][NT];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j) wv[u][j] = wnext[u][j];
    if (ks + NWV * UNROLL < ksteps) load_trip(ks + NWV * UNROLL, wnext);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int k = ks + NWV * u;
      const uint4 av = (arow && k < ksteps) ? a_lds[nr * kch + k * 4 + g] : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av),
                                                         __builtin_bit_cast(bf16x8, wv[u][j]), acc[j], 0, 0, 0);
    }
  }
  // reduce the waves' partial sums; C layout: acc[j][i] = out[m = 4g + i][n = n0 + 16j + nr]
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wid][4 * g + i][16 * j + nr] = acc[j][i];
  __syncthreads();
  sk_reduce_store<NWV, 16, NT * 16>(red, s.e, n0, [&](int m) { return NORM ? sk_rstd(ssq_s[m], s.e) : 1.f; });
}

// Packed-weight variant of skinny_lds_kernel (M <= 4).  W is re-laid out once at load time
// (pack_skinny_weight) so the 64 lanes' MFMA B fragments of one (16-row tile, 32-wide k-step) are
// one contiguous 1 KiB granule: [tile][kstep][g][nr][8].  Each wave then streams a CONTIGUOUS
// range of granules (its 1/NWV of the tile's k-steps), so every load instruction reads 1 KiB of
// consecutive bytes and consecutive instructions continue the same run -- instead of 16 rows x
// 64 B scattered K*2 bytes apart per instruction in the row-major layout.  NTL: non-temporal
// cache policy on the weight stream (read exactly once per call).
template <int UNROLL, int NWV, int FUSE, int NTL>
__global__ __launch_bounds__(NWV * 64) void skinny_packed_kernel(const SkArgs s) {
  extern __shared__ __attribute__((aligned(16))) uint4 a_lds[];  // [M][K/8]
  __shared__ float red[NWV][16][17];
  __shared__ float ssq_s[4];
  constexpr int T = NWV * 64;
  constexpr bool NORM = FUSE == FUSE_NORM || FUSE == FUSE_ADD_NORM;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int ksteps = s.e.K >> 5;
  const int kch = s.e.K >> 3;
  const int kpw = (ksteps + NWV - 1) / NWV;
  const int kb = wid * kpw, ke = min(ksteps, kb + kpw);
  const rsrc_t wr = make_rsrc(s.w, s.w_bytes);
  const rsrc_t ar = make_rsrc(s.a, s.a_bytes);
  const rsrc_t a2r = make_rsrc(s.a2, FUSE == FUSE_ADD_NORM ? s.a_bytes : 0);
  const int wbase = blockIdx.x * ksteps * 1024 + lane * 16;

  auto load_trip = [&](int ks0, uint4 (&wv)[UNROLL]) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) wv[u] = bload16_pol<NTL>(wr, ks0 + u < ke ? wbase + (ks0 + u) * 1024 : OOB);
  };
  const int nq = s.e.M * kch;
  // The staging below (early loads, stage step, tail loop) is repeated in skinny_fp8_kernel and
  // skinny_w4_kernel<ALDS>: shared as a closure it cost each of the three 0.05-0.1 us per launch
  // (docs/PERF_NOTES.md, "csrc/skinny_tiles.h"), so a fix to one has to be made in the others.
  // The first QPT A (+ A2) chunks per thread -- all of A up to 2048 chunks, e.g. 4 rows at K = 4096
  // -- are loaded BEFORE the first weight trip: the vector memory counter retires in order, so
  // consuming them then does not wait for the weights, and the barriers below are LDS-only (a
  // __syncthreads would drain the weight loads too).  Larger A goes through the loop after.
  constexpr int QPT = 2048 / T;
  uint4 a0[QPT], a20[QPT];
#pragma unroll
  for (int j = 0; j < QPT; ++j) {
    const int q = tid + j * T;
    const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
    const int off = q < nq ? (m * s.lda + c * 8) * 2 : OOB;
    a0[j] = bload16(ar, off);
    if constexpr (FUSE == FUSE_ADD_NORM) a20[j] = bload16(a2r, off);
  }
  uint4 wnext[UNROLL];
  load_trip(kb, wnext);  // in flight during the prologue

  if (tid < 4) ssq_s[tid] = 0.f;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  const bool wr_res = FUSE == FUSE_ADD_NORM && s.a_out && blockIdx.x == 0;
  int lens4[4] = {0, 0, 0, 0};
  if constexpr (FUSE == FUSE_COMBINE) {
    // block-uniform reads (scalar loads): they do not queue behind the weight loads in flight
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) lens4[mm] = mm < s.e.M ? __builtin_nontemporal_load(s.lens + mm) : 0;
  }
  auto stage = [&](int q, uint4 v, uint4 v2) {
    const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
    if constexpr (FUSE == FUSE_COMBINE) {
      // the decode_combine_kernel arithmetic for this row's 8 dims of one head
      const int h = fastdiv(c * 8, s.fd_hd), d0 = c * 8 - h * s.c_hd;
      const int L = m == 0 ? lens4[0] : m == 1 ? lens4[1] : m == 2 ? lens4[2] : lens4[3];
      const int ns = min(s.c_nsplit, (L + s.c_chunk - 1) / s.c_chunk);
      if (ns > 1) v = splitkv_merge(m, h, d0, ns, s.cws, s.cml, s.c_hq, s.c_nsplit, s.c_hd);
    }
    if constexpr (FUSE == FUSE_ADD_NORM) {
      v = add_round(v, v2);
      if (wr_res) st16(s.a_out + (size_t)m * s.lda + c * 8, v);
    }
    a_lds[q] = v;
    if constexpr (NORM) {
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
    stage(q, ld16(s.a + (size_t)m * s.lda + c * 8),
          FUSE == FUSE_ADD_NORM ? ld16(s.a2 + (size_t)m * s.lda + c * 8) : make_uint4(0, 0, 0, 0));
  }
  if constexpr (NORM) {
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
      const float t = wave_sum(part[mm]);
      if (lane == 0 && mm < s.e.M) atomicAdd(&ssq_s[mm], t);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool arow = nr < s.e.M;
  for (int ks = kb; ks < ke; ks += UNROLL) {
    uint4 wv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) wv[u] = wnext[u];
    if (ks + UNROLL < ke) load_trip(ks + UNROLL, wnext);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int k = ks + u;
      const uint4 av = (arow && k < ke) ? a_lds[nr * kch + k * 4 + g] : make_uint4(0, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, wv[u]),
                                                    acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wid][4 * g + i][nr] = acc[i];
  __syncthreads();
  sk_reduce_store<NWV, 16, 16>(red, s.e, n0, [&](int m) { return NORM ? sk_rstd(ssq_s[m], s.e) : 1.f; });
  if (s.arf.world) ar_fused_tail(s.arf, s.e.out, s.e.M, s.e.N, n0, 16);
}

// Packed weights, M <= 16 (or A too large for LDS): the A fragments (+ A2) ride beside the weight
// granules in registers, read per k-step from L2 (every block re-reads A; at M = 16 that is half
// the weight bytes, all L2 / MALL hits), register double-buffered like the weight stream.  Each
// wave folds its own k range of the RMSNorm square sums; the block reduces them through LDS.
template <int UNROLL, int NWV, int FUSE, int NTL, int NT, int TMS>
__global__ __launch_bounds__(NWV * 64) void skinny_packed_reg_kernel(const SkArgs s) {
  __shared__ float red[NWV][16 * TMS][NT * 16 + 1];
  __shared__ float ssq_red[NWV][16 * TMS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  const int ksteps = s.e.K >> 5;
  const int kpw = (ksteps + NWV - 1) / NWV;
  const int kb = wid * kpw, ke = min(ksteps, kb + kpw);
  const rsrc_t wr = make_rsrc(s.w, s.w_bytes);
  const rsrc_t ar = make_rsrc(s.a, s.a_bytes);
  const rsrc_t a2r = make_rsrc(s.a2, FUSE == FUSE_ADD_NORM ? s.a_bytes : 0);
  const int wbase = blockIdx.x * NT * ksteps * 1024 + lane * 16;  // tile j: + j * ksteps * 1024
  int abase[TMS];
#pragma unroll
  for (int t = 0; t < TMS; ++t) abase[t] = 16 * t + nr < s.e.M ? ((16 * t + nr) * s.lda + 8 * g) * 2 : OOB;
  const bool wr_res = FUSE == FUSE_ADD_NORM && s.a_out && blockIdx.x == 0;

  struct Trip {
    uint4 w[UNROLL][NT], a[UNROLL][TMS], a2[UNROLL][TMS];
  };
  auto load_trip = [&](int ks0, Trip& tr) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const bool in = ks0 + u < ke;
#pragma unroll
      for (int j = 0; j < NT; ++j)
        tr.w[u][j] = bload16_pol<NTL>(wr, in ? wbase + (j * ksteps + ks0 + u) * 1024 : OOB);
#pragma unroll
      for (int t = 0; t < TMS; ++t) {
        const int ao = (in && abase[t] != OOB) ? abase[t] + (ks0 + u) * 64 : OOB;
        tr.a[u][t] = bload16(ar, ao);
        if constexpr (FUSE == FUSE_ADD_NORM) tr.a2[u][t] = bload16(a2r, ao);
      }
    }
  };
  Trip nxt;
  load_trip(kb, nxt);
  f32x4 acc[TMS][NT];
  float ssq[TMS];
#pragma unroll
  for (int t = 0; t < TMS; ++t) {
    ssq[t] = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int ks = kb; ks < ke; ks += UNROLL) {
    Trip cur = nxt;
    if (ks + UNROLL < ke) load_trip(ks + UNROLL, nxt);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int t = 0; t < TMS; ++t) {
        uint4 av = cur.a[u][t];
        if constexpr (FUSE == FUSE_ADD_NORM) {
          av = add_round(av, cur.a2[u][t]);
          if (wr_res && abase[t] != OOB && ks + u < ke)
            st16(s.a_out + (16 * t + nr) * s.lda + (ks + u) * 32 + 8 * g, av);
        }
        if constexpr (FUSE != FUSE_NONE) ssq[t] += sumsq8(av);
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av),
                                                              __builtin_bit_cast(bf16x8, cur.w[u][j]), acc[t][j], 0, 0, 0);
      }
  }
#pragma unroll
  for (int t = 0; t < TMS; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wid][16 * t + 4 * g + i][16 * j + nr] = acc[t][j][i];
  if constexpr (FUSE != FUSE_NONE) {
#pragma unroll
    for (int t = 0; t < TMS; ++t) {
      float v = ssq[t];  // lanes nr, nr+16, nr+32, nr+48 hold row 16t+nr's k slices
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (g == 0) ssq_red[wid][16 * t + nr] = v;
    }
  }
  __syncthreads();
  constexpr int COLS = NT * 16;
  sk_reduce_store<NWV, 16 * TMS, COLS>(red, s.e, n0,
                                       [&](int m) { return FUSE != FUSE_NONE ? sk_rstd(ssq_red, m, s.e) : 1.f; });
  if (s.arf.world) ar_fused_tail(s.arf, s.e.out, s.e.M, s.e.N, n0, COLS);
}


// FP8 (OCP e4m3) weight-and-activation decode GEMM, M <= 4: W8A8 with a per-output-channel weight
// scale and a per-row dynamic activation scale, on v_mfma_f32_16x16x32_fp8_fp8.  Half the weight
// bytes of the bf16 stream (decode is weight-bandwidth bound).  W is packed in 1 KiB granules of
// 16 rows x 64 k ([N/16][K/64][g][nr][2 k-steps][8]), so one 16-B load per lane feeds two MFMAs.
// Prologue: A (+ A2) staged in LDS as bf16 with the row square sums and |max|, then requantised
// in place to fp8 with scale |max| / 448; epilogue: acc * s_a[m] * s_w[n] (* rstd[m]).
template <int UNROLL, int NWV, int FUSE>
__global__ __launch_bounds__(NWV * 64) void skinny_fp8_kernel(const SkArgs s) {
  extern __shared__ __attribute__((aligned(16))) uint4 a_lds[];  // bf16 [M][K], then fp8 [M][K]
  __shared__ float red[NWV][16][17];
  __shared__ float ssq_s[4];
  __shared__ int amax_s[4];
  constexpr int T = NWV * 64;
  constexpr bool NORM = FUSE == FUSE_NORM || FUSE == FUSE_ADD_NORM;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int kgs = s.e.K >> 6;  // 64-wide granules per row
  const int kch = s.e.K >> 3;
  const int nq = s.e.M * kch;
  const int kpw = (kgs + NWV - 1) / NWV;
  const int kb = wid * kpw, ke = min(kgs, kb + kpw);
  const rsrc_t wr = make_rsrc(s.w, s.w_bytes);
  const rsrc_t ar = make_rsrc(s.a, s.a_bytes);
  const rsrc_t a2r = make_rsrc(s.a2, FUSE == FUSE_ADD_NORM ? s.a_bytes : 0);
  const int wbase = blockIdx.x * kgs * 1024 + lane * 16;

  auto load_trip = [&](int kg0, uint4 (&wv)[UNROLL]) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) wv[u] = bload16_pol<1>(wr, kg0 + u < ke ? wbase + (kg0 + u) * 1024 : OOB);
  };
  constexpr int QPT = 2048 / T;
  uint4 a0[QPT], a20[QPT];
#pragma unroll
  for (int j = 0; j < QPT; ++j) {
    const int q = tid + j * T;
    const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
    const int off = q < nq ? (m * s.lda + c * 8) * 2 : OOB;
    a0[j] = bload16(ar, off);
    if constexpr (FUSE == FUSE_ADD_NORM) a20[j] = bload16(a2r, off);
  }
  uint4 wnext[UNROLL];
  load_trip(kb, wnext);

  if (tid < 4) {
    ssq_s[tid] = 0.f;
    amax_s[tid] = 0;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  float part[4] = {0.f, 0.f, 0.f, 0.f}, amx[4] = {0.f, 0.f, 0.f, 0.f};
  const bool wr_res = FUSE == FUSE_ADD_NORM && s.a_out && blockIdx.x == 0;
  auto stage = [&](int q, uint4 v, uint4 v2) {
    const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
    if constexpr (FUSE == FUSE_ADD_NORM) {
      v = add_round(v, v2);
      if (wr_res) st16(s.a_out + (size_t)m * s.lda + c * 8, v);
    }
    a_lds[q] = v;
    float x[8];
    unpack8(v, x);
    float sq = 0.f, mx = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sq += x[e] * x[e];
      mx = fmaxf(mx, fabsf(x[e]));
    }
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
      part[mm] += mm == m ? sq : 0.f;
      amx[mm] = mm == m ? fmaxf(amx[mm], mx) : amx[mm];
    }
  };
#pragma unroll
  for (int j = 0; j < QPT; ++j)
    if (tid + j * T < nq) stage(tid + j * T, a0[j], a20[j]);
  for (int q = tid + QPT * T; q < nq; q += T) {
    const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
    stage(q, ld16(s.a + (size_t)m * s.lda + c * 8),
          FUSE == FUSE_ADD_NORM ? ld16(s.a2 + (size_t)m * s.lda + c * 8) : make_uint4(0, 0, 0, 0));
  }
#pragma unroll
  for (int mm = 0; mm < 4; ++mm) {
    const float t = wave_sum(part[mm]);
    const float mxw = wave_max(amx[mm]);
    if (lane == 0 && mm < s.e.M) {
      if constexpr (NORM) atomicAdd(&ssq_s[mm], t);
      atomicMax(&amax_s[mm], __float_as_int(mxw));  // non-negative floats order as their bits
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  // requantise A to fp8 in place: every thread first reads its chunks, then (after a barrier) writes
  float inv[4];
#pragma unroll
  for (int mm = 0; mm < 4; ++mm) {
    const float amax = __int_as_float(amax_s[mm]);
    inv[mm] = amax > 0.f ? 448.f / amax : 0.f;
  }
  constexpr int QMAX = 4096 / T;  // M * K / 8 <= 4096 chunks (host: M * K * 2 <= 64 KiB)
  uint4 hold[QMAX];
#pragma unroll
  for (int j = 0; j < QMAX; ++j) {
    const int q = tid + j * T;
    hold[j] = q < nq ? a_lds[q] : make_uint4(0, 0, 0, 0);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  uint2* a8 = reinterpret_cast<uint2*>(a_lds);  // fp8 [M][K]: chunk q -> 8 bytes at q * 8
#pragma unroll
  for (int j = 0; j < QMAX; ++j) {
    const int q = tid + j * T;
    if (q < nq) {
      const int m = fastdiv(q, s.fd_kch);
      const float sc = m == 0 ? inv[0] : m == 1 ? inv[1] : m == 2 ? inv[2] : inv[3];
      float x[8];
      unpack8(hold[j], x);
      int lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * sc, x[1] * sc, 0, false);
      lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * sc, x[3] * sc, lo, true);
      int hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] * sc, x[5] * sc, 0, false);
      hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] * sc, x[7] * sc, hi, true);
      a8[q] = make_uint2((uint32_t)lo, (uint32_t)hi);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool arow = nr < s.e.M;
  const char* a8b = reinterpret_cast<const char*>(a_lds) + nr * s.e.K + 8 * g;
  for (int kg = kb; kg < ke; kg += UNROLL) {
    uint4 wv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) wv[u] = wnext[u];
    if (kg + UNROLL < ke) load_trip(kg + UNROLL, wnext);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int k = kg + u;
      const bool ok = arow && k < ke;
      const long x0 = ok ? *reinterpret_cast<const long*>(a8b + k * 64) : 0;
      const long x1 = ok ? *reinterpret_cast<const long*>(a8b + k * 64 + 32) : 0;
      const long w0 = (long)(((unsigned long)wv[u].y << 32) | wv[u].x);
      const long w1 = (long)(((unsigned long)wv[u].w << 32) | wv[u].z);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(x0, w0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(x1, w1, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wid][4 * g + i][nr] = acc[i];
  __syncthreads();
  // acc * s_a[m] * s_w[n] (* rstd[m])
  sk_reduce_store<NWV, 16, 16>(
      red, s.e, n0,
      [&](int m) { return (NORM ? sk_rstd(ssq_s[m], s.e) : 1.f) * (__int_as_float(amax_s[m]) * (1.f / 448.f)); },
      [&](int n) { return s.wscale[n]; });
}

// [N][K] row-major -> [N/16][K/32][4][16][8] (the packed granule layout above)
__global__ __launch_bounds__(256) void pack_skinny_kernel(const bf16* __restrict__ w, bf16* __restrict__ wp, int N,
                                                          int K) {
  const int ksteps = K >> 5;
  const long total = (long)N * (K >> 3);  // 16-B chunks
  for (long q = blockIdx.x * 256L + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
    const int lane = (int)(q & 63);
    const long gr = q >> 6;  // granule = tile * ksteps + ks
    const int ks = (int)(gr % ksteps), tile = (int)(gr / ksteps);
    const int n = tile * 16 + (lane & 15), k = ks * 32 + 8 * (lane >> 4);
    st16(wp + q * 8, ld16(w + (size_t)n * K + k));
  }
}

__global__ __launch_bounds__(256) void skinny_finish_kernel(const SkArgs s) {
  const bool glu = s.e.act == ACT_SILU_MUL;
  const int ncols = glu ? s.e.N / 2 : s.e.N;
  const long total = (long)s.e.M * ncols;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int m = (int)(q / ncols), c = (int)(q % ncols);
    const int n = glu ? (c / 8) * 16 + (c % 8) : c;
    float v = 0.f, u = 0.f;
    for (int sp = 0; sp < s.nsplit; ++sp) {
      const float* row = s.ws + ((size_t)sp * s.e.M + m) * s.e.N;
      v += row[n];
      if (glu) u += row[n + 8];
    }
    if (s.norm) {
      float t2 = 0.f;
      for (int sp = 0; sp < s.nsplit; ++sp) t2 += s.ws[(size_t)s.nsplit * s.e.M * s.e.N + sp * s.e.M + m];
      const float rs = sk_rstd(t2, s.e);
      v *= rs;
      u *= rs;
    }
    sk_emit(s.e, glu, m, n, v, u);
  }
}

// what every launcher fills: A (+ A2, A_out) [M][K], the weights (wb bytes), the epilogue, no K split
SkArgs sk_args(const void* A, const void* A2, void* A_out, const void* W, size_t wb, const float* bias, const void* res,
               void* out, int M, int N, int K, int act, int norm, float eps, const ArFuse* arf = nullptr) {
  SkArgs s{};
  s.e = sk_epi(bias, res, out, M, N, K, act, eps);
  s.a = (const bf16*)A;
  s.a2 = (const bf16*)A2;
  s.a_out = (bf16*)A_out;
  s.w = (const bf16*)W;
  s.lda = K;
  s.nsplit = 1;
  s.norm = norm;
  s.a_bytes = (uint32_t)((size_t)M * K * 2);
  s.w_bytes = (uint32_t)wb;
  s.fd_kch = fastdiv_make((uint32_t)(K >> 3));
  if (arf) s.arf = *arf;
  return s;
}

// one launch per kernel family: the shape from the caller, the fusion mode at run time (with_fuse)
template <int TMS, int UN, int NT>
void launch_gemm(const SkArgs& s, int mode, dim3 grid, hipStream_t st) {
  with_fuse(mode, [&](auto F) {
    hipLaunchKernelGGL((skinny_gemm_kernel<TMS, UN, 8, decltype(F)::value, NT>), grid, dim3(512), 0, st, s);
  });
}
template <int TMS, int UN>
void launch_gemm_nt(const SkArgs& s, int mode, int nt, dim3 grid, hipStream_t st) {
  if (nt == 4) launch_gemm<TMS, (UN > 4 ? 4 : UN), 4>(s, mode, grid, st);
  else if (nt == 2) launch_gemm<TMS, UN, 2>(s, mode, grid, st);
  else launch_gemm<TMS, UN, 1>(s, mode, grid, st);
}
template <int UN, int NT>
void launch_lds(const SkArgs& s, int mode, dim3 grid, hipStream_t st) {
  with_fuse(mode, [&](auto F) {
    hipLaunchKernelGGL((skinny_lds_kernel<UN, 8, decltype(F)::value, NT>), grid, dim3(512), s.a_bytes, st, s);
  });
}
template <int UN, int NW, int NT, int TM = 1>
void launch_reg(const SkArgs& s, int mode, hipStream_t st) {
  with_fuse(mode, [&](auto F) {
    hipLaunchKernelGGL((skinny_packed_reg_kernel<UN, NW, decltype(F)::value, 1, NT, TM>), dim3(s.e.N / (16 * NT)),
                       dim3(NW * 64), 0, st, s);
  });
}
template <int UN, int NW, int NTL>
void launch_packed(const SkArgs& s, int mode, hipStream_t st) {
  with_fuse(mode, [&](auto F) {
    hipLaunchKernelGGL((skinny_packed_kernel<UN, NW, decltype(F)::value, NTL>), dim3(s.e.N / 16), dim3(NW * 64),
                       s.a_bytes, st, s);
  });
}
template <int UN, int NW>
void launch_fp8(const SkArgs& s, int mode, hipStream_t st) {
  with_fuse(mode, [&](auto F) {
    hipLaunchKernelGGL((skinny_fp8_kernel<UN, NW, decltype(F)::value>), dim3(s.e.N / 16), dim3(NW * 64), s.a_bytes, st,
                       s);
  });
}

}  // namespace

int g_skinny_no_lds = 0;     // A/B switch for probes (mls_skinny_set_variant)
int g_skinny_max_split = 0;  // cap on the automatic cross-block K split (0: none)

extern "C" {

int mls_ar_fuse_desc(void* ctx, long n, ArFuse* f);  // custom_allreduce.hip

int mls_skinny_set_variant(int no_lds) {
  g_skinny_no_lds = no_lds;
  return 0;
}

int mls_skinny_set_max_split(int cap) {
  g_skinny_max_split = cap;
  return 0;
}

// M <= 32, N % 16 == 0, K % 8 == 0.  nsplit <= 0: auto (fill the chip).  ws: >= nsplit*M*(N+1) floats.
// A2 / A_out / norm: the fused residual-add + RMSNorm prologue (header comment); A_out must not alias A/A2.
int mls_skinny_gemm_norm(const void* A, const void* A2, void* A_out, const void* W, const float* bias, const void* res,
                         void* out, void* ws, size_t ws_bytes, int M, int N, int K, int act, int nsplit, int norm,
                         float eps, void* stream) {
  if (M <= 0 || M > 32 || N % 16 || K % 8 || K <= 0) return MLS_BAD_ARG;
  if (const int rc = sk_check_fuse(A, A2, A_out, norm)) return rc;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K * 2;
  if (ab >= 0x7FFFFFFFull || wb >= 0x7FFFFFFFull) return MLS_UNSUPPORTED;
  SkArgs s = sk_args(A, A2, A_out, W, wb, bias, res, out, M, N, K, act, norm, eps);
  s.ws = (float*)ws;
  // M > 2: NT tiles per block while that still leaves >= 384 blocks (1.5 per CU) -- measured: NT = 4
  // halves gate_up at M = 16 but costs ~10 % at M = 1, where the activation traffic is negligible
  // and the deeper single-tile unroll wins (profiles/r1_decode_probe.jsonl).  K is split across
  // blocks only when even single-tile blocks cannot cover 256 CUs.
  int nt = 1;
  while (M > 2 && nt < 4 && N % (32 * nt) == 0 && N / (32 * nt) >= 384) nt *= 2;
  const int tiles = N / (16 * nt);
  const int ksteps = (K + 31) / 32;
  if (nsplit <= 0) {  // 8 waves split K inside a block; split across blocks only below 256 blocks
    nsplit = 1;
    // M <= 4 with >= 32 column tiles: never split -- the finish launch costs more than the idle
    // CUs (emulated TP = 8 rank, batch 1: 1.55 -> 1.44 ms/token; TP = 1 unchanged, its GEMMs
    // already have >= 256 tiles).  At M = 8 the split still wins (1.67 vs 1.73 ms/token).
    const bool no_split = M <= 4 && tiles >= 32;
    while (!no_split && tiles * nsplit < 256 && ksteps / (nsplit * 2) >= 32) nsplit *= 2;
    if (g_skinny_max_split > 0 && nsplit > g_skinny_max_split) nsplit = g_skinny_max_split;
  }
  if (nsplit > 1 && (ws == nullptr || ws_bytes < (size_t)nsplit * M * (N + 1) * 4)) nsplit = 1;
  s.nsplit = nsplit;
  s.ksteps_per_split = (ksteps + nsplit - 1) / nsplit;
  dim3 grid(tiles, nsplit);
  hipStream_t st = (hipStream_t)stream;
  const int mode = sk_fuse_mode(A2, norm);
  if (M <= 4 && nsplit == 1 && K % 32 == 0 && ab <= 65536 && !g_skinny_no_lds) {
    if (nt == 4) launch_lds<4, 4>(s, mode, grid, st);
    else if (nt == 2) launch_lds<4, 2>(s, mode, grid, st);
    else launch_lds<8, 1>(s, mode, grid, st);
    return (int)hipGetLastError();
  }
  if (M <= 16) launch_gemm_nt<1, 8>(s, mode, nt, grid, st);
  else launch_gemm_nt<2, 4>(s, mode, nt, grid, st);
  if (nsplit > 1) {
    const long total = (long)M * (act == ACT_SILU_MUL ? N / 2 : N);
    int blocks = (int)((total + 255) / 256);
    blocks = blocks > 2048 ? 2048 : blocks;
    hipLaunchKernelGGL(skinny_finish_kernel, dim3(blocks), dim3(256), 0, st, s);
  }
  return (int)hipGetLastError();
}

// W [N][K] -> packed granules (N % 16 == 0, K % 32 == 0); Wp must not alias W.
int mls_skinny_pack(const void* W, void* Wp, int N, int K, void* stream) {
  if (N <= 0 || K <= 0 || N % 16 || K % 32 || W == Wp) return MLS_BAD_ARG;
  const long chunks = (long)N * (K / 8);
  int blocks = (int)((chunks + 255) / 256);
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(pack_skinny_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)W, (bf16*)Wp,
                     N, K);
  return (int)hipGetLastError();
}

// Packed-weight skinny GEMM (+ optional fused add + RMSNorm prologue), M <= 32.  M <= 4 with A
// within 64 KiB stages A in LDS (skinny_packed_kernel), otherwise A rides in registers
// (skinny_packed_reg_kernel; variant | 16 forces it).  variant = probe knob, (granules per trip,
// waves, non-temporal): 0 (8,8,no) 1 (8,8,nt) 2 (8,4,no) 3 (8,4,nt) 4 (16,8,no) 5 (16,8,nt)
// 6 (16,4,no) 7 (16,4,nt) 8 (8,16,nt) 9 (4,16,nt; the measured default) 10 (4,8,nt); register
// path only: 11 / 12 = (4,8) over 2 / 4 column tiles per block, 13 = (4,16) over 2.
static int skinny_packed_impl(const void* A, const void* A2, void* A_out, const void* Wp, const float* bias,
                              const void* res, void* out, int M, int N, int K, int act, int norm, float eps, int variant,
                              void* stream, const ArFuse* arf) {
  if (M <= 0 || M > 32 || N % 16 || K % 32 || K <= 0) return MLS_BAD_ARG;
  if (const int rc = sk_check_fuse(A, A2, A_out, norm)) return rc;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K * 2;
  if (wb >= 0x7FFFFFFFull) return MLS_UNSUPPORTED;
  const SkArgs s = sk_args(A, A2, A_out, Wp, wb, bias, res, out, M, N, K, act, norm, eps, arf);
  const int mode = sk_fuse_mode(A2, norm);
  hipStream_t st = (hipStream_t)stream;
  if (M > 4 || ab > 65536 || (variant & 16)) {  // A fragments from L2 in registers (16: forced)
    int v = variant & 15;
    if (M > 16) {  // two 16-row A fragments per granule
      if (N / 16 >= 384 && N % 32 == 0 && v != 10) {
        launch_reg<4, 8, 2, 2>(s, mode, st);  // 8 waves: the double-buffered 2-tile trip needs > 128 VGPRs
      } else if (v == 10) {
        launch_reg<4, 8, 1, 2>(s, mode, st);
      } else {
        launch_reg<4, 16, 1, 2>(s, mode, st);
      }
      return (int)hipGetLastError();
    }
    // default: two column tiles per block once there are >= 384 tiles (A fragments amortised over
    // two weight granules; M = 8: QKV 14.3 -> 12.1 us, gate_up 47.0 -> 43.4), else one tile, 16 waves
    // (profiles/r2_decode_packed_weight_probe.jsonl)
    if (v == 9 && N / 16 >= 384) v = 11;
    if ((v == 11 || v == 13) && N % 32) v = 9;
    if (v == 12 && N % 64) v = 9;
    switch (v) {
      case 1: launch_reg<8, 8, 1>(s, mode, st); break;
      case 10: launch_reg<4, 8, 1>(s, mode, st); break;
      case 11: launch_reg<4, 8, 2>(s, mode, st); break;
      case 12: launch_reg<4, 8, 4>(s, mode, st); break;
      case 13: launch_reg<4, 16, 2>(s, mode, st); break;
      default: launch_reg<4, 16, 1>(s, mode, st); break;
    }
    return (int)hipGetLastError();
  }
  switch (variant) {
    case 0: launch_packed<8, 8, 0>(s, mode, st); break;
    case 2: launch_packed<8, 4, 0>(s, mode, st); break;
    case 3: launch_packed<8, 4, 1>(s, mode, st); break;
    case 4: launch_packed<16, 8, 0>(s, mode, st); break;
    case 5: launch_packed<16, 8, 1>(s, mode, st); break;
    case 6: launch_packed<16, 4, 0>(s, mode, st); break;
    case 7: launch_packed<16, 4, 1>(s, mode, st); break;
    case 8: launch_packed<8, 16, 1>(s, mode, st); break;
    case 9: launch_packed<4, 16, 1>(s, mode, st); break;
    case 10: launch_packed<4, 8, 1>(s, mode, st); break;
    default: launch_packed<8, 8, 1>(s, mode, st); break;  // 1: the measured default
  }
  return (int)hipGetLastError();
}

// Packed-weight decode GEMM whose A operand is the split-KV decode attention's output, merged
// from its partials in the prologue (FUSE_COMBINE; the attention launch then skips its combine
// kernel).  M <= 4, M * K * 2 <= 64 KiB, K == Hq * D, D % 8 == 0.
static int skinny_packed_combine_impl(const void* A, const float* cws, const float* cml, const int* lens, int nsplit,
                                      int chunk, int Hq, int D, const void* Wp, const float* bias, const void* res,
                                      void* out, int M, int N, int K, int act, int variant, void* stream,
                                      const ArFuse* arf) {
  if (M <= 0 || M > 4 || N % 16 || K % 32 || K != Hq * D || D % 8 || nsplit <= 0 || chunk <= 0) return MLS_BAD_ARG;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K * 2;
  if (wb >= 0x7FFFFFFFull || ab > 65536) return MLS_UNSUPPORTED;
  SkArgs s = sk_args(A, nullptr, nullptr, Wp, wb, bias, res, out, M, N, K, act, 0, 0.f, arf);
  s.cws = cws;
  s.cml = cml;
  s.lens = lens;
  s.c_nsplit = nsplit;
  s.c_chunk = chunk;
  s.c_hq = Hq;
  s.c_hd = D;
  s.fd_hd = fastdiv_make((uint32_t)D);
  hipStream_t st = (hipStream_t)stream;
  if (variant == 1)
    hipLaunchKernelGGL((skinny_packed_kernel<8, 8, FUSE_COMBINE, 1>), dim3(N / 16), dim3(512), ab, st, s);
  else
    hipLaunchKernelGGL((skinny_packed_kernel<4, 16, FUSE_COMBINE, 1>), dim3(N / 16), dim3(1024), ab, st, s);
  return (int)hipGetLastError();
}

int mls_skinny_packed(const void* A, const void* A2, void* A_out, const void* Wp, const float* bias, const void* res,
                      void* out, int M, int N, int K, int act, int norm, float eps, int variant, void* stream) {
  return skinny_packed_impl(A, A2, A_out, Wp, bias, res, out, M, N, K, act, norm, eps, variant, stream, nullptr);
}

int mls_skinny_packed_combine(const void* A, const float* cws, const float* cml, const int* lens, int nsplit,
                              int chunk, int Hq, int D, const void* Wp, const float* bias, const void* res, void* out,
                              int M, int N, int K, int act, int variant, void* stream) {
  return skinny_packed_combine_impl(A, cws, cml, lens, nsplit, chunk, Hq, D, Wp, bias, res, out, M, N, K, act, variant,
                                    stream, nullptr);
}

// Row-parallel tensor-parallel projection with its all-reduce FUSED (ar_protocol.h): out = the sum
// over the ranks of A . Wp^T, reduced in this launch through the one-shot IPC context ar_ctx
// (custom_allreduce.hip) -- no bias / residual / activation (they would be summed world times).
// out must be contiguous [M][N] with M * N * 2 <= the context's one-shot cap.
static int ar_fuse_check(void* ar_ctx, const float* bias, const void* res, int act, int M, int N, ArFuse* f) {
  if (!ar_ctx || bias || res || act != ACT_NONE) return MLS_BAD_ARG;
  return mls_ar_fuse_desc(ar_ctx, (long)M * N, f);
}

int mls_skinny_packed_ar(const void* A, const void* A2, void* A_out, const void* Wp, const void* out_, int M, int N,
                         int K, int norm, float eps, int variant, void* ar_ctx, void* stream) {
  ArFuse f;
  const int rc = ar_fuse_check(ar_ctx, nullptr, nullptr, ACT_NONE, M, N, &f);
  if (rc) return rc;
  return skinny_packed_impl(A, A2, A_out, Wp, nullptr, nullptr, const_cast<void*>(out_), M, N, K, ACT_NONE, norm, eps,
                            variant, stream, &f);
}

int mls_skinny_packed_combine_ar(const void* A, const float* cws, const float* cml, const int* lens, int nsplit,
                                 int chunk, int Hq, int D, const void* Wp, void* out, int M, int N, int K, int variant,
                                 void* ar_ctx, void* stream) {
  ArFuse f;
  const int rc = ar_fuse_check(ar_ctx, nullptr, nullptr, ACT_NONE, M, N, &f);
  if (rc) return rc;
  return skinny_packed_combine_impl(A, cws, cml, lens, nsplit, chunk, Hq, D, Wp, nullptr, nullptr, out, M, N, K,
                                    ACT_NONE, variant, stream, &f);
}

// FP8 (e4m3) decode GEMM (W8A8, see skinny_fp8_kernel): M <= 4, K % 64 == 0, M * K * 2 <= 64 KiB.
// Wq: packed fp8 granules; wscale [N] fp32.  Same fusion options as mls_skinny_packed.
int mls_skinny_fp8(const void* A, const void* A2, void* A_out, const void* Wq, const float* wscale, const float* bias,
                   const void* res, void* out, int M, int N, int K, int act, int norm, float eps, int variant,
                   void* stream) {
  if (M <= 0 || M > 4 || N % 16 || K % 64 || K <= 0 || !wscale) return MLS_BAD_ARG;
  if (const int rc = sk_check_fuse(A, A2, A_out, norm)) return rc;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K;
  if (wb >= 0x7FFFFFFFull || ab > 65536) return MLS_UNSUPPORTED;
  SkArgs s = sk_args(A, A2, A_out, Wq, wb, bias, res, out, M, N, K, act, norm, eps);
  s.wscale = wscale;
  const int mode = sk_fuse_mode(A2, norm);
  hipStream_t st = (hipStream_t)stream;
  // variant: 1 (default) 4 granules per trip x 8 waves; 0: 4 x 16; 2: 2 x 16
  // (profiles/r2_decode_fp8_weight_probe.jsonl: 1 is fastest on every Llama-3-8B shape)
  if (variant == 0) launch_fp8<4, 16>(s, mode, st);
  else if (variant == 2) launch_fp8<2, 16>(s, mode, st);
  else launch_fp8<4, 8>(s, mode, st);
  return (int)hipGetLastError();
}

int mls_skinny_gemm(const void* A, const void* W, const float* bias, const void* res, void* out, void* ws,
                    size_t ws_bytes, int M, int N, int K, int act, int nsplit, void* stream) {
  return mls_skinny_gemm_norm(A, nullptr, nullptr, W, bias, res, out, ws, ws_bytes, M, N, K, act, nsplit, 0, 0.f,
                              stream);
}

}  // extern "C"
