// Prompt scoring: the lm_head GEMM fused with the cross-entropy reduction, for one vocabulary shard:
//     logits[M][N] = xn[M][K] . w[N][K]^T        (never stored)
//     m[r] = max_n logits[r][n],  s[r] = sum_n exp(logits[r][n] - m[r])   over the columns n < valid
//     t[r] = logits[r][targets[r] - lo]          (-inf: target -1, outside the shard or in its padded tail)
// so log p(target | row) = t - m - log s once the shards' triples are folded (ops.reference.logprob_merge).
// A [rows][vocab] logit matrix is 513 KB of fp32 per row at vocab 128256; this writes 12 B per (row, 256 columns).
//
// Design.  The k-loop is the persistent LDS-DMA ring of gemm_tile.hip (gemm_ring.h: both operands K-contiguous,
// 16 B per lane buffer_load ... lds with the bank swizzle on the source address, counted vmcnt, one raw barrier per
// 64-deep k-step, the fragment pipeline across a step's two 32-deep halves, XCD-contiguous blocks walking the
// GROUP_M-banded tile order so the blocks that share a 256-row slice of w -- 1.05 GB for Llama-3-8B -- run together
// on one XCD's L2), with the swapped product D = W_tile . A_tile^T: lane (fr, fq) of a 16 x 16 MFMA tile holds row
// m = fr of xn against the 4 consecutive columns n = 4 fq + e.  A row's BN logits are therefore
//   * in one wave: the NTL x 4 accumulator registers of a lane and of the 3 other lanes fq that share its fr --
//     folded in registers, then across lanes by v_permlane16_swap / v_permlane32_swap (xor16_f / xor32_f);
//   * across the WN waves of the block's column split: WN triples per row through 3 floats of LDS scratch past the
//     ring and one block barrier (the shape of ring_epilogue_t's PART combine), folded in wave order by one thread
//     per row, which stores the tile's (m, s, t) to the slab [ceil(N / BN)][M][3].
// No atomics, no tickets, nothing data-dependent in an address: the target only selects among registers.
// Edges: rows >= M and columns >= N read as zero through the buffer range check; columns >= valid (the shard's
// zero-padded tail, and with it every column >= N) are set to -inf before the fold -- a zero logit is not neutral
// for a softmax.  A slice with no valid column has m = -inf, s = 0: exp() is taken against 0 there, never
// (-inf) - (-inf).
// mls_logprob_merge then folds a row's ceil(N / BN) tile triples (one wave per row, lane-strided in tile order, a
// fixed xor tree across lanes) into out[M][3]: deterministic, device arrays only, capturable.
//
// Tiles: BN = 256 (4 waves across, 64 columns each).  BM = 256 (8 waves 2 x 4, 128 x 64 wave tiles, 2-deep ring,
// 128 KB) and BM = 64 (4 waves 1 x 4, 64 x 64 wave tiles, 3-deep ring, 120 KB) for short prompts: below 129 rows
// the launch is bound by streaming w once, and a 256-row tile would spend 2-4x the MFMA time on rows that are not
// there (docs/PERF_NOTES.md, "lm_head log-likelihood").
#include "gemm_ring.h"

namespace {

constexpr int LP_BN = 256;

struct LogprobArgs {
  const bf16* a;       // xn [M][K]
  const bf16* w;       // [N][K]
  const int* targets;  // [M] global token ids, -1: not scored
  float* slab;         // [tiles_n][M][3]
  int M, N, K, lo, valid, vocab;
  uint32_t a_bytes, w_bytes;
  int tiles_n;
};

// (m, s, t) of rows wrow + i * 16 + fr over this wave's WTN columns from column n0 + wcol on, parked by the lanes
// fq == 0 in scr[wn][row][3]
template <int MT, int NTL, int BM>
MLS_DEV void lp_wave_fold(f32x4 (&acc)[MT][NTL], const LogprobArgs& g, int m0, int n0, int wrow, int wcol, int wn,
                          float* scr) {
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int rows = g.M - m0 < BM ? g.M - m0 : BM;
  const rsrc_t rt = make_rsrc(g.targets + m0, (uint32_t)rows * 4u);
  int tl[MT];  // the target's column in this shard (rows past M read 0 and are never stored)
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int r = wrow + i * 16 + fr;
    const int tg = (int)__builtin_amdgcn_raw_buffer_load_b32(rt, r < rows ? r * 4 : OOB, 0, 0);
    MLS_CHECK(r >= rows || (tg >= -1 && tg < g.vocab), 515);
    tl[i] = tg < 0 ? -1 : tg - g.lo;
  }
  const int c0 = n0 + wcol + 4 * fq;  // this lane's first column of column tile jn = 0
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    float mx = -INFINITY;
#pragma unroll
    for (int jn = 0; jn < NTL; ++jn)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float l = c0 + jn * 16 + e < g.valid ? acc[i][jn][e] : -INFINITY;
        acc[i][jn][e] = l;
        mx = fmaxf(mx, l);
      }
    mx = fmaxf(mx, xor16_f(mx));
    mx = fmaxf(mx, xor32_f(mx));
    const float ms = mx == -INFINITY ? 0.f : mx;
    float s = 0.f, t = -INFINITY;
#pragma unroll
    for (int jn = 0; jn < NTL; ++jn)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float l = acc[i][jn][e];
        s += __expf(l - ms);
        t = c0 + jn * 16 + e == tl[i] ? l : t;
      }
    s += xor16_f(s);
    s += xor32_f(s);
    t = fmaxf(t, xor16_f(t));
    t = fmaxf(t, xor32_f(t));
    if (fq == 0) {
      float* p = scr + ((wn * BM) + wrow + i * 16 + fr) * 3;
      p[0] = mx;
      p[1] = s;
      p[2] = t;
    }
  }
}

// fold n triples (stride elements apart) in order; exp() against 0 when no slice has a valid column
MLS_DEV void lp_fold(const float* p, int n, int stride, float& m, float& s, float& t) {
  m = -INFINITY;
  for (int i = 0; i < n; ++i) m = fmaxf(m, p[i * stride]);
  const float ms = m == -INFINITY ? 0.f : m;
  s = 0.f;
  t = -INFINITY;
  for (int i = 0; i < n; ++i) {
    s = fmaf(p[i * stride + 1], __expf(p[i * stride] - ms), s);
    t = fmaxf(t, p[i * stride + 2]);
  }
}

template <int BM, int WM, int STAGES>
__global__ __launch_bounds__(WM * 4 * 64) void lm_logprob_kernel(const LogprobArgs g) {
  constexpr int BN = LP_BN, WN = 4, BKS = 64;
  constexpr int NT = WM * WN * 64;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int MT = WTM / 16, NTL = WTN / 16;
  constexpr int ROWB = BKS * 2, CPR = ROWB / 16;
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int A_LD = A_BYTES / (NT * 16), B_LD = B_BYTES / (NT * 16), LOADS = A_LD + B_LD;
  static_assert(A_BYTES % (NT * 16) == 0 && B_BYTES % (NT * 16) == 0, "stage must split into whole DMA rounds");
  static_assert(NT >= BM, "one thread per row folds the waves' triples");
  // the cross-wave scratch sits past the ring in the SAME __shared__ object (a second one can make hipcc wait
  // vmcnt(0) before every k-step's first ds_read: gemm_tile.hip)
  constexpr int SCR_BYTES = WN * BM * 3 * 4;
  static_assert(STAGES * STAGE_BYTES + SCR_BYTES <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[STAGES * STAGE_BYTES + SCR_BYTES];
  float* const scr = reinterpret_cast<float*>(smem + STAGES * STAGE_BYTES);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid - wm * WN;
  const int tiles_m = (g.M + BM - 1) / BM, ntiles = tiles_m * g.tiles_n;
  const int G = gridDim.x, bq = xcd_remap(blockIdx.x, G);
  const int my_tiles = bq < ntiles ? (ntiles - 1 - bq) / G + 1 : 0;
  const int nk = g.K / BKS, nsteps = my_tiles * nk;

  const rsrc_t ra = make_rsrc(g.a, g.a_bytes), rw = make_rsrc(g.w, g.w_bytes);
  // DMA source: LDS byte i*NT*16 + tid*16 of a stage image is row p / 128, lane-linear chunk tid & 7 = source
  // chunk (tid & 7) ^ swz(row); the tile row / k-step base rides in soffset
  int a_row[A_LD], a_col[A_LD], w_row[B_LD], w_col[B_LD];
#pragma unroll
  for (int i = 0; i < A_LD; ++i) {
    a_row[i] = (i * NT + tid) / CPR;
    a_col[i] = ((tid % CPR) ^ ring_swz<ROWB>(a_row[i])) * 16;
  }
#pragma unroll
  for (int i = 0; i < B_LD; ++i) {
    w_row[i] = (i * NT + tid) / CPR;
    w_col[i] = ((tid % CPR) ^ ring_swz<ROWB>(w_row[i])) * 16;
  }
  const int K2 = g.K * 2;

  auto tile_mn = [&](int ti, int& m0, int& n0) {
    int tm, tn;
    ring_tile(bq + ti * G, tiles_m, g.tiles_n, tm, tn);
    m0 = tm * BM;
    n0 = tn * BN;
  };
  // loader cursor: the (tile, k-step) of the next DMA, running ahead of the compute cursor across tile ends
  int l_ti = 0, l_kt = 0, l_m0 = 0, l_n0 = 0, l_slot = 0;
  if (nsteps > 0) tile_mn(0, l_m0, l_n0);
  auto stage = [&]() {
    const int kt = l_kt, m0 = l_m0, n0 = l_n0;
    char* base = smem + l_slot * STAGE_BYTES + wid * 1024;
    l_slot = l_slot + 1 == STAGES ? 0 : l_slot + 1;
    if (++l_kt == nk) {
      l_kt = 0;
      if (++l_ti < my_tiles) tile_mn(l_ti, l_m0, l_n0);
    }
    const int sa = m0 * K2 + kt * ROWB, sb = n0 * K2 + kt * ROWB;
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      ring_glds16(ra, base + i * NT * 16, m0 + a_row[i] < g.M ? a_row[i] * K2 + a_col[i] : OOB, sa);
#pragma unroll
    for (int i = 0; i < B_LD; ++i)
      ring_glds16(rw, base + A_BYTES + i * NT * 16, n0 + w_row[i] < g.N ? w_row[i] * K2 + w_col[i] : OOB, sb);
  };

  f32x4 acc[MT][NTL];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NTL; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  const int sw = ring_swz<ROWB>(fr);
  const int a_rd = (wm * WTM + fr) * ROWB, w_rd = A_BYTES + (wn * WTN + fr) * ROWB;
  const int coff0 = (fq ^ sw) << 4, coff1 = ((4 + fq) ^ sw) << 4;

#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nsteps) stage();

  int c_kt = 0, c_ti = 0, c_slot = 0;
  for (int j = 0; j < nsteps; ++j) {
    ring_wait<STAGES, LOADS>(nsteps - 1 - j);  // step j landed; later ones may still fly
    ring_barrier();  // step j visible to every wave; step j - 1 fully read by every wave
    if (j + STAGES - 1 < nsteps) stage();
    const char* base = smem + c_slot * STAGE_BYTES;
    c_slot = c_slot + 1 == STAGES ? 0 : c_slot + 1;
    {
      // the k 32-63 W fragments are read up front, each A fragment of k 32-63 right after the last MFMA that
      // reads its k 0-31 register (gemm_tile_kernel's PIPE form)
      bf16x8 af[MT], w0[NTL], w1[NTL];
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn) w0[jn] = *reinterpret_cast<const bf16x8*>(base + w_rd + jn * 16 * ROWB + coff0);
#pragma unroll
      for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const bf16x8*>(base + a_rd + i * 16 * ROWB + coff0);
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn) w1[jn] = *reinterpret_cast<const bf16x8*>(base + w_rd + jn * 16 * ROWB + coff1);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int jn = 0; jn < NTL; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0[jn], af[i], acc[i][jn], 0, 0, 0);
        af[i] = *reinterpret_cast<const bf16x8*>(base + a_rd + i * 16 * ROWB + coff1);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int jn = 0; jn < NTL; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[jn], af[i], acc[i][jn], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (++c_kt < nk) continue;
    c_kt = 0;

    // ---- epilogue of this tile (the next tile's first k-steps are already in flight) ----
    int m0, n0;
    tile_mn(c_ti++, m0, n0);
    lp_wave_fold<MT, NTL, BM>(acc, g, m0, n0, wm * WTM, wn * WTN, wn, scr);
    ring_barrier();  // every wave runs every tile's epilogue: uniform.  The scratch is next written a k-step
                     // barrier (nk >= 2) after these reads
    if (tid < BM && m0 + tid < g.M) {
      float m, s, t;
      lp_fold(scr + tid * 3, WN, BM * 3, m, s, t);
      float* o = g.slab + ((size_t)(n0 / BN) * g.M + m0 + tid) * 3;
      o[0] = m;
      o[1] = s;
      o[2] = t;
    }
    ring_epilogue_done(acc);
  }
}

// one wave per row: lane l folds tiles l, l + 64, ... in order, then the lanes fold by a fixed xor tree
__global__ __launch_bounds__(256) void lm_logprob_merge_kernel(const float* slab, float* out, int M, int tiles) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* p = slab + (size_t)row * 3;
  const size_t stride = (size_t)M * 3;
  float m = -INFINITY;
  for (int i = lane; i < tiles; i += 64) m = fmaxf(m, p[i * stride]);
  m = wave_max(m);
  const float ms = m == -INFINITY ? 0.f : m;
  float s = 0.f, t = -INFINITY;
  for (int i = lane; i < tiles; i += 64) {
    s = fmaf(p[i * stride + 1], __expf(p[i * stride] - ms), s);
    t = fmaxf(t, p[i * stride + 2]);
  }
  s = wave_sum(s);
  t = wave_max(t);
  if (lane == 0) {
    out[row * 3] = m;
    out[row * 3 + 1] = s;
    out[row * 3 + 2] = t;
  }
}

// host rule of M: up to 128 rows the 64-row tile (1-2 row tiles that share each slice of w in one XCD's L2)
int lp_pick(int M) { return M <= 128 ? 2 : 1; }

}  // namespace

extern "C" {

// Per (256-column tile of w, row) the (m, s, t) triple described at the top, into slab [ceil(N / 256)][M][3] fp32.
// Any M >= 1, N >= 1; K % 128 == 0 (else MLS_UNSUPPORTED); 0 <= valid <= N (0: a shard that is all padding).
// vocab: the debug build's bound on a target id (-1 <= id < vocab).  tile: 0 = by M, 1 = 256 rows, 2 = 64 rows.
int mls_linear_logprob(const void* xn, const void* w, const void* targets, void* slab, long long slab_elems, int M,
                       int N, int K, int lo, int valid, int vocab, int tile, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || valid < 0 || valid > N || tile < 0 || tile > 2 || !xn || !w || !targets || !slab)
    return MLS_BAD_ARG;
  if (K % 128) return MLS_UNSUPPORTED;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K * 2;
  const long long tiles_n = (N + LP_BN - 1) / LP_BN;
  if (ab >= 0x7FFFFFFFull || wb >= 0x7FFFFFFFull || tiles_n * M * 3 >= 0x7FFFFFFFll) return MLS_UNSUPPORTED;
  if (slab_elems < tiles_n * M * 3) return MLS_BAD_ARG;
  LogprobArgs g{};
  g.a = (const bf16*)xn;
  g.w = (const bf16*)w;
  g.targets = (const int*)targets;
  g.slab = (float*)slab;
  g.M = M; g.N = N; g.K = K; g.lo = lo; g.valid = valid; g.vocab = vocab;
  g.a_bytes = (uint32_t)ab;
  g.w_bytes = (uint32_t)wb;
  g.tiles_n = (int)tiles_n;
  const int c = tile ? tile : lp_pick(M);
  const int bm = c == 1 ? 256 : 64;
  const dim3 grid = ring_grid((long long)((M + bm - 1) / bm) * tiles_n, mls_num_cus());
  if (c == 1) hipLaunchKernelGGL((lm_logprob_kernel<256, 2, 2>), grid, dim3(512), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL((lm_logprob_kernel<64, 1, 3>), grid, dim3(256), 0, (hipStream_t)stream, g);
  return hipGetLastError() == hipSuccess ? MLS_OK : MLS_BAD_ARG;
}

// slab [tiles][M][3] -> out [M][3]: a row's tile triples folded in tile order
int mls_logprob_merge(const void* slab, void* out, int M, int tiles, void* stream) {
  if (M <= 0 || tiles <= 0 || !slab || !out) return MLS_BAD_ARG;
  hipLaunchKernelGGL(lm_logprob_merge_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     (const float*)slab, (float*)out, M, tiles);
  return hipGetLastError() == hipSuccess ? MLS_OK : MLS_BAD_ARG;
}

}  // extern "C"

MLS_DEBUG_EXPORT(lm_logprob)
