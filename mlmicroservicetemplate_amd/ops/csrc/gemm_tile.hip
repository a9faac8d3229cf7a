// K2 of SURVEY.md §2.E.1 for large M: the transformer projection GEMM on gfx950 MFMA,
//     out[M][N] = act(A[M][K] . W[N][K]^T + bias[N]) (+ residual[M][N])
// (BERT QKV / O / FFN at T = B*S tokens, Llama prefill QKV / O / gate_up / down / lm_head).  This is
// the kernel that replaces the hipBLASLt call ops.linear used to make for M >= 33.
//
// The ring primitives, the split-K combine, the tile epilogue and the design notes they share with
// gemm_w8a8.hip are gemm_ring.h's.  This file holds the bf16 ring kernel (a 128-B LDS row = BK 64, one 16-B
// ds_read_b128 of 8 consecutive k per 16x16x32 MFMA fragment; plain and PIPE), the LayerNorm-folding
// dispatch, the probe-only arms (x2 epilogue, stamps, ping-pong and deep-ring kernels), the cfg table and
// the launchers.
#include "gemm_ring.h"

namespace {

struct GemmTileArgs {
  const bf16* a;
  const bf16* w;
  const float* bias;  // [N] or nullptr
  const bf16* res;    // [M][ldr] or nullptr
  bf16* out;          // [M][ldo]
  int M, N, K, act, ldo, ldr;
  uint32_t a_bytes, w_bytes;
  int tiles_n;
  int flags;  // probe-only ablations (GT_ABL_*), 0 in every real call
  int splitk;  // K splits per output tile (>= 1); > 1: fp32 slabs in ws + per-tile arrival counters
  float* ws;   // [tiles][splitk][BM * BN] fp32 partial tiles (fragment-linear)
  int* cnt;    // [tiles] arrival counters: zero before the launch, reset to zero by each tile's reducer
  // LayerNorm folding (see "LayerNorm folding" below)
  const float* fold_c;    // EPI 4: [N] sum_k W'[n][k] of the gamma-folded weight
  const float* ln_part;   // EPI 3 / 4: [M][P][2] row partials (sum, sum of squares) of the LN'd operand,
                          // P = its width / 128 (as a PART epilogue wrote them)
  const float* ln_g;      // EPI 3: [N] fp32 gamma of the residual's LN (its beta is folded into bias)
  float* stats_part;      // PART: [M][N / 128][2] partials of the OUTPUT rows, one per 128-column block
                          // (its two 64-column waves combined through LDS): M * N / 64 floats
  float eps;
  static constexpr bool SCALED = false;  // ring_epilogue_t: acc + bias
  MLS_DEV int res_pitch() const { return ldr; }
};

#define GCONST4 __attribute__((address_space(4)))

// The bf16x4-per-lane form of the epilogue (one 8-B store per (i, jn), scalar-loaded bias): kept as
// the A/B arm of the 16-B form (cfg 19 = cfg 1 with it) -- probe only.
template <int MT, int NTL, int EPI, int ACT>
MLS_DEV void gt_epilogue_x2(f32x4 (&acc)[MT][NTL], const GemmTileArgs& g, int m0, int n0, int wrow, int wcol) {
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int ldo2 = g.ldo * 2, ldr2 = g.ldr * 2;
  const int rows = g.M - m0 < 256 ? g.M - m0 : 256;
  const bool nostore = g.flags & GT_ABL_NOSTORE;
  const rsrc_t ro = make_rsrc(g.out + (size_t)m0 * g.ldo, nostore ? 0u : (uint32_t)(rows * ldo2));
  const rsrc_t rr = make_rsrc(EPI == 1 ? g.res + (size_t)m0 * g.ldr : g.out, EPI == 1 ? (uint32_t)(rows * ldr2) : 0u);
#pragma unroll
  for (int jn = 0; jn < NTL; ++jn) {
    const int nt0 = n0 + wcol + jn * 16, n = nt0 + 4 * fq;
    const bool col_ok = nt0 < g.N;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f}, bu = {0.f, 0.f, 0.f, 0.f};
    if (g.bias && col_ok && !(g.flags & GT_ABL_NOBIAS)) {
      const GCONST4 f32x4* bp = (const GCONST4 f32x4*)(g.bias + nt0);
      const f32x4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
      bv = fq == 0 ? b0 : fq == 1 ? b1 : fq == 2 ? b2 : b3;
      bu = fq == 0 ? b2 : b3;
    }
    uint2 rv[MT];
    if constexpr (EPI == 1) {
#pragma unroll
      for (int i = 0; i < MT; ++i) rv[i] = bload8(rr, col_ok ? (wrow + i * 16 + fr) * ldr2 + n * 2 : OOB);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int r = wrow + i * 16 + fr;
      const f32x4 v = acc[i][jn];
      bf16x4 b;
      int off;
      if constexpr (EPI == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (bf16)(silu_fast(v[e] + bv[e]) * (xor32_f(v[e]) + bu[e]));
        off = fq < 2 && col_ok ? r * ldo2 + ((nt0 >> 1) + 4 * fq) * 2 : OOB;
      } else {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = v[e] + bv[e];
          o[e] = ACT == ACT_GELU ? gelu_fast(x) : ACT == ACT_RELU ? fmaxf(x, 0.f) : ACT == ACT_SILU ? silu_fast(x)
                 : ACT == ACT_TANH ? tanhf(x) : x;
        }
        if constexpr (EPI == 1) {
          const bf16x4 rb = __builtin_bit_cast(bf16x4, rv[i]);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += (float)rb[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (bf16)o[e];
        off = col_ok ? r * ldo2 + n * 2 : OOB;
      }
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, b), ro, off, 0, 0);
    }
  }
}

#define GT_EPI_CALL(ACTV)                                                   \
  do {                                                                      \
    if constexpr (X2) gt_epilogue_x2<MT, NTL, EPI, ACTV>(acc, g, m0, n0, wrow, wcol); \
    else ring_epilogue_t<MT, NTL, EPI, ACTV>(acc, g, m0, n0, wrow, wcol);    \
  } while (0)
template <int MT, int NTL, int EPI, bool X2>
MLS_DEV void gt_epilogue_a(f32x4 (&acc)[MT][NTL], const GemmTileArgs& g, int m0, int n0, int wrow, int wcol) {
  switch (g.act) {
    case ACT_GELU: GT_EPI_CALL(ACT_GELU); break;
    case ACT_RELU: GT_EPI_CALL(ACT_RELU); break;
    case ACT_SILU: GT_EPI_CALL(ACT_SILU); break;
    case ACT_TANH: GT_EPI_CALL(ACT_TANH); break;
    default: GT_EPI_CALL(ACT_NONE); break;
  }
}

// dispatch once per tile, then zero the accumulators for the next tile in one straight run.  LN: the
// LayerNorm-folding epilogues (EPI 3 / 4, + row statistics) -- gemm_tile_kernel instantiations only
// LNK 1: the folded projection (EPI 4, act none / gelu); LNK 2: the residual projection (EPI 1 / 3,
// + PART when g.stats_part) -- one instantiation per kind keeps each kernel's register peak to its own
template <int MT, int NTL, int LNK, int BM, int WN>
MLS_DEV void gt_epilogue_ln(f32x4 (&acc)[MT][NTL], const GemmTileArgs& g, int m0, int n0, int wrow, int wcol,
                            float* pscr) {
  if constexpr (LNK == 1) {
    if (g.act == ACT_GELU) ring_epilogue_t<MT, NTL, 4, ACT_GELU>(acc, g, m0, n0, wrow, wcol);
    else ring_epilogue_t<MT, NTL, 4, ACT_NONE>(acc, g, m0, n0, wrow, wcol);
  } else if (g.stats_part) {
    if (g.ln_part) ring_epilogue_t<MT, NTL, 3, ACT_NONE, true, BM, WN>(acc, g, m0, n0, wrow, wcol, pscr);
    else ring_epilogue_t<MT, NTL, 1, ACT_NONE, true, BM, WN>(acc, g, m0, n0, wrow, wcol, pscr);
  } else {
    if (g.ln_part) ring_epilogue_t<MT, NTL, 3, ACT_NONE>(acc, g, m0, n0, wrow, wcol);
    else ring_epilogue_t<MT, NTL, 1, ACT_NONE>(acc, g, m0, n0, wrow, wcol);
  }
}
// LNK != 0: pscr = the LDS scratch past the ring that a PART epilogue combines its waves through
template <int MT, int NTL, bool X2 = false, int LNK = 0, int BM = 256, int WN = 4>
MLS_DEV void gt_epilogue(f32x4 (&acc)[MT][NTL], const GemmTileArgs& g, int m0, int n0, int wrow, int wcol,
                         float* pscr = nullptr) {
  if constexpr (LNK != 0) {
    gt_epilogue_ln<MT, NTL, LNK, BM, WN>(acc, g, m0, n0, wrow, wcol, pscr);
  } else if (g.act == ACT_SILU_MUL) {
    if constexpr (X2) gt_epilogue_x2<MT, NTL, 2, ACT_NONE>(acc, g, m0, n0, wrow, wcol);
    else ring_epilogue_t<MT, NTL, 2, ACT_NONE>(acc, g, m0, n0, wrow, wcol);
  } else if (g.res) {
    gt_epilogue_a<MT, NTL, 1, X2>(acc, g, m0, n0, wrow, wcol);
  } else {
    gt_epilogue_a<MT, NTL, 0, X2>(acc, g, m0, n0, wrow, wcol);
  }
  ring_epilogue_done(acc);
}

// In-kernel stamps (cdna_hip_programming.md §7) for the STAMP build of the tile kernel (cfg 13/14 =
// cfg 1/2 + stamps, probe only): s_memtime with its own lgkmcnt wait, fenced by sched_barriers.
MLS_DEV unsigned long long gt_stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
MLS_DEV unsigned long long gt_realtime() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}

// LayerNorm folding (BERT post-LN: x = LN(h) feeds the next projection AND the residual add after
// it).  No LN kernel runs and x is never formed:
//  * the producer of h (O / FFN-down projection, residual epilogue) stores h and, per output row and
//    128-column block, the sum and sum of squares of the bf16 values it stored (PART: [M][N/128][2],
//    the block's two 64-column waves combined through LDS);
//  * the projection that consumes x reads A = h and W' = W . diag(gamma): x . W^T = rstd * (h . W'^T -
//    mu * c) + beta . W^T with c[n] = sum_k W'[n][k], applied to the accumulator in the epilogue
//    (EPI 4);
//  * the residual add after it normalizes its residual operand in the epilogue: (h - mu) * rstd *
//    gamma + beta (EPI 3);
//  * both consumers finish each row's (mu, rstd) from the partials themselves (ring_row_stats; the
//    loads ride beside the bias loads) -- the kernel boundary orders them after the producer, so no
//    cross-block protocol or extra launch is needed.
// Removes the LN launch and its T x H read + write per LayerNorm.
template <int BM, int BN, int WM, int WN, int STAGES, int BKS, bool STAMP = false, bool PIPE = false, bool X2 = false,
          int LNK = 0>
__global__ __launch_bounds__(WM * WN * 64) void gemm_tile_kernel(const GemmTileArgs g0) {
  static_assert(LNK == 0 || (!STAMP && !X2 && BN / WN == 64), "LayerNorm-folding builds: 64-column wave tiles");
  // STAMP: g0.res is the stamp buffer [grid][8] (u64): t0 start, t1 first k-step landed, t2 first
  // tile's last MFMA, t3 its epilogue issued, t4 all stores retired, t5/t6 realtime at t0/t4, t7 tiles
  unsigned long long st[5] = {0, 0, 0, 0, 0}, rt0 = 0;
  GemmTileArgs g = g0;
  if constexpr (STAMP) {
    g.res = nullptr;
    st[0] = gt_stamp();
    rt0 = gt_realtime();
  }
  constexpr int NT = WM * WN * 64;
  constexpr int WTM = BM / WM, WTN = BN / WN;  // wave tile: WTM rows (m) x WTN columns (n)
  constexpr int MT = WTM / 16, NTL = WTN / 16;
  constexpr int ROWB = BKS * 2, CPR = ROWB / 16;  // bytes / 16-B chunks per LDS row
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int A_LD = A_BYTES / (NT * 16), B_LD = B_BYTES / (NT * 16), LOADS = A_LD + B_LD;
  static_assert(A_BYTES % (NT * 16) == 0 && B_BYTES % (NT * 16) == 0, "stage must split into whole DMA rounds");
  static_assert(BKS == 32 || BKS == 64, "stage depth");
  // + 16 B: the split-K "last arriver" flag -- in the SAME __shared__ object as the ring (a second
  // one can make hipcc wait vmcnt(0) before every k-step's first ds_read: §5 item 4(a))
  // LNK == 2: [WN][BM] float2 scratch past the ring for the PART epilogue's cross-wave combine
  constexpr int PSCR_BYTES = LNK == 2 ? WN * BM * 8 : 0;
  static_assert(STAGES * STAGE_BYTES + 16 + PSCR_BYTES <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[STAGES * STAGE_BYTES + 16 + PSCR_BYTES];
  float* const pscr = reinterpret_cast<float*>(smem + STAGES * STAGE_BYTES + 16);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid - wm * WN;
  const int tiles_m = (g.M + BM - 1) / BM, ntiles = tiles_m * g.tiles_n;
  // work unit = (tile, K split): unit u -> tile u / S, split u % S (the S splits of a tile are
  // adjacent units, so they land on one XCD and its reducer reads same-XCD slabs).  Persistent:
  // block b takes units b', b' + G, ... where b' = XCD-contiguous remap of b
  const int S = g.splitk, nunits = ntiles * S;
  const int G = gridDim.x, bq = xcd_remap(blockIdx.x, G);
  const int my_tiles = bq < nunits ? (nunits - 1 - bq) / G + 1 : 0;  // units of this block
  const int nk = g.K / BKS / S, nsteps = my_tiles * nk;              // k-steps per unit

  const rsrc_t ra = make_rsrc(g.a, g.a_bytes), rw = make_rsrc(g.w, g.w_bytes);
  // DMA source: LDS byte p = i*NT*16 + tid*16 of a stage image is row p / 128, lane-linear chunk
  // tid & 7 = source chunk (tid & 7) ^ swz(row); the tile row / k-step base rides in soffset
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

  // unit ui of this block -> tile origin (m0, n0) and its first k-step k0
  auto tile_mn = [&](int ti, int& m0, int& n0, int& k0) {
    const int u = bq + ti * G, t = S == 1 ? u : u / S;
    int tm, tn;
    ring_tile(t, tiles_m, g.tiles_n, tm, tn);
    m0 = tm * BM;
    n0 = tn * BN;
    k0 = (u - t * S) * nk;
  };
  // loader cursor: the (unit, k-step) of the next DMA, advanced without divisions
  int l_ti = 0, l_kt = 0, l_m0 = 0, l_n0 = 0, l_k0 = 0, l_slot = 0;
  if (nsteps > 0) tile_mn(0, l_m0, l_n0, l_k0);
  auto stage = [&]() {  // DMA the loader cursor's k-step into ring slot l_slot, then advance it
    const int kt = l_k0 + l_kt, m0 = l_m0, n0 = l_n0;
    char* base = smem + l_slot * STAGE_BYTES + wid * 1024;
    l_slot = l_slot + 1 == STAGES ? 0 : l_slot + 1;
    if (++l_kt == nk) {
      l_kt = 0;
      if (++l_ti < my_tiles) tile_mn(l_ti, l_m0, l_n0, l_k0);
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

  // fragment reads inside a stage image (row r, 16-B chunk c -> r*128 + (c ^ swz(r))*16)
  const int fr = lane & 15, fq = lane >> 4;
  const int sw = ring_swz<ROWB>(fr);  // tile rows are 16-aligned: swz(r) depends on r & 15 only
  const int a_rd = (wm * WTM + fr) * ROWB, w_rd = A_BYTES + (wn * WTN + fr) * ROWB;


#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nsteps) stage();

  int c_kt = 0, c_ti = 0, c_slot = 0;  // compute cursor
  for (int j = 0; j < nsteps; ++j) {
    ring_wait<STAGES, LOADS>(nsteps - 1 - j);  // step j landed; later ones may still fly
    ring_barrier();  // step j visible to every wave; step j - 1 fully read by every wave
    if constexpr (STAMP)
      if (j == 0) st[1] = gt_stamp();
    if (j + STAGES - 1 < nsteps) stage();
    const char* base = smem + c_slot * STAGE_BYTES;
    c_slot = c_slot + 1 == STAGES ? 0 : c_slot + 1;
    if constexpr (PIPE && BKS == 64) {
      // fragment pipeline across the two 32-deep halves of the step: the k 32-63 W fragments are
      // read up front, each A fragment of k 32-63 right after the last MFMA that reads its k 0-31
      // register -- the second half's LDS latency hides under the first half's MFMAs instead of
      // stalling both waves of the SIMD after them
      const int coff0 = (fq ^ sw) << 4, coff1 = ((4 + fq) ^ sw) << 4;
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
    } else {
#pragma unroll
    for (int ks = 0; ks < BKS / 32; ++ks) {
      const int coff = ((ks * 4 + fq) ^ sw) << 4;
      bf16x8 af[MT], wf[NTL];
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn) wf[jn] = *reinterpret_cast<const bf16x8*>(base + w_rd + jn * 16 * ROWB + coff);
#pragma unroll
      for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const bf16x8*>(base + a_rd + i * 16 * ROWB + coff);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int jn = 0; jn < NTL; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[jn], af[i], acc[i][jn], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    }
    if (++c_kt < nk) continue;
    c_kt = 0;

    // ---- epilogue of this unit (the next unit's first k-steps are already in flight) ----
    int m0, n0, k0;
    if constexpr (STAMP)
      if (c_ti == 0) st[2] = gt_stamp();
    const int cu = bq + c_ti * G;
    tile_mn(c_ti++, m0, n0, k0);
    // LNK: the LayerNorm-folding epilogues live in their own instantiations (all of them in one
    // kernel cost ~30 VGPRs + ~60 SGPRs kernel-wide and spilled the 256 x 256 tile)
    const bool reducer = S == 1 || ring_splitk_arrive<BM * BN, MT, NTL>(acc, g.ws, g.cnt, S, cu / S, cu - (cu / S) * S,
                                                                        (int*)(smem + STAGES * STAGE_BYTES));
    if (reducer) gt_epilogue<MT, NTL, X2, LNK, BM, WN>(acc, g, m0, n0, wm * WTM, wn * WTN, pscr);
    if constexpr (STAMP)
      if (c_ti == 1) st[3] = gt_stamp();
  }
  if constexpr (STAMP) {
    ring_wait_vmcnt<0>();
    st[4] = gt_stamp();
    const unsigned long long rt1 = gt_realtime();
    if (threadIdx.x == 0) {
      unsigned long long* o = (unsigned long long*)g0.res + blockIdx.x * 8;
#pragma unroll
      for (int k = 0; k < 5; ++k) o[k] = st[k];
      o[5] = rt0;
      o[6] = rt1;
      o[7] = (unsigned long long)my_tiles;
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Ping-pong variant (cfg 8 / 9): the 8 waves are two groups of 4 -- group 0 = waves 0-3, group 1 =
// waves 4-7, one wave of each per SIMD -- and group 1 runs one barrier behind group 0.  Each wave's
// k-step is an L section (DMA issue + every ds_read of the step's fragments) and an M section (its
// MFMAs only), separated by block barriers; with the one-barrier stagger, in every barrier interval
// one wave per SIMD is in its M section while the other loads, so the MFMA pipe never waits on LDS
// latency or the barrier (the structure of cdna_hip_programming.md §5's 256^2 template, at k-step
// granularity).  Barrier intervals I_k: group 0 reads stage s in I_{2s-1} and multiplies in I_{2s};
// group 1 reads in I_{2s} and multiplies in I_{2s+1}.  Stage s + 1 (same buffer as s - 1, free once
// group 1 finished reading s - 1 in I_{2s-2}) is DMA'd in two halves: group 0 issues the A tile in
// its L section (I_{2s-1}), group 1 the W tile in its M section of step s - 1 (I_{2s-1}); both
// retire their half with vmcnt(0) before barrier B_{2s+1}, the first after which stage s + 1 is
// read -- ~1.5 intervals of slack for every DMA.
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(512) void gemm_pp_kernel(const GemmTileArgs g) {
  static_assert(WM * WN == 8, "8 waves");
  constexpr int WTM = BM / WM, WTN = BN / WN, MT = WTM / 16, NTL = WTN / 16;
  constexpr int ROWB = 128, A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int A_LD = A_BYTES / (256 * 16), B_LD = B_BYTES / (256 * 16);  // per thread of its group
  static_assert(A_BYTES % (256 * 16) == 0 && B_BYTES % (256 * 16) == 0, "whole DMA rounds per group");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int grp = __builtin_amdgcn_readfirstlane(wid >> 2), gt = tid & 255, gw = (tid >> 6) & 3;
  const int wm = wid / WN, wn = wid - wm * WN;
  const int tiles_m = (g.M + BM - 1) / BM, ntiles = tiles_m * g.tiles_n;
  const int G = gridDim.x, bq = xcd_remap(blockIdx.x, G);
  const int my_tiles = bq < ntiles ? (ntiles - 1 - bq) / G + 1 : 0;
  const int nk = g.K / 64, nsteps = my_tiles * nk;
  const rsrc_t ra = make_rsrc(g.a, g.a_bytes), rw = make_rsrc(g.w, g.w_bytes);
  const int K2 = g.K * 2;
  // this thread's DMA pieces: group 0 copies the A tile, group 1 the W tile of a stage
  constexpr int LD = A_LD > B_LD ? A_LD : B_LD;
  const int nld = grp == 0 ? A_LD : B_LD;
  int d_row[LD], d_col[LD];
#pragma unroll
  for (int i = 0; i < LD; ++i) {
    d_row[i] = (i * 256 + gt) >> 3;
    d_col[i] = ((gt & 7) ^ ring_swz<128>(d_row[i])) * 16;
  }
  auto tile_mn = [&](int ti, int& m0, int& n0) {
    int tm, tn;
    ring_tile(bq + ti * G, tiles_m, g.tiles_n, tm, tn);
    m0 = tm * BM;
    n0 = tn * BN;
  };
  auto dma_half = [&](int j) {  // this group's half of stage j
    const int ti = j / nk, kt = j - ti * nk;
    int m0, n0;
    tile_mn(ti, m0, n0);
    char* base = smem + (j & 1) * STAGE_BYTES + gw * 1024;
    if (grp == 0) {
      const int sa = m0 * K2 + kt * ROWB;
#pragma unroll
      for (int i = 0; i < A_LD; ++i)
        ring_glds16(ra, base + i * 4096, m0 + d_row[i] < g.M ? d_row[i] * K2 + d_col[i] : OOB, sa);
    } else {
      const int sb = n0 * K2 + kt * ROWB;
#pragma unroll
      for (int i = 0; i < B_LD; ++i)
        ring_glds16(rw, base + A_BYTES + i * 4096, n0 + d_row[i] < g.N ? d_row[i] * K2 + d_col[i] : OOB, sb);
    }
  };
  (void)nld;

  f32x4 acc[MT][NTL];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NTL; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4, sw = ring_swz<128>(fr);
  const int a_rd = (wm * WTM + fr) * ROWB, w_rd = A_BYTES + (wn * WTN + fr) * ROWB;


  // prologue: stage 0 (both halves), group 1's half of stage 1; stage 0 visible to all
  if (nsteps > 0) dma_half(0);
  if (grp == 1 && nsteps > 1) dma_half(1);
  if (grp == 0) ring_wait_vmcnt<0>();
  else if (nsteps > 1) ring_wait_vmcnt<B_LD>();
  else ring_wait_vmcnt<0>();
  ring_barrier();
  if (grp == 1) ring_barrier();  // the stagger

  bf16x8 af[2][MT], wf[2][NTL];
  for (int j = 0; j < nsteps; ++j) {
    // ---- L section: DMA (group 0: A of stage j + 1) + all fragment reads of stage j ----
    if (grp == 0 && j + 1 < nsteps) dma_half(j + 1);
    const char* base = smem + (j & 1) * STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int coff = ((ks * 4 + fq) ^ sw) << 4;
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn) wf[ks][jn] = *reinterpret_cast<const bf16x8*>(base + w_rd + jn * 2048 + coff);
#pragma unroll
      for (int i = 0; i < MT; ++i) af[ks][i] = *reinterpret_cast<const bf16x8*>(base + a_rd + i * 2048 + coff);
    }
    if (grp == 1) ring_wait_vmcnt<0>();  // group 1's W half of stage j + 1 (issued in its last M section)
    ring_barrier();
    // ---- M section: group 1 issues its W half of stage j + 2, then every MFMA of step j ----
    if (grp == 1 && j + 2 < nsteps) dma_half(j + 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int jn = 0; jn < NTL; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][jn], af[ks][i], acc[i][jn], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    if (j % nk == nk - 1) {
      int m0, n0;
      tile_mn(j / nk, m0, n0);
      gt_epilogue<MT, NTL>(acc, g, m0, n0, wm * WTM, wn * WTN);
    }
    if (grp == 0) ring_wait_vmcnt<0>();  // group 0's A half of stage j + 1
    ring_barrier();
  }
  if (grp == 0) ring_barrier();  // balance group 1's stagger barrier
}

// ---------------------------------------------------------------------------------------------
// Ring variant (cfg 10-12): the ping-pong stagger of gemm_pp_kernel on a DEEP LDS-DMA ring.
//
// Measured on the kernels above (profiles/r3_gemm_tile_probe_*.jsonl): the 2-stage 256 x 256 loop
// runs at ~48 % of MFMA peak on 8192^3 -- the DMA of step j + 1 has one k-step (~0.85 us of MFMA)
// to land, less than a loaded L2-miss round trip -- and the ping-pong kernel, whose DMA had even
// less lead, was slower still.  This kernel keeps the stagger (one wave per SIMD in its MFMA section
// while the other reads fragments, so barriers never empty the MFMA pipe) and gives every DMA
// R - 1 sub-steps of lead:
//  * sub-step = 32 of K: one 16x16x32 MFMA per (i, jn) per wave (32 per wave on the 256^2 tile);
//    ring slot = A[BM][32] + W[BN][32] (24-32 KB, 64-B rows), R slots (160 KB for 256^2 x 5);
//  * group 0 = waves 0-3, group 1 = waves 4-7 (one of each per SIMD); group 1 runs one barrier
//    behind.  Barrier interval 2u: G0 reads slot u (L section) while G1 multiplies u - 1 (M
//    section); interval 2u + 1: G0 multiplies u, G1 reads u;
//  * G0 DMAs the A half of sub-step u + R - 1 in its L section of u, G1 the W half of u + R in its M
//    section of u -- both into slot (u - 1) % R / u % R, free since the barrier that closed the
//    last read of it; each wave retires its half of sub-step u + 1 (counted vmcnt, never 0 in steady
//    state) before the barrier that precedes the first read of it, so a DMA has ~2(R - 2) barrier
//    intervals of lead instead of 2;
//  * epilogue bias through the scalar cache (constant address space, uniform per wave): a vector
//    load there would make hipcc drain the whole DMA ring with vmcnt(0) at every tile end.
template <int L, int MAXN>
MLS_DEV void gt_wait_groups(int n) {  // wait until <= L * min(n, MAXN) of this wave's loads are in flight
  if constexpr (MAXN == 0) {
    ring_wait_vmcnt<0>();
  } else {
    if (n >= MAXN) ring_wait_vmcnt<L * MAXN>();
    else gt_wait_groups<L, MAXN - 1>(n);
  }
}

template <int BM, int BN, int WM, int WN, int R>
__global__ __launch_bounds__(512) void gemm_ring_kernel(const GemmTileArgs g) {
  static_assert(WM * WN == 8, "8 waves");
  constexpr int WTM = BM / WM, WTN = BN / WN, MT = WTM / 16, NTL = WTN / 16;
  constexpr int ROWB = 64;  // 32 k of bf16
  constexpr int A_BYTES = BM * ROWB, SLOT = (BM + BN) * ROWB;
  constexpr int LA = A_BYTES / (256 * 16), LB = BN * ROWB / (256 * 16);  // DMAs per thread per half
  static_assert(LA * 256 * 16 == A_BYTES && LB * 256 * 16 == BN * ROWB, "whole DMA rounds per group");
  static_assert(R * SLOT <= 160 * 1024 && R >= 3, "ring");
  static_assert(WTN == 64 || WTN == 32, "bias slice");
  __shared__ __attribute__((aligned(16))) char smem[R * SLOT];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int grp = __builtin_amdgcn_readfirstlane(wid >> 2), gt = tid & 255, gw = wid & 3;
  const int wm = wid / WN, wn = wid - wm * WN;
  const int tiles_m = (g.M + BM - 1) / BM, ntiles = tiles_m * g.tiles_n;
  const int G = gridDim.x, bq = xcd_remap(blockIdx.x, G);
  const int my_tiles = bq < ntiles ? (ntiles - 1 - bq) / G + 1 : 0;
  const int nk = g.K / 32, nsub = my_tiles * nk;
  const rsrc_t ra = make_rsrc(g.a, g.a_bytes), rw = make_rsrc(g.w, g.w_bytes);
  const int K2 = g.K * 2;

  auto tile_mn = [&](int ti, int& m0, int& n0) {
    int tm, tn;
    ring_tile(bq + ti * G, tiles_m, g.tiles_n, tm, tn);
    m0 = tm * BM;
    n0 = tn * BN;
  };
  // this thread's DMA pieces (group 0: A rows, group 1: W rows): LDS byte i*4096 + gt*16 of the
  // half = row (i*4096 + gt*16) / 64, lane-linear chunk gt & 3 = source chunk (gt & 3) ^ swz(row)
  constexpr int LD = LA > LB ? LA : LB;
  int d_off[LD];
  const int lim = grp == 0 ? g.M : g.N;
#pragma unroll
  for (int i = 0; i < LD; ++i) {
    const int row = i * 64 + (gt >> 2);
    d_off[i] = row * K2 + (((gt & 3) ^ ring_swz<64>(row)) << 4);
  }
  // loader cursor of this group (its half of sub-step l_u goes to slot l_u % R)
  int l_u = 0, l_kt = 0, l_ti = 0, l_m0 = 0, l_n0 = 0, l_slot = 0;
  tile_mn(0, l_m0, l_n0);
  auto issue = [&]() {
    char* base = smem + l_slot * SLOT + gw * 1024;
    if (grp == 0) {
      const int so = l_m0 * K2 + l_kt * ROWB;
#pragma unroll
      for (int i = 0; i < LA; ++i)
        ring_glds16(ra, base + i * 4096, l_m0 + i * 64 + (gt >> 2) < lim ? d_off[i] : OOB, so);
    } else {
      const int so = l_n0 * K2 + l_kt * ROWB;
#pragma unroll
      for (int i = 0; i < LB; ++i)
        ring_glds16(rw, base + A_BYTES + i * 4096, l_n0 + i * 64 + (gt >> 2) < lim ? d_off[i] : OOB, so);
    }
    ++l_u;
    l_slot = l_slot + 1 == R ? 0 : l_slot + 1;
    if (++l_kt == nk) {
      l_kt = 0;
      if (++l_ti < my_tiles) tile_mn(l_ti, l_m0, l_n0);
    }
  };

  f32x4 acc[MT][NTL];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NTL; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  const int coff = (fq ^ ring_swz<64>(fr)) << 4;
  const int a_rd = (wm * WTM + fr) * ROWB + coff, w_rd = A_BYTES + (wn * WTN + fr) * ROWB + coff;


  // prologue: G0 A halves of 0 .. R-2, G1 W halves of 0 .. R-1; sub-step 0 retired; G1 staggers
  {
    const int n_pro = grp == 0 ? R - 1 : R;
    for (int u = 0; u < n_pro && u < nsub; ++u) issue();
    const int after = l_u - 1;  // loads issued after sub-step 0's
    if (grp == 0) gt_wait_groups<LA, R - 2>(after);
    else gt_wait_groups<LB, R - 1>(after);
  }
  ring_barrier();
  if (grp == 1) ring_barrier();

  int c_slot = 0, c_kt = 0, c_ti = 0;
  bf16x8 af[MT], wf[NTL];
  for (int u = 0; u < nsub; ++u) {
    // ---- L section ----
    if (grp == 0 && l_u < nsub) issue();  // A half of u + R - 1
    {
      const char* base = smem + c_slot * SLOT;
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn) wf[jn] = *reinterpret_cast<const bf16x8*>(base + w_rd + jn * 16 * ROWB);
#pragma unroll
      for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const bf16x8*>(base + a_rd + i * 16 * ROWB);
    }
    c_slot = c_slot + 1 == R ? 0 : c_slot + 1;
    if (grp == 1 && u + 1 < nsub) gt_wait_groups<LB, R - 2>(l_u - 1 - (u + 1));  // W half of u + 1 retired
    ring_barrier();
    // ---- M section ----
    if (grp == 1 && l_u < nsub) issue();  // W half of u + R
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn)
        acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[jn], af[i], acc[i][jn], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    if (++c_kt == nk) {
      c_kt = 0;
      int m0, n0;
      tile_mn(c_ti++, m0, n0);
      gt_epilogue<MT, NTL>(acc, g, m0, n0, wm * WTM, wn * WTN);
    }
    if (grp == 0 && u + 1 < nsub) gt_wait_groups<LA, R - 2>(l_u - 1 - (u + 1));  // A half of u + 1 retired
    ring_barrier();
  }
  if (grp == 0) ring_barrier();  // balance group 1's stagger barrier
}

struct GtCfg {
  int bm, bn, threads;
};

// cfg ids (ops.GEMM_TILE_CFGS), tile / waves / ring (stages x K depth) / LDS:
//   1: 256x256, 8 waves 2x4, 2 x 64, 128 KB      6: 256x256, 8 waves 2x4, 4 x 32, 128 KB
//   2: 256x128, 8 waves 4x2, 3 x 64, 144 KB      7: 256x128, 8 waves 4x2, 4 x 32,  96 KB
//   3: 128x128, 4 waves 2x2, 2 x 64,  64 KB (2 blocks / CU)
//   4: 128x128, 4 waves 2x2, 3 x 64,  96 KB      5: 128x256, 8 waves 2x4, 3 x 64, 144 KB
//   8: 256x256 ping-pong (gemm_pp_kernel), 2 x 64, 128 KB    9: 256x128 ping-pong, 2 x 64, 96 KB
//  10: 256x256 ring (gemm_ring_kernel), 5 x 32, 160 KB      11: 256x256 ring, 4 x 32, 128 KB
//  12: 256x128 ring, 6 x 32, 144 KB
//  21: 192x192, 8 waves 4x2, 3 x 64, 144 KB (a 3-deep ring at ~the 256^2 tile's reuse)   22: + PIPE
//  (a 4-wave 256x256 tile -- one wave per SIMD, 128x128 wave tile, 256 accumulators -- spills
//   101-138 VGPRs in the k-loop under hipcc 7.2; not kept: docs/PERF_NOTES.md Round 4)
GtCfg gt_cfg(int cfg) {
  switch (cfg) {
    case 1: return {256, 256, 512};
    case 2: return {256, 128, 512};
    case 3: return {128, 128, 256};
    case 4: return {128, 128, 256};
    case 5: return {128, 256, 512};
    case 6: return {256, 256, 512};
    case 7: return {256, 128, 512};
    case 8: return {256, 256, 512};
    case 9: return {256, 128, 512};
    case 10: return {256, 256, 512};
    case 11: return {256, 256, 512};
    case 12: return {256, 128, 512};
    case 13: return {256, 256, 512};
    case 14: return {256, 128, 512};
    case 15: return {256, 256, 512};
    case 16: return {256, 128, 512};
    case 17: return {256, 256, 512};
    case 18: return {256, 128, 512};
    case 19: return {256, 256, 512};
    case 20: return {256, 256, 512};
    case 21: return {192, 192, 512};
    case 22: return {192, 192, 512};
    default: return {0, 0, 0};
  }
}

int gt_launch(const GemmTileArgs& g0, int cfg, int grid_cap, hipStream_t st) {
  const GtCfg c = gt_cfg(cfg);
  if (!c.bm) return MLS_BAD_ARG;
  GemmTileArgs g = g0;
  const int tiles_m = (g.M + c.bm - 1) / c.bm;
  g.tiles_n = (g.N + c.bn - 1) / c.bn;
  // one resident wave of blocks (cfg 3 fits 2 per CU)
  const int per_cu = cfg == 3 ? 2 : 1;
  int cap = grid_cap > 0 ? grid_cap : mls_num_cus() * per_cu;
  const int ntiles = tiles_m * g.tiles_n;
  // split-K (validated by mls_gemm_tile): tile-kernel cfgs only
  const bool sk_ok = cfg <= 7 || cfg >= 13;
  if (g.splitk < 1) g.splitk = 1;
  if (g.splitk > 1 && !sk_ok) return MLS_BAD_ARG;
  const dim3 grid = ring_grid(ntiles * g.splitk, cap), block(c.threads);
  if (g.fold_c || g.ln_part || g.stats_part) {  // LayerNorm folding (mls_gemm_tile_ln maps the cfg)
#define GT_LN_LAUNCH(K)                                                                                              \
  switch (cfg) {                                                                                                     \
    case 15: hipLaunchKernelGGL((gemm_tile_kernel<256, 256, 2, 4, 2, 64, false, true, false, K>), grid, block, 0, st, g); break; \
    case 16: hipLaunchKernelGGL((gemm_tile_kernel<256, 128, 4, 2, 3, 64, false, true, false, K>), grid, block, 0, st, g); break; \
    case 5: hipLaunchKernelGGL((gemm_tile_kernel<128, 256, 2, 4, 3, 64, false, false, false, K>), grid, block, 0, st, g); break; \
    case 4: hipLaunchKernelGGL((gemm_tile_kernel<128, 128, 2, 2, 3, 64, false, false, false, K>), grid, block, 0, st, g); break; \
    default: return MLS_BAD_ARG;                                                                                     \
  }
    if (g.fold_c) {
      GT_LN_LAUNCH(1)
    } else {
      GT_LN_LAUNCH(2)
    }
#undef GT_LN_LAUNCH
    return hipGetLastError() == hipSuccess ? MLS_OK : MLS_BAD_ARG;
  }
  switch (cfg) {
    case 1: hipLaunchKernelGGL((gemm_tile_kernel<256, 256, 2, 4, 2, 64>), grid, block, 0, st, g); break;
    case 2: hipLaunchKernelGGL((gemm_tile_kernel<256, 128, 4, 2, 3, 64>), grid, block, 0, st, g); break;
    case 3: hipLaunchKernelGGL((gemm_tile_kernel<128, 128, 2, 2, 2, 64>), grid, block, 0, st, g); break;
    case 4: hipLaunchKernelGGL((gemm_tile_kernel<128, 128, 2, 2, 3, 64>), grid, block, 0, st, g); break;
    case 5: hipLaunchKernelGGL((gemm_tile_kernel<128, 256, 2, 4, 3, 64>), grid, block, 0, st, g); break;
    case 6: hipLaunchKernelGGL((gemm_tile_kernel<256, 256, 2, 4, 4, 32>), grid, block, 0, st, g); break;
    case 7: hipLaunchKernelGGL((gemm_tile_kernel<256, 128, 4, 2, 4, 32>), grid, block, 0, st, g); break;
    case 8: hipLaunchKernelGGL((gemm_pp_kernel<256, 256, 2, 4>), grid, block, 0, st, g); break;
    case 9: hipLaunchKernelGGL((gemm_pp_kernel<256, 128, 4, 2>), grid, block, 0, st, g); break;
    case 10: hipLaunchKernelGGL((gemm_ring_kernel<256, 256, 2, 4, 5>), grid, block, 0, st, g); break;
    case 11: hipLaunchKernelGGL((gemm_ring_kernel<256, 256, 2, 4, 4>), grid, block, 0, st, g); break;
    case 12: hipLaunchKernelGGL((gemm_ring_kernel<256, 128, 4, 2, 6>), grid, block, 0, st, g); break;
    case 13: hipLaunchKernelGGL((gemm_tile_kernel<256, 256, 2, 4, 2, 64, true>), grid, block, 0, st, g); break;
    case 14: hipLaunchKernelGGL((gemm_tile_kernel<256, 128, 4, 2, 3, 64, true>), grid, block, 0, st, g); break;
    case 15: hipLaunchKernelGGL((gemm_tile_kernel<256, 256, 2, 4, 2, 64, false, true>), grid, block, 0, st, g); break;
    case 16: hipLaunchKernelGGL((gemm_tile_kernel<256, 128, 4, 2, 3, 64, false, true>), grid, block, 0, st, g); break;
    case 17: hipLaunchKernelGGL((gemm_tile_kernel<256, 256, 2, 4, 2, 64, true, true>), grid, block, 0, st, g); break;
    case 18: hipLaunchKernelGGL((gemm_tile_kernel<256, 128, 4, 2, 3, 64, true, true>), grid, block, 0, st, g); break;
    case 19: hipLaunchKernelGGL((gemm_tile_kernel<256, 256, 2, 4, 2, 64, false, false, true>), grid, block, 0, st, g); break;
    case 20: hipLaunchKernelGGL((gemm_tile_kernel<256, 256, 2, 4, 2, 64, true, false, true>), grid, block, 0, st, g); break;
    case 21: hipLaunchKernelGGL((gemm_tile_kernel<192, 192, 4, 2, 3, 64>), grid, block, 0, st, g); break;
    case 22: hipLaunchKernelGGL((gemm_tile_kernel<192, 192, 4, 2, 3, 64, false, true>), grid, block, 0, st, g); break;
  }
  return hipGetLastError() == hipSuccess ? MLS_OK : MLS_BAD_ARG;
}

// default tile by shape: the largest tile that still gives the chip >= ~1 block per CU, else the
// one with the most blocks (the projection GEMMs run under 4-5-way stream concurrency in serving)
int gt_pick(int M, int N) {
  auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
  if (blocks(256, 256) >= 256) return 15;  // cfg 1 + fragment pipeline (>= cfg 1 on every probed shape)
  if (blocks(256, 128) >= 256) return 16;
  if (blocks(128, 256) >= 256) return 5;
  return 4;
}

}  // namespace

extern "C" {

// out[M][N] = act(A[M][K] . W[N][K]^T + bias (+ res));  ACT_SILU_MUL: W rows gate/up interleaved in
// groups of 8, out [M][N/2].  K % 64 == 0, N % 16 == 0; cfg 0 = pick by shape; grid_cap 0 = one
// resident wave of persistent blocks.  splitk > 1: K in that many whole-k-step splits combined in
// the launch -- ws >= tiles * splitk * BM * BN fp32, cnt >= tiles int32, all ZERO before the first
// launch (each tile's reducer resets its counter).
int mls_gemm_tile(const void* A, const void* W, const float* bias, const void* res, void* out, int M, int N, int K,
                  int act, int ldo, int ldr, int cfg, int grid_cap, int splitk, void* ws, long long ws_elems,
                  void* cnt, int cnt_elems, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 16 || (res && act == ACT_SILU_MUL)) return MLS_BAD_ARG;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K * 2;
  if (ab >= 0x7FFFFFFFull || wb >= 0x7FFFFFFFull || (size_t)M * ldo >= 0x7FFFFFFFFFull) return MLS_UNSUPPORTED;
  GemmTileArgs g{};
  g.flags = cfg >> 8;
  cfg &= 0xFF;
  g.a = (const bf16*)A;
  g.w = (const bf16*)W;
  g.bias = bias;
  g.res = (const bf16*)res;
  g.out = (bf16*)out;
  g.M = M; g.N = N; g.K = K; g.act = act;
  g.ldo = ldo > 0 ? ldo : (act == ACT_SILU_MUL ? N / 2 : N);
  g.ldr = ldr > 0 ? ldr : N;
  g.a_bytes = g.flags & GT_ABL_NOLOAD ? 0u : (uint32_t)ab;
  g.w_bytes = g.flags & GT_ABL_NOLOAD ? 0u : (uint32_t)wb;
  const int c = cfg > 0 ? cfg : gt_pick(M, N);
  g.splitk = splitk > 1 ? splitk : 1;
  if (g.splitk > 1) {
    const GtCfg t = gt_cfg(c);
    if (!t.bm) return MLS_BAD_ARG;
    const long long tiles = (long long)((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
    const int bks = c == 6 || c == 7 ? 32 : 64;
    if (!ring_splitk_ok(g.splitk, K / bks, tiles, (long long)t.bm * t.bn, ws, ws_elems, cnt, cnt_elems))
      return MLS_BAD_ARG;
    g.ws = (float*)ws;
    g.cnt = (int*)cnt;
  }
  return gt_launch(g, c, grid_cap, (hipStream_t)stream);
}

int mls_gemm_tile_pick(int M, int N) { return gt_pick(M, N); }

// LayerNorm-folding forms of mls_gemm_tile (module comment "LayerNorm folding"; no split-K, ldo = ldr = N).
// Row statistics travel as [M][width / 128][2] partials (sum, sum of squares) written by a PART launch.
//  * fold_c != null: A = the raw pre-LN rows, W = W . diag(gamma), bias = b + W . beta (ops.fold_layernorm);
//    out = act(rstd * (A . W^T - mu * fold_c) + bias), A-row statistics from ln_part (K / 128 partials).
//    act: none / gelu;
//  * res != null: out = A . W^T + bias + res', res' = res, or (res - mu) * rstd * ln_g with ln_part (N / 128
//    partials) given -- the LN's beta must be folded into bias; stats_part != null: also write the OUTPUT
//    rows' partials there
//    ([M][N / 128][2]: >= M * N / 64 floats in total; N % 128 == 0).
// The LN'd widths must be multiples of 256 and at most 1024.  cfg: 0 = by shape; the folding kernels
// are the 256 x 256 / 256 x 128 PIPE tiles (15 / 16) and the 128 x 256 / 128 x 128 tiles (5 / 4).
int mls_gemm_tile_ln(const void* A, const void* W, const float* bias, const void* res, void* out, int M, int N,
                     int K, int act, int cfg, const float* fold_c, const float* ln_part, const float* ln_g,
                     float* stats_part, long long part_elems, float eps, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 16) return MLS_BAD_ARG;
  // the LN'd rows' partials are read two per lane with 16-B loads (ring_row_stats_issue): their width
  // must be a multiple of 256 (an even partial count) and at most 1024
  if (fold_c && (res || !ln_part || stats_part || (act != ACT_NONE && act != ACT_GELU) || K % 256 || K > 1024))
    return MLS_BAD_ARG;
  if (!fold_c && (!res || act != ACT_NONE)) return MLS_BAD_ARG;
  if (ln_part && !fold_c && (!ln_g || N % 256 || N > 1024)) return MLS_BAD_ARG;
  if (stats_part && (N % 128 || (long long)M * (N / 128) * 2 > part_elems)) return MLS_BAD_ARG;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K * 2;
  if (ab >= 0x7FFFFFFFull || wb >= 0x7FFFFFFFull || (size_t)M * N >= 0x3FFFFFFFull) return MLS_UNSUPPORTED;
  int c = (cfg & 0xFF) > 0 ? (cfg & 0xFF) : gt_pick(M, N);
  switch (c) {
    case 15: case 16: case 5: case 4: break;
    case 3: c = 4; break;
    default: c = gt_cfg(c).bn == 128 ? 16 : 15; break;
  }
  GemmTileArgs g{};
  g.a = (const bf16*)A;
  g.w = (const bf16*)W;
  g.bias = bias;
  g.res = (const bf16*)res;
  g.out = (bf16*)out;
  g.M = M; g.N = N; g.K = K; g.act = act;
  g.ldo = N;
  g.ldr = N;
  g.a_bytes = (uint32_t)ab;
  g.w_bytes = (uint32_t)wb;
  g.splitk = 1;
  g.fold_c = fold_c;
  g.ln_part = ln_part;
  g.ln_g = ln_g;
  g.stats_part = stats_part;
  g.eps = eps;
  return gt_launch(g, c, 0, (hipStream_t)stream);
}

}  // extern "C"
