// FP8 (OCP e4m3) W8A8 projection GEMM on the gfx950 block-scaled MFMA, and the activation-row quantiser
// that feeds it:
//     out[M][N] = act((Aq[M][K] . Wq[N][K]^T) * xs[m] * ws[n] + bias[N]) (+ residual[M][N])
// Aq / Wq are e4m3 codes, xs one fp32 scale per activation row (dynamic, mls_quant_rows_fp8), ws one per
// output channel (ops.pack_w8).  The rule of both quantisers is ops/reference.py kv_quant_fp8's:
// scale = max(max|row|, 2^-40) / 448, q = e4m3fn_rne(row * (1 / scale)).
//
// Arithmetic: v_mfma_scale_f32_16x16x128_f8f6f4 with both formats e4m3 (cbsz = blgp = 0) and every E8M0
// block scale 127 = 2^0 -- the only fp8 MFMA that runs at twice the bf16 rate; the non-scaled _fp8_fp8
// forms run at the bf16 rate.  Every e4m3 x e4m3 product is exact in fp32, xs[m] * ws[n] multiplies the
// fp32 accumulator in the epilogue.
//
// Structure: gemm_ring.h's persistent LDS-DMA ring, split-K combine and tile epilogue (its SCALED form), one
// byte per element instead of two --
//  * a k-step is 128 k = one 128-B LDS row per tile row, so the LDS image, the LDS-DMA and the ds_read_b128
//    lane pattern are exactly the bf16 kernel's BK = 64 ones (conflict-free for the same reason);
//  * a lane's 32-byte operand (fr = lane & 15 the tile row, fq = lane >> 4 the k group) is two 16-B reads:
//    k = 16 fq .. + 16 and k = 64 + 16 fq .. + 16 of the step.  The instruction pairs byte b of k group fq
//    of its A operand with byte b of k group fq of its B operand, and both operands are read the same way,
//    so every k of the step meets its partner once whatever order the hardware sums them in
//    (tests/test_w8a8_gpu.py checks the map with exact one-hot rows);
//  * at twice the MFMA rate and half the operand bytes per k the LDS read rate per clock equals the bf16
//    kernel's at the same register tiling (32 B per lane per 16x16x128 step against 16 B per 16x16x32);
//  * the short-M configurations split K so the weights stream once over the chip.
#include "gemm_ring.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr float W8_FP8_MAX = 448.f;
constexpr float W8_AMAX_FLOOR = 9.094947017729282e-13f;  // 2^-40
constexpr int W8_ROWB = 128;                             // bytes (= k values) of one k-step row
constexpr int W8_E8M0_ONE = 0x7F7F7F7F;                  // block scale 2^0 in every byte

struct W8Args {
  const uint8_t* a;   // [M][K] e4m3
  const uint8_t* w;   // [N][K] e4m3
  const float* xs;    // [M]
  const float* wsc;   // [N]
  const float* bias;  // [N] or nullptr
  const bf16* res;    // [M][N] or nullptr
  bf16* out;          // [M][ldo]
  int M, N, K, act, ldo;
  uint32_t a_bytes, w_bytes;
  int tiles_n;
  int splitk;  // K splits per output tile (>= 1)
  float* ws;   // [tiles][splitk][BM * BN] fp32 partial tiles (fragment-linear)
  int* cnt;    // [tiles] arrival counters: zero before the launch, reset by each tile's reducer
  static constexpr bool SCALED = true;  // ring_epilogue_t: fma(acc, xs[m] * wsc[n], bias)
  static constexpr int flags = 0;       // no ablation builds: the epilogue's flag tests fold away
  MLS_DEV int res_pitch() const { return N; }
};

// EPI of ring_epilogue_t: 0 plain (+ bias), 1 + residual, 2 SiLU-mul
template <int MT, int NTL>
MLS_DEV void w8_epilogue(f32x4 (&acc)[MT][NTL], const W8Args& g, int m0, int n0, int wrow, int wcol) {
  if (g.act == ACT_SILU_MUL) ring_epilogue_t<MT, NTL, 2, ACT_NONE>(acc, g, m0, n0, wrow, wcol);
  else if (g.res) ring_epilogue_t<MT, NTL, 1, ACT_NONE>(acc, g, m0, n0, wrow, wcol);
  else ring_epilogue_t<MT, NTL, 0, ACT_NONE>(acc, g, m0, n0, wrow, wcol);
  ring_epilogue_done(acc);
}

MLS_DEV i32x8 w8_frag(const char* p0, const char* p1) {
  const i32x4 lo = *reinterpret_cast<const i32x4*>(p0), hi = *reinterpret_cast<const i32x4*>(p1);
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int BM, int BN, int WM, int WN, int STAGES>
__global__ __launch_bounds__(WM * WN * 64) void gemm_w8a8_kernel(const W8Args g) {
  constexpr int NT = WM * WN * 64;
  constexpr int WTM = BM / WM, WTN = BN / WN;  // wave tile: WTM rows (m) x WTN columns (n)
  constexpr int MT = WTM / 16, NTL = WTN / 16;
  constexpr int ROWB = W8_ROWB, CPR = ROWB / 16;  // bytes / 16-B chunks per LDS row
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int A_LD = A_BYTES / (NT * 16), B_LD = B_BYTES / (NT * 16), LOADS = A_LD + B_LD;
  static_assert(A_BYTES % (NT * 16) == 0 && B_BYTES % (NT * 16) == 0, "stage must split into whole DMA rounds");
  static_assert(A_LD >= 1 && BM <= 256 && WTM % 16 == 0 && WTN % 32 == 0, "tile shape");
  // + 16 B: the split-K "last arriver" flag, in the same __shared__ object as the ring
  static_assert(STAGES * STAGE_BYTES + 16 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[STAGES * STAGE_BYTES + 16];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid - wm * WN;
  const int tiles_m = (g.M + BM - 1) / BM, ntiles = tiles_m * g.tiles_n;
  // work unit = (tile, K split); persistent: block b takes units b', b' + G, ... (b' = XCD-contiguous b)
  const int S = g.splitk, nunits = ntiles * S;
  const int G = gridDim.x, bq = xcd_remap(blockIdx.x, G);
  const int my_tiles = bq < nunits ? (nunits - 1 - bq) / G + 1 : 0;
  const int nk = g.K / ROWB / S, nsteps = my_tiles * nk;

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
  const int K1 = g.K;  // bytes per source row

  auto tile_mn = [&](int ti, int& m0, int& n0, int& k0) {
    const int u = bq + ti * G, t = S == 1 ? u : u / S;
    int tm, tn;
    ring_tile(t, tiles_m, g.tiles_n, tm, tn);
    m0 = tm * BM;
    n0 = tn * BN;
    k0 = (u - t * S) * nk;
  };
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
    const int sa = m0 * K1 + kt * ROWB, sb = n0 * K1 + kt * ROWB;
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      ring_glds16(ra, base + i * NT * 16, m0 + a_row[i] < g.M ? a_row[i] * K1 + a_col[i] : OOB, sa);
#pragma unroll
    for (int i = 0; i < B_LD; ++i)
      ring_glds16(rw, base + A_BYTES + i * NT * 16, n0 + w_row[i] < g.N ? w_row[i] * K1 + w_col[i] : OOB, sb);
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
  const int coff0 = (fq ^ sw) << 4, coff1 = ((4 + fq) ^ sw) << 4;

#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nsteps) stage();

  int c_kt = 0, c_ti = 0, c_slot = 0;  // compute cursor
  for (int j = 0; j < nsteps; ++j) {
    ring_wait<STAGES, LOADS>(nsteps - 1 - j);  // step j landed; later ones may still fly
    ring_barrier();  // step j visible to every wave; step j - 1 fully read by every wave
    if (j + STAGES - 1 < nsteps) stage();
    const char* base = smem + c_slot * STAGE_BYTES;
    c_slot = c_slot + 1 == STAGES ? 0 : c_slot + 1;
    i32x8 wf[NTL];
#pragma unroll
    for (int jn = 0; jn < NTL; ++jn)
      wf[jn] = w8_frag(base + w_rd + jn * 16 * ROWB + coff0, base + w_rd + jn * 16 * ROWB + coff1);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const i32x8 af = w8_frag(base + a_rd + i * 16 * ROWB + coff0, base + a_rd + i * 16 * ROWB + coff1);
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn)
        acc[i][jn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[jn], af, acc[i][jn], 0, 0, 0, W8_E8M0_ONE,
                                                                      0, W8_E8M0_ONE);
    }
    __builtin_amdgcn_s_setprio(0);
    if (++c_kt < nk) continue;
    c_kt = 0;

    // ---- epilogue of this unit (the next unit's first k-steps are already in flight) ----
    int m0, n0, k0;
    const int cu = bq + c_ti * G;
    tile_mn(c_ti++, m0, n0, k0);
    const bool reducer = S == 1 || ring_splitk_arrive<BM * BN, MT, NTL>(acc, g.ws, g.cnt, S, cu / S, cu - (cu / S) * S,
                                                                        (int*)(smem + STAGES * STAGE_BYTES));
    if (reducer) w8_epilogue<MT, NTL>(acc, g, m0, n0, wm * WTM, wn * WTN);
  }
}

// variant ids (ops.W8A8_CFGS), tile / waves / ring / LDS:
//   1: 256x256, 8 waves 2x4, 2 stages, 128 KB   (prefill)
//   2: 256x128, 8 waves 4x2, 3 stages, 144 KB
//   3: 128x128, 4 waves 2x2, 3 stages,  96 KB
//   4:  64x128, 4 waves 1x4, 4 stages,  96 KB   (decode-shaped: split-K)
//   5:  32x128, 4 waves 1x4, 4 stages,  80 KB   (decode-shaped: split-K)
constexpr int W8_NUM_VARIANTS = 6;  // 0 = by shape
struct W8Cfg {
  int bm, bn, threads;
};
W8Cfg w8_cfg(int v) {
  switch (v) {
    case 1: return {256, 256, 512};
    case 2: return {256, 128, 512};
    case 3: return {128, 128, 256};
    case 4: return {64, 128, 256};
    case 5: return {32, 128, 256};
    default: return {0, 0, 0};
  }
}

// by shape: the short-M tiles up to 64 rows, then the largest tile that still gives >= ~1 block per CU
int w8_pick(int M, int N) {
  auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
  if (M <= 32) return 5;
  if (M <= 64) return 4;
  const int cus = mls_num_cus();
  if (blocks(256, 256) >= cus) return 1;
  if (blocks(256, 128) >= cus) return 2;
  return 3;
}

// K splits: doubled while the units still fit one resident wave of blocks, every split keeps >= 2 whole
// k-steps, and the slabs fit the workspace
int w8_split(int tiles, int nk, long long tile_elems, long long ws_elems, int cnt_elems) {
  if (tiles > cnt_elems) return 1;
  const int cus = mls_num_cus();
  int s = 1;
  while (s < 16 && tiles * s * 2 <= cus && nk % (s * 2) == 0 && nk / (s * 2) >= 2 &&
         (long long)tiles * s * 2 * tile_elems <= ws_elems)
    s *= 2;
  return s;
}

// ---- activation rows -> e4m3 codes + one fp32 scale per row, one pass: a block per row keeps the row's
// bf16 values h = bf16(x + delta) in registers (written to resid_out when asked), reduces max|h| (and the
// square sum with `norm`), then writes q = e4m3(h * (1 / scale)) and scale (* rstd(h) with `norm`: a
// per-row dynamic scale absorbs the RMSNorm's per-row scalar, its gain is folded into the weights).
constexpr int QR_MAXC = 8;  // 16-B chunks per thread
__global__ __launch_bounds__(1024) void quant_rows_fp8_kernel(const bf16* __restrict__ x, const bf16* __restrict__ delta,
                                                              bf16* __restrict__ resid_out, uint8_t* __restrict__ q,
                                                              float* __restrict__ scale, int K, int norm, float eps) {
  __shared__ float red[32];
  const long row = blockIdx.x;
  const int nchunk = K >> 3, tid = threadIdx.x, nt = blockDim.x;
  const uint4* xr = reinterpret_cast<const uint4*>(x + row * K);
  const uint4* dr = delta ? reinterpret_cast<const uint4*>(delta + row * K) : nullptr;
  uint4 h[QR_MAXC];
  float amax = 0.f, ss = 0.f;
#pragma unroll
  for (int c = 0; c < QR_MAXC; ++c) {
    const int ch = c * nt + tid;
    h[c] = uint4{0, 0, 0, 0};
    if (ch < nchunk) {
      uint4 v = xr[ch];
      if (dr) {
        float a[8], b[8];
        unpack8(v, a);
        unpack8(dr[ch], b);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += b[e];
        v = pack8(a);
        if (resid_out) reinterpret_cast<uint4*>(resid_out + row * K)[ch] = v;
      }
      h[c] = v;
      float f[8];
      unpack8(v, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        amax = fmaxf(amax, fabsf(f[e]));
        ss = fmaf(f[e], f[e], ss);
      }
    }
  }
  amax = block_max(amax, red);
  float rstd = 1.f;
  if (norm) {
    ss = block_sum(ss, red + 16);
    rstd = rsqrtf(ss / (float)K + eps);
  }
  const float sc = fmaxf(amax, W8_AMAX_FLOOR) / W8_FP8_MAX;
  const float inv = 1.f / sc;
#pragma unroll
  for (int c = 0; c < QR_MAXC; ++c) {
    const int ch = c * nt + tid;
    if (ch < nchunk) {
      float f[8];
      unpack8(h[c], f);
      int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, 0, false);
      lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, lo, true);
      int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * inv, f[5] * inv, 0, false);
      hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * inv, f[7] * inv, hi, true);
      reinterpret_cast<int2*>(q + row * K)[ch] = int2{lo, hi};
    }
  }
  if (tid == 0) scale[row] = norm ? sc * rstd : sc;
}

}  // namespace

extern "C" {

int mls_gemm_w8a8_num_variants() { return W8_NUM_VARIANTS; }

// out[M][N] = act((Aq . Wq^T) * xs[m] * ws[n] + bias) (+ res); ACT_SILU_MUL: W rows gate / up interleaved in
// groups of 8, out [M][N/2].  K % 128 == 0, N % 16 == 0, any M >= 1.  variant 0: by shape.  splitk 0: the
// launcher's pick (needs ws / cnt: fp32 slabs and int32 arrival counters, the counters ZERO before the
// first launch; without them no split), > 0: that many.
int mls_gemm_w8a8(const void* Aq, const void* xs, const void* Wq, const void* wsc, const float* bias, const void* res,
                  void* out, int M, int N, int K, int act, int variant, int splitk, void* ws, long long ws_elems,
                  void* cnt, int cnt_elems, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 128 || N % 16 || variant < 0 || variant >= W8_NUM_VARIANTS) return MLS_BAD_ARG;
  if (act != ACT_NONE && act != ACT_SILU_MUL) return MLS_BAD_ARG;
  if (res && act == ACT_SILU_MUL) return MLS_BAD_ARG;
  const size_t ab = (size_t)M * K, wb = (size_t)N * K;
  // operand offsets are 32-bit (buffer voffset + soffset); the output / residual descriptors are per tile
  if (ab >= 0x7FFFFFFFull || wb >= 0x7FFFFFFFull) return MLS_UNSUPPORTED;
  const int v = variant > 0 ? variant : w8_pick(M, N);
  const W8Cfg c = w8_cfg(v);
  W8Args g{};
  g.a = (const uint8_t*)Aq;
  g.w = (const uint8_t*)Wq;
  g.xs = (const float*)xs;
  g.wsc = (const float*)wsc;
  g.bias = bias;
  g.res = (const bf16*)res;
  g.out = (bf16*)out;
  g.M = M; g.N = N; g.K = K; g.act = act;
  g.ldo = act == ACT_SILU_MUL ? N / 2 : N;
  g.a_bytes = (uint32_t)ab;
  g.w_bytes = (uint32_t)wb;
  const int tiles_m = (M + c.bm - 1) / c.bm;
  g.tiles_n = (N + c.bn - 1) / c.bn;
  const int tiles = tiles_m * g.tiles_n, nk = K / 128;
  const long long tile_elems = (long long)c.bm * c.bn;
  const bool have_ws = ws && cnt;
  if (splitk <= 0) {
    // by shape: the decode-shaped tiles and the 128 x 128 tile split K when their tiles leave CUs idle
    g.splitk = have_ws && v >= 3 ? w8_split(tiles, nk, tile_elems, ws_elems, cnt_elems) : 1;
  } else {
    g.splitk = splitk;
    if (splitk > 1 && !ring_splitk_ok(splitk, nk, tiles, tile_elems, ws, ws_elems, cnt, cnt_elems)) return MLS_BAD_ARG;
  }
  g.ws = (float*)ws;
  g.cnt = (int*)cnt;
  const dim3 grid = ring_grid(tiles * g.splitk, mls_num_cus()), block(c.threads);
  hipStream_t st = (hipStream_t)stream;
  switch (v) {
    case 1: hipLaunchKernelGGL((gemm_w8a8_kernel<256, 256, 2, 4, 2>), grid, block, 0, st, g); break;
    case 2: hipLaunchKernelGGL((gemm_w8a8_kernel<256, 128, 4, 2, 3>), grid, block, 0, st, g); break;
    case 3: hipLaunchKernelGGL((gemm_w8a8_kernel<128, 128, 2, 2, 3>), grid, block, 0, st, g); break;
    case 4: hipLaunchKernelGGL((gemm_w8a8_kernel<64, 128, 1, 4, 4>), grid, block, 0, st, g); break;
    case 5: hipLaunchKernelGGL((gemm_w8a8_kernel<32, 128, 1, 4, 4>), grid, block, 0, st, g); break;
  }
  return hipGetLastError() == hipSuccess ? MLS_OK : MLS_BAD_ARG;
}

// q[M][K] e4m3, scale[M] fp32 of h = bf16(x + delta) (delta optional; h also to resid_out when given);
// norm: scale[m] *= rsqrt(mean(h^2) + eps).  K % 8 == 0, K <= 65536.
int mls_quant_rows_fp8(const void* x, const void* delta, void* resid_out, void* q, void* scale, int M, int K, int norm,
                       float eps, void* stream) {
  if (M <= 0 || K <= 0 || K % 8 || (resid_out && !delta)) return MLS_BAD_ARG;
  const int nchunk = K / 8;
  if (nchunk > QR_MAXC * 1024) return MLS_UNSUPPORTED;
  int threads = 64;
  while (threads * QR_MAXC < nchunk) threads *= 2;
  if (threads < 256 && nchunk >= 256) threads = 256;
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3(M), dim3(threads), 0, (hipStream_t)stream, (const bf16*)x,
                     (const bf16*)delta, (bf16*)resid_out, (uint8_t*)q, (float*)scale, K, norm, eps);
  return hipGetLastError() == hipSuccess ? MLS_OK : MLS_BAD_ARG;
}

}  // extern "C"
