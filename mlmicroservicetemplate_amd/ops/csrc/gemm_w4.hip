// W4A16 tiled GEMM for every row count: out[M][N] = act(x[M][K] . dequant(W)[N][K]^T + bias) (+ residual), x bf16,
// W the (codes, scales) pair of ops.pack_skinny_w4 -- the layout csrc/skinny_w4.hip streams for <= 32 rows, so a
// model holds one copy for both kernels: 1 KiB granules [N/16][K/128][g][nr][kstep] of 4-bit codes q + 8 and bf16
// scales [N/16][K/128][16], one per (weight row, 128 k).
//
// How the work is split.  A block of four waves owns a BM x BN output tile (x one K split); BN = 4 waves x NTL
// 16-column weight tiles, and a wave computes ALL BM rows of its own NTL column tiles.  So
//  * weights never pass through LDS and are never read twice inside a block: a lane's non-temporal 16-B buffer
//    load of a granule is its MFMA fragments of four consecutive 32-wide k-steps of one 16-row weight tile (one
//    scale group), global -> VGPR in a STAGES-deep register ring beside the scales;
//  * activations are what the waves share: one k-step of the ring is a granule's worth of A, BM rows x 128 k, as
//    two BM x 128-B images (k 0..63, 64..127) written by LDS-DMA (ring_glds16, gemm_ring.h) with the 128-B row
//    swizzle on the source address, and read back as 16-B fragments, conflict-free, by every wave;
//  * one counted s_waitcnt vmcnt per step covers a stage's DMAs and weight loads alike (the counter retires in
//    order; every step issues the same LOADS, past the K range on the OOB offset, so the count is a constant), then
//    one ring_barrier -- no __syncthreads(), the loads of the next STAGES - 1 steps stay in flight across it;
//  * swapped product D = W_tile . A_tile^T as in gemm_tile.hip, so gemm_ring.h's epilogue (bias, residual, SiLU-mul,
//    16-B stores) and its in-launch split-K combine apply unchanged.  The granule's lane map (nr = weight row,
//    g = k group) is the MFMA's first-operand map, the LDS fragment (row fr, chunk fq) its second.
//
// Expansion, amortised over the BM / 16 row fragments an expanded fragment feeds:
//  * offset form (SC = false): ((word >> 4p) & 0x000F000F) | 0x43004300 = the bf16 pair 136 + q, 2 VALU ops per 2
//    weights; a row fragment's four k-steps accumulate on top of one MFMA chain against the constant -136 (shared
//    by the wave's NTL column tiles), and the group's scales fold it in: acc += s[n] * acc_group.  The accumulator
//    rows are n = 4 fq + e here, so a lane loads those four scales (8 B).  Costs MFMAs: + 1 / NTL.
//  * scaled form (SC = true): skinny_w4.hip's w4_expand_scaled, (q s) rounded to bf16, ~3.5 VALU ops per weight, no
//    extra MFMAs, no fold.  Per granule and column tile that is 112 VALU issues against 4 BM / 16 MFMAs of 16
//    cycles: hidden behind the matrix core from BM = 128 up, where the offset form's + 50 % MFMAs (NTL = 2) are
//    not.  Hence variants 1 (64 rows) offset, 2 (128) and 3 (256) scaled; 4 and 5 are the other form of 1 and 2,
//    kept for the A/B (docs/PERF_NOTES.md, "W4A16 at every row count": measured, 1 beats 4 and 5 beats 2 at every
//    shape, and the 64-row tile is never behind the larger ones -- see the pick in mls_gemm_w4a16).
//
// One unit (tile, split) per block, the splits of a tile adjacent (same XCD); split s takes the scale groups
// [G s / S, G (s + 1) / S), so K / 128 need not divide.  No data-dependent addressing: every offset is a function
// of the launch shape; rows past M and weight tiles past N read as zero through the range check, never stored.
#include "gemm_ring.h"

namespace {

struct W4GArgs {
  const bf16* a;      // [M][K]
  const uint8_t* w;   // granules, N K / 2 bytes
  const bf16* sc;     // [N/16][K/128][16]
  const float* bias;  // [N] or nullptr
  const bf16* res;    // [M][N] or nullptr
  bf16* out;          // [M][ldo]
  int M, N, K, act, ldo;
  uint32_t a_bytes, w_bytes, s_bytes;
  int tiles_n;
  int splitk;  // K splits per output tile (>= 1, <= K / 128)
  float* ws;   // [tiles][splitk][BM * BN] fp32 partial tiles (fragment-linear)
  int* cnt;    // [tiles] arrival counters: zero before the launch, reset by each tile's reducer
  static constexpr bool SCALED = false;  // ring_epilogue_t: acc + bias (the scales are applied in the k loop)
  static constexpr int flags = 0;
  MLS_DEV int res_pitch() const { return N; }
};

MLS_DEV float w4g_bf(uint32_t bits16) { return __builtin_bit_cast(float, bits16 << 16); }

// one k-step's word -> the fragment 136 + q (k order)
MLS_DEV bf16x8 w4g_expand(uint32_t w) {
  constexpr uint32_t m = 0x000F000Fu, b = 0x43004300u;
  return __builtin_bit_cast(bf16x8, make_uint4((w & m) | b, ((w >> 4) & m) | b, ((w >> 8) & m) | b, ((w >> 12) & m) | b));
}
// ... -> the fragment bf16(q s): (0x4300 | nib) << 16 is the fp32 128 + nib, one FMA gives (nib - 8) s exactly
MLS_DEV bf16x8 w4g_expand_scaled(uint32_t w, float sc, float off) {
  bf16x8 b;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t t = w >> (4 * p);
    b[2 * p] = (bf16)fmaf(__builtin_bit_cast(float, ((t & 0xFu) << 16) | 0x43000000u), sc, off);
    b[2 * p + 1] = (bf16)fmaf(__builtin_bit_cast(float, (t & 0x000F0000u) | 0x43000000u), sc, off);
  }
  return b;
}

template <int BM, int NTL, int STAGES, bool SC>
__global__ __launch_bounds__(256) void gemm_w4_kernel(const W4GArgs g) {
  constexpr int NW = 4, NT = NW * 64, MT = BM / 16, BN = NW * NTL * 16;
  constexpr int HALF = BM * 128, STAGE_BYTES = 2 * HALF;  // a stage: BM rows x (64 + 64) k of bf16
  constexpr int A_LD = HALF / (NT * 16);                  // DMA rounds per half
  constexpr int LOADS = 2 * A_LD + 2 * NTL;               // vector-memory ops a wave issues per step
  static_assert(BM % 16 == 0 && BM <= 256 && A_LD >= 1 && HALF % (NT * 16) == 0, "tile shape");
  static_assert(STAGES >= 2 && (STAGES - 2) * LOADS < 64, "vmcnt field");
  static_assert(STAGES * STAGE_BYTES + 16 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[STAGES * STAGE_BYTES + 16];  // + the split-K flag

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int tiles_m = (g.M + BM - 1) / BM;
  const int S = g.splitk;
  const int u = xcd_remap(blockIdx.x, gridDim.x), t = u / S, split = u - t * S;
  int tm, tn;
  ring_tile(t, tiles_m, g.tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int G = g.K >> 7;  // scale groups = granules per weight tile = k-steps of the whole K
  const int q0 = G * split / S, q1 = G * (split + 1) / S, nsteps = q1 - q0;

  const rsrc_t ra = make_rsrc(g.a, g.a_bytes), rw = make_rsrc(g.w, g.w_bytes), rs = make_rsrc(g.sc, g.s_bytes);
  // A DMA: LDS byte p = i NT 16 + tid 16 of a half image is row p / 128, lane-linear chunk tid & 7 = source
  // chunk (tid & 7) ^ swz(row); the tile row / k base rides in soffset
  const int K2 = g.K * 2;
  int a_off[A_LD];
#pragma unroll
  for (int i = 0; i < A_LD; ++i) {
    const int row = (i * NT + tid) >> 3;
    a_off[i] = m0 + row < g.M ? row * K2 + (((tid & 7) ^ ring_swz<128>(row)) << 4) : OOB;
  }
  // weights: this wave's column tiles (n0 / 16 + wid NTL + jn); tile j, granule q: (j G + q) 1024 + lane 16,
  // scales (j G + q) 32 + the four rows 4 fq .. (offset form) or the lane's own row fr (scaled form)
  int w_off[NTL], s_off[NTL];
#pragma unroll
  for (int jn = 0; jn < NTL; ++jn) {
    const int tile = (n0 >> 4) + wid * NTL + jn;
    const bool in = tile * 16 < g.N;
    w_off[jn] = in ? tile * G * 1024 + lane * 16 : OOB;
    s_off[jn] = in ? tile * G * 32 + (SC ? fr * 2 : fq * 8) : OOB;
  }

  uint4 wq[STAGES][NTL];
  uint2 wsc[STAGES][NTL];
  auto issue = [&](int q, int slot, uint4 (&w)[NTL], uint2 (&s)[NTL]) {
    const bool in = q < q1;
    char* base = smem + slot * STAGE_BYTES + wid * 1024;
    const int sa = m0 * K2 + q * 256;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < A_LD; ++i) ring_glds16(ra, base + h * HALF + i * NT * 16, in ? a_off[i] : OOB, sa + h * 128);
#pragma unroll
    for (int jn = 0; jn < NTL; ++jn) {
      const bool ok = in && w_off[jn] != OOB;
      w[jn] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rw, ok ? w_off[jn] + q * 1024 : OOB, 0, 2));
      if constexpr (SC) {
        s[jn].x = __builtin_amdgcn_raw_buffer_load_b16(rs, ok ? s_off[jn] + q * 32 : OOB, 0, 0);
        s[jn].y = 0;
      } else {
        s[jn] = bload8(rs, ok ? s_off[jn] + q * 32 : OOB);
      }
    }
  };

  f32x4 acc[MT][NTL];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int jn = 0; jn < NTL; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment reads of a stage: row r, 16-B chunk c of half h -> h HALF + r 128 + (c ^ swz(r)) 16; tile rows are
  // 16-aligned, so swz(r) depends on fr only.  k-step ks of the granule: half ks >> 1, chunk 4 (ks & 1) + fq
  const int sw = ring_swz<128>(fr);
  const int a_rd[4] = {fr * 128 + ((fq ^ sw) << 4), fr * 128 + (((4 + fq) ^ sw) << 4), HALF + fr * 128 + ((fq ^ sw) << 4),
                       HALF + fr * 128 + (((4 + fq) ^ sw) << 4)};
  const bf16x8 neg136 = __builtin_bit_cast(bf16x8, make_uint4(0xC308C308u, 0xC308C308u, 0xC308C308u, 0xC308C308u));

#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s) issue(q0 + s, s, wq[s], wsc[s]);

  for (int j0 = 0; j0 < nsteps; j0 += STAGES) {
#pragma unroll
    for (int us = 0; us < STAGES; ++us) {
      const int j = j0 + us;
      if (j >= nsteps) break;
      ring_wait_vmcnt<(STAGES - 2) * LOADS>();  // step j's DMAs and weights landed; later ones may still fly
      ring_barrier();                           // ... for every wave, and step j - 1 is fully read
      constexpr int NS = STAGES - 1;
      issue(q0 + j + NS, (us + NS) % STAGES, wq[(us + NS) % STAGES], wsc[(us + NS) % STAGES]);
      const char* base = smem + us * STAGE_BYTES;
      if constexpr (SC) {
        bf16x8 b[NTL][4];
#pragma unroll
        for (int jn = 0; jn < NTL; ++jn) {
          const uint4 wv = wq[us][jn];
          const float sc = w4g_bf(wsc[us][jn].x), off = -136.f * sc;
          b[jn][0] = w4g_expand_scaled(wv.x, sc, off);
          b[jn][1] = w4g_expand_scaled(wv.y, sc, off);
          b[jn][2] = w4g_expand_scaled(wv.z, sc, off);
          b[jn][3] = w4g_expand_scaled(wv.w, sc, off);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          bf16x8 af[4];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) af[ks] = *reinterpret_cast<const bf16x8*>(base + a_rd[ks] + i * 16 * 128);
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int jn = 0; jn < NTL; ++jn)
              acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[jn][ks], af[ks], acc[i][jn], 0, 0, 0);
        }
      } else {
        bf16x8 b[NTL][4];
        float sf[NTL][4];
#pragma unroll
        for (int jn = 0; jn < NTL; ++jn) {
          const uint4 wv = wq[us][jn];
          b[jn][0] = w4g_expand(wv.x);
          b[jn][1] = w4g_expand(wv.y);
          b[jn][2] = w4g_expand(wv.z);
          b[jn][3] = w4g_expand(wv.w);
          const uint2 sv = wsc[us][jn];
          sf[jn][0] = w4g_bf(sv.x & 0xFFFFu);
          sf[jn][1] = __builtin_bit_cast(float, sv.x & 0xFFFF0000u);
          sf[jn][2] = w4g_bf(sv.y & 0xFFFFu);
          sf[jn][3] = __builtin_bit_cast(float, sv.y & 0xFFFF0000u);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          bf16x8 af[4];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) af[ks] = *reinterpret_cast<const bf16x8*>(base + a_rd[ks] + i * 16 * 128);
          f32x4 corr = {0.f, 0.f, 0.f, 0.f};  // -136 * (the rows' sums of a over the group), the same for every n
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) corr = __builtin_amdgcn_mfma_f32_16x16x32_bf16(neg136, af[ks], corr, 0, 0, 0);
#pragma unroll
          for (int jn = 0; jn < NTL; ++jn) {
            f32x4 ag = corr;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) ag = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[jn][ks], af[ks], ag, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][jn][e] = fmaf(sf[jn][e], ag[e], acc[i][jn][e]);
          }
        }
      }
    }
  }
  ring_wait_vmcnt<0>();  // the DMAs issued past the K range (zeros) retire before LDS is handed on

  const bool reducer = S == 1 || ring_splitk_arrive<BM * BN, MT, NTL>(acc, g.ws, g.cnt, S, t, split,
                                                                       (int*)(smem + STAGES * STAGE_BYTES));
  if (!reducer) return;
  const int wcol = wid * NTL * 16;
  if (g.act == ACT_SILU_MUL) ring_epilogue_t<MT, NTL, 2, ACT_NONE>(acc, g, m0, n0, 0, wcol);
  else if (g.res) ring_epilogue_t<MT, NTL, 1, ACT_NONE>(acc, g, m0, n0, 0, wcol);
  else ring_epilogue_t<MT, NTL, 0, ACT_NONE>(acc, g, m0, n0, 0, wcol);
}

// variant ids (ops.W4_GEMM_CFGS): tile rows x columns, column tiles per wave, ring depth, expansion, LDS
//   1:  64 x 128, 2, 4 stages, offset,  64 KB   (33..64 rows)
//   2: 128 x 128, 2, 3 stages, scaled,  96 KB
//   3: 256 x 128, 2, 2 stages, scaled, 128 KB   (four column tiles per wave spilled: 256 accumulator registers)
//   4:  64 x 128, 2, 4 stages, scaled           (the other form of 1)
//   5: 128 x 128, 2, 3 stages, offset           (the other form of 2)
constexpr int W4G_NUM_VARIANTS = 6;  // 0 = by shape
struct W4GCfg {
  int bm, bn;
};
W4GCfg w4g_cfg(int v) {
  switch (v) {
    case 1: case 4: return {64, 128};
    case 2: case 5: return {128, 128};
    case 3: return {256, 128};
    default: return {0, 0};
  }
}

// K splits: while the units still fit one resident wave of blocks, every split keeps >= 2 scale groups, the
// slabs (8 B written + read per output and split) stay below the weight bytes the split spreads (K / 2 per
// column: S 16 BM <= K), and the slabs fit the workspace
int w4g_split(int tiles, int groups, int bm, int K, long long tile_elems, long long ws_elems, int cnt_elems) {
  if (tiles > cnt_elems) return 1;
  const int cus = mls_num_cus();
  int s = 1;
  while (s < 64 && tiles * (s + 1) <= cus && groups / (s + 1) >= 2 && (s + 1) * 16 * bm <= K &&
         (long long)tiles * (s + 1) * tile_elems <= ws_elems)
    ++s;
  return s;
}

}  // namespace

extern "C" {

int mls_gemm_w4a16_num_variants() { return W4G_NUM_VARIANTS; }

// out[M][N] = act(x . dequant(Wq, scales)^T + bias) (+ res); ACT_SILU_MUL: W rows gate / up interleaved in groups
// of 8, out [M][N/2].  Any M >= 1 with M K 2 < 2 GiB (ops.gemm_w4a16 runs more rows in blocks), N % 16 == 0,
// K % 128 == 0, N K / 2 < 2 GiB.  variant 0: by shape.  splitk 0: the launcher's
// pick (needs ws / cnt: fp32 slabs and int32 arrival counters, ZERO before the first launch; without them no
// split), > 0: that many, <= K / 128.
int mls_gemm_w4a16(const void* A, const void* Wq, const void* scales, const float* bias, const void* res, void* out,
                   int M, int N, int K, int act, int variant, int splitk, void* ws, long long ws_elems, void* cnt,
                   int cnt_elems, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 128 || N % 16 || variant < 0 || variant >= W4G_NUM_VARIANTS) return MLS_BAD_ARG;
  if (!A || !Wq || !scales || !out) return MLS_BAD_ARG;
  if (act != ACT_NONE && act != ACT_SILU_MUL) return MLS_BAD_ARG;
  if (res && act == ACT_SILU_MUL) return MLS_BAD_ARG;
  const size_t ab = (size_t)M * K * 2, wb = (size_t)N * K / 2;
  // operand offsets are 32-bit (buffer voffset + soffset); the output / residual descriptors are per tile
  if (ab >= 0x7FFFFFFFull || wb >= 0x7FFFFFFFull) return MLS_UNSUPPORTED;
  // by shape: measured (profiles/w4_gemm_ab.jsonl), the 64-row tile is ahead of, or level with (down at 512 rows,
  // variant 5), the 128- and 256-row ones on all four Llama-3-8B shapes from 33 to 4096 rows -- two blocks per CU
  // hide its barriers, and the row tiles of one weight panel re-read it from L2 -- so it serves every row count;
  // 2 .. 5 stay selectable
  const int v = variant > 0 ? variant : 1;
  const W4GCfg c = w4g_cfg(v);
  W4GArgs g{};
  g.a = (const bf16*)A;
  g.w = (const uint8_t*)Wq;
  g.sc = (const bf16*)scales;
  g.bias = bias;
  g.res = (const bf16*)res;
  g.out = (bf16*)out;
  g.M = M; g.N = N; g.K = K; g.act = act;
  g.ldo = act == ACT_SILU_MUL ? N / 2 : N;
  g.a_bytes = (uint32_t)ab;
  g.w_bytes = (uint32_t)wb;
  g.s_bytes = (uint32_t)((size_t)N * K / 128 * 2);
  const int tiles_m = (M + c.bm - 1) / c.bm;
  g.tiles_n = (N + c.bn - 1) / c.bn;
  const long long tiles = (long long)tiles_m * g.tiles_n, tile_elems = (long long)c.bm * c.bn;
  const int groups = K / 128;
  if (splitk <= 0) {
    g.splitk = ws && cnt && tiles <= cnt_elems ? w4g_split((int)tiles, groups, c.bm, K, tile_elems, ws_elems, cnt_elems) : 1;
  } else {
    g.splitk = splitk;
    if (splitk > 1 && (!ws || !cnt || splitk > groups || tiles > cnt_elems || tiles * splitk * tile_elems > ws_elems))
      return MLS_BAD_ARG;
  }
  if (tiles * g.splitk > 0x7FFFFFFFll) return MLS_UNSUPPORTED;
  g.ws = (float*)ws;
  g.cnt = (int*)cnt;
  const dim3 grid((unsigned)(tiles * g.splitk)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (v) {
    case 1: hipLaunchKernelGGL((gemm_w4_kernel<64, 2, 4, false>), grid, block, 0, st, g); break;
    case 2: hipLaunchKernelGGL((gemm_w4_kernel<128, 2, 3, true>), grid, block, 0, st, g); break;
    case 3: hipLaunchKernelGGL((gemm_w4_kernel<256, 2, 2, true>), grid, block, 0, st, g); break;
    case 4: hipLaunchKernelGGL((gemm_w4_kernel<64, 2, 4, true>), grid, block, 0, st, g); break;
    case 5: hipLaunchKernelGGL((gemm_w4_kernel<128, 2, 3, false>), grid, block, 0, st, g); break;
  }
  return hipGetLastError() == hipSuccess ? MLS_OK : MLS_BAD_ARG;
}

}  // extern "C"
