// Bottleneck boundary chain: one ResNet bottleneck's last 1x1 conv (+ residual + ReLU) and the NEXT
// bottleneck's first 1x1 conv in ONE kernel, so the block output y -- the widest tensor of the
// network (56x56x256 / 28x28x512 at bs=32: 51 / 26 MB) -- is written once and never re-read:
//
//   y  = relu(A1 . W3^T + b3 (+ res))      [M][N1]   stored (the next block's residual)
//   t1 = relu(y  . W1^T + b1)              [M][N2]   stored (the next block's conv2 input)
//
// A1 is the conv3 input [M][Ka] or, for a stage's first block, the dual operand [t2 | x_strided]
// (conv3 + downsample projection as one reduction, conv_gemm.hip MODE_DUAL) with no residual.
//
// Why: at bs = 32 the layer1 / layer2 1x1 convs run at 4-5 TB/s of HBM under concurrent streams
// (docs/PERF_NOTES.md, r2 PMC): bytes, not MFMAs, are their cost.  Unchained, y is written by conv3
// and read back by the next conv1 (+51 MB per layer1 boundary); here it stays in LDS.
//
// Structure (per block: one BM-row tile, 8 waves as 4 (M) x 2 (N)):
//   * A1 tile staged once into LDS (KS 64-wide slabs, 128-B rows, 16-B chunks XOR-swizzled by
//     row & 7 on the SOURCE address so the LDS-DMA stays lane-linear; conflict-free ds_read_b128).
//   * loop over the N1 / 64 output-channel chunks j, a 2-deep LDS-DMA ring of stages
//     {W3 rows j*64.. (64 x K1), W1 columns j*64.. (N2 x 64), residual chunk (BM x 64)}, stage j+1
//     in flight during chunk j (counted vmcnt + raw s_barrier, never a full drain in the loop):
//       GEMM1  acc1[BM x 64] = A1 . W3_j^T                       (MFMA 16x16x32 bf16)
//       pass 1 y = relu(acc1 + b3 + res) -> bf16, IN PLACE over the residual chunk in LDS
//       y chunk -> HBM with 16-B buffer stores
//       GEMM2  acc2[BM x N2] += y_j . W1_j^T   (the y chunk in LDS is exactly GEMM2's K-slab j)
//   * epilogue: t1 = relu(acc2 + b1) -> bf16 through LDS -> 16-B stores.
//   * C2 (mls_conv_chain_conv2, the layer1 boundaries): the A1 tile's first slab is not loaded but
//     computed, t2 = relu(conv3x3(t1_in, W2) + b2) -- the bottleneck's conv2 -- from a strip of t1_in
//     pixels and a ring of tap weights staged over the chunk ring before GEMM1 needs it.
// Numerics: y rounds once exactly as conv_gemm.hip's epilogue (acc + bias + res, ReLU, bf16); t1
// accumulates the same K order in fp32.
#include "common.h"  // + chain_sched.h
#include "fastdiv.h"

namespace {

#define LDS3 __attribute__((address_space(3)))

MLS_DEV void glds16(rsrc_t r, char* lds, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (LDS3 void*)lds, 16, voff, soff, 0, 0);
}

typedef unsigned int u32x4v __attribute__((__vector_size__(16)));

// LDS reads the waitcnt pass does not see (defined, with the why and the hazard, above
// conv_chain_ring_kernel); conv_chain_kernel's conv2 producer reads its tap ring through them
MLS_DEV uint32_t lds_off(const void* p);
MLS_DEV u32x4v lds_ld16_issue(uint32_t off);
template <typename T>
MLS_DEV void lds_landed(T& v);

// SW (template parameter): MFMA operand order.  true: D = W . A^T, so a lane's 4 accumulators are
// 4 consecutive output channels of one row -- pass 1 reads the residual and writes y as one 8-B
// LDS access per fragment (instead of four 2-B read-modify-writes), the t1 epilogue parks 8 B per
// fragment, and the biases come from wave-uniform scalar loads (no VGPR-resident bias table, no
// VMEM op beside the DMA ring); false: D = A . W^T.  Per boundary from the per-call A/B
// (profiles/r3_swap_epilogue_component_costs.jsonl): the single-slab (KS = 1) layer1 boundaries
// take SW (layer1.1 -> 1.2: 27.4 -> 23.2 us co-running), the others measured level or slower.
// MLS_CHAIN_SWAP=0/1 at build time forces one order everywhere (A/B builds).
#define CONST4 __attribute__((address_space(4)))

// the 4 biases of lane group fq in the 16 output channels starting at the wave-uniform nt0
MLS_DEV f32x4 bias4(const float* b, int nt0, int fq) {
  if (!b) return f32x4{0.f, 0.f, 0.f, 0.f};
  const CONST4 f32x4* bp = (const CONST4 f32x4*)(b + nt0);
  const f32x4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
  return fq == 0 ? b0 : fq == 1 ? b1 : fq == 2 ? b2 : b3;
}

struct ChainArgs {
  const bf16* a1;   // [M][Ka]            (conv3 input, stride 1)
  const bf16* a2;   // [B][H2][W2][Kb]    (dual: the block input, sampled at stride2) or null
  const bf16* w3;   // [N1][Ka + Kb]
  const float* b3;  // [N1]
  const bf16* res;  // [M][N1] or null
  bf16* y;          // [M][N1]
  const bf16* w1;   // [N2][N1]
  const float* b1;  // [N2]
  bf16* t1;         // [M][N2]
  int M, Ka, Kb, N1, N2;
  int Ho, Wo, H2, W2, stride2;  // dual geometry (M = B * Ho * Wo)
  FastDiv fd_howo, fd_wo;       // Ho * Wo, Wo (fastdiv.h)
  uint32_t a1_bytes, a2_bytes, w3_bytes, res_bytes, y_bytes, w1_bytes, t1_bytes;
  // conv2 producer (C2): a1 is not read; slab 0 of the A1 image is relu(conv3x3(t1in, w2) + b2)
  const bf16* t1in;  // [B][Ho][Wo][64]
  const bf16* w2;    // [64][3][3][64]
  const float* b2;   // [64]
  uint32_t t1in_bytes, w2_bytes;
};

// 16-B chunk swizzle of an LDS image row: 128-B rows (8 chunks): chunk ^ (r & 7); 64-B rows (4
// chunks): chunk ^ f(r & 7), f = (r0 | r2 << 1) -- conflict-free for the 16x16x32 fragment reads
// (conv_gemm.hip row_swz).  The LDS-DMA writes lane-linearly, so the swizzle goes on the SOURCE.
template <int CPR>
MLS_DEV int row_swz(int r) {
  if constexpr (CPR == 8) return r & 7;
  else return (r & 1) | ((r >> 1) & 2);
}

// Y2 (template parameter of both kernels): y feeds only a stride-2 1x1 projection (the last block of
// a stage whose successor is a dual block), so only the pixels with even oh and even ow are kept,
// compactly as [B][Hc][Wc][N1], Hc = (Ho + 1) / 2, Wc = (Wo + 1) / 2.  Element offset of output
// row m's y row in that tensor, or -1 for a pixel that is not kept (or a row past M).  The store of
// such a row is still issued, at the out-of-range offset: every wave keeps issuing Y_ST stores per
// chunk, which is what the counted vmcnt waits assume.  Branch-free, and computed once per tile.
MLS_DEV int y2_row_off(const ChainArgs& a, int m, int N1) {
  const int b = fastdiv(m, a.fd_howo), rem = m - b * (a.Ho * a.Wo);
  const int oh = fastdiv(rem, a.fd_wo), ow = rem - oh * a.Wo;
  const int off = ((b * ((a.Ho + 1) >> 1) + (oh >> 1)) * ((a.Wo + 1) >> 1) + (ow >> 1)) * N1;
  return (m < a.M && !((oh | ow) & 1)) ? off : -1;
}

// KS = (Ka + Kb) / 64 A1 slabs; KSA = Ka / 64 of them from a1, the rest from a2 (dual).  CW = the
// output-channel chunk of GEMM1 = the K slab of GEMM2 (64, or 32 where the weights of a 64-wide
// stage would not fit the LDS next to the A tile: layer2 -> 3 and layer3).  N1 is a template
// parameter so the chunk loop unrolls and every bias lives in registers, loaded before the first
// LDS-DMA: a plain global load consumed beside in-flight DMA makes hipcc wait vmcnt(0) and drain
// the ring (cdna_hip_programming.md §5, "Projection GEMM" item 4(b)).  OCC = waves per SIMD the
// register allocation must allow: 4 where the LDS footprint lets two blocks share a CU (<= 80 KB).
template <int BM, int KS, int N1, int N2, int CW, int OCC, bool SW, bool C2 = false, bool Y2 = false>
__global__ __launch_bounds__(512, OCC) void conv_chain_kernel(const ChainArgs a) {
  constexpr int NW = 8, NT = 512, WM = 4, WN = 2;
  constexpr int WTM = BM / WM, TM = WTM / 16;  // GEMM1 / GEMM2 wave rows
  constexpr int TN = CW / WN / 16;             // GEMM1 column fragments per wave
  constexpr int TN2 = N2 / WN / 16;            // GEMM2 column fragments per wave
  constexpr int CPR = CW / 8;                  // 16-B chunks per row of the W1 / residual / y images
  constexpr int RPP = 64 / CPR;                // rows of those images per 1-KiB DMA piece
  constexpr int A1_BYTES = BM * KS * 128;
  constexpr int W3_BYTES = CW * KS * 128;
  constexpr int W1_BYTES = N2 * CW * 2;
  constexpr int R_BYTES = BM * CW * 2;
  constexpr int STAGE = W3_BYTES + W1_BYTES + R_BYTES;
  constexpr int EPI_BYTES = BM * N2 * 2;
  constexpr int RING = A1_BYTES + 2 * STAGE;
  constexpr int LDS_BYTES = RING > EPI_BYTES ? RING : EPI_BYTES;
  constexpr int A1_PW = BM / 8 * KS / NW;  // 1-KiB DMA pieces per wave
  constexpr int A1_S0 = C2 ? 1 : 0;        // first A1 slab that is loaded (C2: slab 0 is computed)
  constexpr int A1_PWL = BM / 8 * (KS - A1_S0) / NW;
  constexpr int W3_PW = CW / 8 * KS / NW;
  constexpr int W1_PW = N2 / RPP / NW;
  constexpr int R_PW = BM / RPP / NW;
  constexpr int Y_ST = BM * CPR / NT;     // 16-B y stores per thread per chunk
  constexpr int T_ST = BM * N2 / 8 / NT;  // 16-B t1 stores per thread
  constexpr int NJ = N1 / CW;
  static_assert(TM >= 1 && TN >= 1 && TN2 >= 1 && (CW == 64 || CW == 32), "tile");
  static_assert(A1_PW * NW * 8 == BM * KS && W3_PW * NW * 8 == CW * KS, "A1 / W3 DMA split");
  static_assert(W1_PW * NW * RPP == N2 && R_PW * NW * RPP == BM, "W1 / residual DMA split");
  static_assert(Y_ST * NT == BM * CPR && T_ST * NT == BM * N2 / 8, "epilogue split");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int fr = lane & 15, fq = lane >> 4;
  const int m0 = xcd_remap(blockIdx.x, gridDim.x) * BM;
  const int K1 = a.Ka + a.Kb, KSA = a.Ka / 64;
  const bool has_res = a.res != nullptr;

  // (original order) biases of every column this lane touches, before any DMA is in flight
  float b3v[SW ? 1 : NJ][TN], b1v[TN2];
  if constexpr (!SW) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) b3v[j][jn] = a.b3 ? a.b3[j * CW + wn * (CW / 2) + jn * 16 + fr] : 0.f;
#pragma unroll
    for (int jn = 0; jn < TN2; ++jn) b1v[jn] = a.b1 ? a.b1[wn * (N2 / 2) + jn * 16 + fr] : 0.f;
  }

  // DMA lane geometry.  128-B rows (A1, W3): 8 rows x 8 chunks per piece; CW-wide rows (W1,
  // residual): RPP rows x CPR chunks.  LDS chunk c of row r holds the logical chunk c ^ swz(r).
  const int r8 = lane >> 3, lc = (lane & 7) ^ r8;
  const int rq = lane / CPR, lq = (lane % CPR) ^ row_swz<CPR>(rq);

  const rsrc_t a1r = make_rsrc(a.a1, a.a1_bytes);
  const rsrc_t a2r = make_rsrc(a.a2, a.a2_bytes);
  const rsrc_t w3r = make_rsrc(a.w3, a.w3_bytes);
  const rsrc_t w1r = make_rsrc(a.w1, a.w1_bytes);
  const rsrc_t rr = make_rsrc(a.res, a.res_bytes);
  const rsrc_t yr = make_rsrc(a.y, a.y_bytes);
  const rsrc_t tr = make_rsrc(a.t1, a.t1_bytes);

  char* const sA1 = smem;
  auto stage_base = [&](int buf) { return smem + A1_BYTES + buf * STAGE; };

  // ---- A1 tile: slab s, row block rb; wave w issues pieces q = w * A1_PW + i
#pragma unroll
  for (int i = 0; i < A1_PWL; ++i) {
    const int q = A1_S0 * (BM / 8) + wid * A1_PWL + i;
    const int s = q / (BM / 8), rb = q - s * (BM / 8);
    const int m = m0 + rb * 8 + r8;
    char* dst = sA1 + q * 1024;
    if (s < KSA) {
      glds16(a1r, dst, m < a.M ? (m * a.Ka + s * 64 + lc * 8) * 2 : OOB, 0);
    } else {  // dual operand: row m of the output grid samples the block input at stride2
      int off = OOB;
      if (m < a.M) {
        const int b = fastdiv(m, a.fd_howo), rem = m - b * (a.Ho * a.Wo);
        const int oh = fastdiv(rem, a.fd_wo), ow = rem - oh * a.Wo;
        off = (((b * a.H2 + oh * a.stride2) * a.W2 + ow * a.stride2) * a.Kb + (s - KSA) * 64 + lc * 8) * 2;
      }
      glds16(a2r, dst, off, 0);
    }
  }

  auto issue = [&](int j, int buf) {
    char* sW3 = stage_base(buf);
    char* sW1 = sW3 + W3_BYTES;
    char* sR = sW1 + W1_BYTES;
#pragma unroll
    for (int i = 0; i < W3_PW; ++i) {  // W3 rows j*CW + rb*8 + r8 of K slab s ([KS][CW][64] image)
      const int q = wid * W3_PW + i;
      const int s = q / (CW / 8), rb = q - s * (CW / 8);
      glds16(w3r, sW3 + q * 1024, ((j * CW + rb * 8 + r8) * K1 + s * 64 + lc * 8) * 2, 0);
    }
#pragma unroll
    for (int i = 0; i < W1_PW; ++i) {  // W1 rows n2 = q*RPP + rq, columns j*CW..
      const int q = wid * W1_PW + i;
      glds16(w1r, sW1 + q * 1024, ((q * RPP + rq) * N1 + j * CW + lq * 8) * 2, 0);
    }
    if (has_res) {
#pragma unroll
      for (int i = 0; i < R_PW; ++i) {
        const int q = wid * R_PW + i;
        const int m = m0 + q * RPP + rq;
        glds16(rr, sR + q * 1024, m < a.M ? (m * N1 + j * CW + lq * 8) * 2 : OOB, 0);
      }
    }
  };

  if constexpr (C2) {
    // ---- conv2 producer: A1 slab 0 = t2 = relu(conv3x3(t1in, W2) + b2) of the tile's BM pixels,
    // rounded to bf16 where the separate conv2 kernel rounds it; t2 never goes to memory.
    //   strip  the t1in pixels [m0 - (Wo + 1), m0 + BM + (Wo + 1)) of the flattened [M][64] tensor,
    //          strip row i = pixel m0 - (Wo + 1) + i (128-B rows, the A1 chunk swizzle by row & 7):
    //          tap (dy, dx) of tile row r is strip row r + (Wo + 1) + dy * Wo + dx.  A tap outside
    //          the image is masked to zero; a tap inside it is a pixel of the same image, so it is
    //          in [0, M) and inside the strip.
    //   taps   W2[:, t, :] ([64][64], 8 KB: one 1-KiB DMA piece per wave) through a 4-slot ring, 3
    //          taps in flight, counted vmcnt + raw s_barrier per tap.
    // Both alias the ring (strip: stage 0, taps: stage 1), which is idle until GEMM1, so the LDS
    // footprint is the unfused kernel's.  The a2 slabs of the dual form and the strip are issued
    // before the taps: older, so every counted wait below covers them.
    constexpr int TAPS = 9, TSLOTS = 4, TAHEAD = 3, SROWS = 256, TNP = 64 / WN / 16;
    static_assert(BM == 128 && STAGE >= SROWS * 128 && STAGE >= TSLOTS * 8192, "strip / tap ring alias one stage each");
    char* const sS = stage_base(0);
    char* const sT = stage_base(1);
    const rsrc_t t1r = make_rsrc(a.t1in, a.t1in_bytes);
    const rsrc_t w2r = make_rsrc(a.w2, a.w2_bytes);
    const int halo = a.Wo + 1;  // host: 2 * halo + BM <= SROWS
#pragma unroll
    for (int i = 0; i < SROWS / 8 / NW; ++i) {
      const int q = wid * (SROWS / 8 / NW) + i;
      const int sr = q * 8 + r8, p = m0 - halo + sr;
      glds16(t1r, sS + q * 1024, (p >= 0 && p < a.M && sr < BM + 2 * halo) ? (p * 64 + lc * 8) * 2 : OOB, 0);
    }
    auto issue_tap = [&](int t) {  // rows n = wid * 8 + r8 of tap t
      glds16(w2r, sT + (t % TSLOTS) * 8192 + wid * 1024, (((wid * 8 + r8) * TAPS + t) * 64 + lc * 8) * 2, 0);
    };
#pragma unroll
    for (int t = 0; t < TAHEAD; ++t) issue_tap(t);

    // bit t of okm[i]: tap t of this lane's row i lies inside the image
    int okm[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * WTM + i * 16 + fr;
      okm[i] = 0;
      if (m < a.M) {
        const int b = fastdiv(m, a.fd_howo), rem = m - b * (a.Ho * a.Wo);
        const int oh = fastdiv(rem, a.fd_wo), ow = rem - oh * a.Wo;
#pragma unroll
        for (int t = 0; t < TAPS; ++t)
          if ((unsigned)(oh + t / 3 - 1) < (unsigned)a.Ho && (unsigned)(ow + t % 3 - 1) < (unsigned)a.Wo)
            okm[i] |= 1 << t;
      }
    }

    f32x4 accp[TM][TNP];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int jn = 0; jn < TNP; ++jn) accp[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      // tap t landed: the younger ops are the taps t + 1 .. t + TAHEAD - 1 that exist
      if (t + 2 < TAPS) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else if (t + 1 < TAPS) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave is done with tap t - 1: its slot is free
      if (t + TAHEAD < TAPS) issue_tap(t + TAHEAD);
      const int shift = halo + (t / 3 - 1) * a.Wo + (t % 3 - 1);
      // asm reads: written in C++, hipcc drains the tap ring (vmcnt(0)) before the first ds_read
      // after every issue_tap.  One batch per tap, issued and landed back to back.
      const uint32_t oS = lds_off(sS), oT = lds_off(sT + (t % TSLOTS) * 8192);
      u32x4v av[2][TM], bv[2][TNP];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ch = fq + 4 * kk;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int r = wm * WTM + i * 16 + fr + shift;
          av[kk][i] = lds_ld16_issue(oS + (r * 8 + (ch ^ (r & 7))) * 16);
        }
#pragma unroll
        for (int jn = 0; jn < TNP; ++jn) {
          const int n = wn * 32 + jn * 16 + fr;
          bv[kk][jn] = lds_ld16_issue(oT + (n * 8 + (ch ^ (n & 7))) * 16);
        }
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < TM; ++i) lds_landed(av[kk][i]);
#pragma unroll
        for (int jn = 0; jn < TNP; ++jn) lds_landed(bv[kk][jn]);
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 af[TM], bfv[TNP];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          u32x4v v = av[kk][i];
          if (!((okm[i] >> t) & 1)) v = u32x4v{0u, 0u, 0u, 0u};
          af[i] = __builtin_bit_cast(bf16x8, v);
        }
#pragma unroll
        for (int jn = 0; jn < TNP; ++jn) bfv[jn] = __builtin_bit_cast(bf16x8, bv[kk][jn]);
        // D = W . A^T: a lane's 4 accumulators are 4 consecutive channels of tile row fr
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int jn = 0; jn < TNP; ++jn)
            accp[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfv[jn], af[i], accp[i][jn], 0, 0, 0);
      }
    }
    // every DMA has landed (vmcnt(0) above), so the plain stores below cost no extra wait
#pragma unroll
    for (int jn = 0; jn < TNP; ++jn) {
      const int nt0 = wn * 32 + jn * 16, col = nt0 + fq * 4;
      const f32x4 bb = bias4(a.b2, nt0, fq);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 16 + fr;
        bf16x4 q;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = accp[i][jn][r];
          q[r] = (bf16)fmaxf(e + bb[r], 0.f);
        }
        *reinterpret_cast<uint2*>(sA1 + row * 128 + (((col >> 3) ^ (row & 7)) << 4) + (col & 7) * 2) =
            __builtin_bit_cast(uint2, q);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave is done with the strip and the taps: the ring is free
  }
  issue(0, 0);

  int yro[Y2 ? Y_ST : 1];  // (Y2) the compact y row of each of this thread's Y_ST store rows
  if constexpr (Y2) {
#pragma unroll
    for (int it = 0; it < Y_ST; ++it) yro[it] = y2_row_off(a, m0 + (tid + it * NT) / CPR, N1);
  }

  f32x4 acc2[TM][TN2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int jn = 0; jn < TN2; ++jn) acc2[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    // stage j landed: the only younger VMEM ops are chunk j-1's y stores
    if (j == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // the biases are retired too: pin their first use here, before stage 1 is issued
      if constexpr (!SW) {
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
          for (int jn = 0; jn < TN; ++jn) asm volatile("" ::"v"(b3v[jj][jn]));
#pragma unroll
        for (int jn = 0; jn < TN2; ++jn) asm volatile("" ::"v"(b1v[jn]));
      }
    } else {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Y_ST) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (j + 1 < NJ) issue(j + 1, (j + 1) & 1);
    char* sW3 = stage_base(j & 1);
    char* sW1 = sW3 + W3_BYTES;
    char* sR = sW1 + W1_BYTES;

    // ---- GEMM1: acc1[BM x CW] = A1 . W3_j^T
    f32x4 acc1[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) acc1[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint4* A1s = reinterpret_cast<const uint4*>(sA1);
    const uint4* W3s = reinterpret_cast<const uint4*>(sW3);
#pragma unroll
    for (int kk = 0; kk < 2 * KS; ++kk) {
      const int s = kk >> 1, ch = fq + 4 * (kk & 1);
      bf16x8 af[TM], bfv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm * WTM + i * 16 + fr;
        af[i] = __builtin_bit_cast(bf16x8, A1s[s * BM * 8 + r * 8 + (ch ^ (r & 7))]);
      }
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) {
        const int n = wn * (CW / 2) + jn * 16 + fr;
        bfv[jn] = __builtin_bit_cast(bf16x8, W3s[s * CW * 8 + n * 8 + (ch ^ (n & 7))]);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn)
          acc1[i][jn] = SW ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfv[jn], af[i], acc1[i][jn], 0, 0, 0)
                                       : __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfv[jn], acc1[i][jn], 0, 0, 0);
    }

    // ---- pass 1: y = relu(acc1 + b3 (+ res)) -> bf16, in place over the residual chunk
    if constexpr (SW) {
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) {
        const int nt0 = wn * (CW / 2) + jn * 16, col = nt0 + fq * 4;  // col % 8 in {0, 4}: 8 B in one chunk
        const f32x4 bb = bias4(a.b3, j * CW + nt0, fq);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = wm * WTM + i * 16 + fr;
          uint2* p = reinterpret_cast<uint2*>(sR + row * (CW * 2) + (((col >> 3) ^ row_swz<CPR>(row)) << 4) +
                                              (col & 7) * 2);
          float rs[4] = {0.f, 0.f, 0.f, 0.f};
          if (has_res) {
            const bf16x4 rv = __builtin_bit_cast(bf16x4, *p);
#pragma unroll
            for (int r = 0; r < 4; ++r) rs[r] = (float)rv[r];
          }
          bf16x4 q;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = acc1[i][jn][r];  // through a named float (ext-vector element bit-cast hazard)
            q[r] = (bf16)fmaxf(e + bb[r] + rs[r], 0.f);
          }
          *p = __builtin_bit_cast(uint2, q);
        }
      }
    } else
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
      const int col = wn * (CW / 2) + jn * 16 + fr;
      const float bb = b3v[j][jn];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wm * WTM + i * 16 + fq * 4 + r;
          bf16* p = reinterpret_cast<bf16*>(sR + row * (CW * 2) + (((col >> 3) ^ row_swz<CPR>(row)) << 4) +
                                            (col & 7) * 2);
          const float e = acc1[i][jn][r];  // through a named float (ext-vector element bit-cast hazard)
          float v = e + bb;
          if (has_res) v += (float)*p;
          *p = (bf16)fmaxf(v, 0.f);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    // ---- y chunk -> HBM (16-B rows), issued before GEMM2 so the stores drain under its MFMAs
#pragma unroll
    for (int it = 0; it < Y_ST; ++it) {
      const int q = tid + it * NT;
      const int row = q / CPR, c = q % CPR;
      const uint4 v = *reinterpret_cast<const uint4*>(sR + row * (CW * 2) + ((c ^ row_swz<CPR>(row)) << 4));
      const int m = m0 + row;
      int off;
      if constexpr (Y2) {
        off = yro[it] >= 0 ? (yro[it] + j * CW + c * 8) * 2 : OOB;
      } else {
        off = m < a.M ? (m * N1 + j * CW + c * 8) * 2 : OOB;
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), yr, off, 0, 0);
    }

    // ---- GEMM2: acc2[BM x N2] += y_j . W1_j^T
    const uint4* Ys = reinterpret_cast<const uint4*>(sR);
    const uint4* W1s = reinterpret_cast<const uint4*>(sW1);
#pragma unroll
    for (int kk = 0; kk < CW / 32; ++kk) {
      const int ch = fq + 4 * kk;
      bf16x8 af[TM], bfv[TN2];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm * WTM + i * 16 + fr;
        af[i] = __builtin_bit_cast(bf16x8, Ys[r * CPR + (ch ^ row_swz<CPR>(r))]);
      }
#pragma unroll
      for (int jn = 0; jn < TN2; ++jn) {
        const int n = wn * (N2 / 2) + jn * 16 + fr;
        bfv[jn] = __builtin_bit_cast(bf16x8, W1s[n * CPR + (ch ^ row_swz<CPR>(n))]);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN2; ++jn)
          acc2[i][jn] = SW ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfv[jn], af[i], acc2[i][jn], 0, 0, 0)
                                       : __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfv[jn], acc2[i][jn], 0, 0, 0);
    }
  }

  // ---- epilogue: t1 = relu(acc2 + b1) -> bf16 tile in LDS -> 16-B stores
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // every wave is done reading the ring
  constexpr int TPR = N2 / 8;    // 16-B chunks per t1 row
  bf16* to = reinterpret_cast<bf16*>(smem);
  if constexpr (SW) {
#pragma unroll
    for (int jn = 0; jn < TN2; ++jn) {
      const int nt0 = wn * (N2 / 2) + jn * 16, col = nt0 + fq * 4;
      const f32x4 bb = bias4(a.b1, nt0, fq);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 16 + fr;
        bf16x4 q;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = acc2[i][jn][r];
          q[r] = (bf16)fmaxf(e + bb[r], 0.f);
        }
        *reinterpret_cast<uint2*>(to + row * N2 + ((((col >> 3) ^ (row & 7))) << 3) + (col & 7)) =
            __builtin_bit_cast(uint2, q);
      }
    }
  } else
#pragma unroll
  for (int jn = 0; jn < TN2; ++jn) {
    const int col = wn * (N2 / 2) + jn * 16 + fr;
    const float bb = b1v[jn];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * WTM + i * 16 + fq * 4 + r;
        const float e = acc2[i][jn][r];
        // chunk swizzle by row (TPR >= 8) keeps the 16-lane column groups on distinct banks
        to[row * N2 + ((((col >> 3) ^ (row & 7))) << 3) + (col & 7)] = (bf16)fmaxf(e + bb, 0.f);
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int it = 0; it < T_ST; ++it) {
    const int q = tid + it * NT;
    const int row = q / TPR, c = q - (q / TPR) * TPR;
    const uint4 v = *reinterpret_cast<const uint4*>(to + row * N2 + ((c ^ (row & 7)) << 3));
    const int m = m0 + row;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), tr, m < a.M ? (m * a.N2 + c * 8) * 2 : OOB,
                                           0, 0);
  }
}

// s_waitcnt vmcnt(n) for a wave-uniform n that is a constant wherever the loops unroll and a
// two-way choice (residual or none, a block's first tile or a later one) elsewhere.  Anything above
// the listed counts waits for everything, which is only ever stricter.
MLS_DEV void vm_wait(int n) {
#define MLS_VMW(k) \
  case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (n) {
    MLS_VMW(1) MLS_VMW(2) MLS_VMW(3) MLS_VMW(4) MLS_VMW(5) MLS_VMW(6) MLS_VMW(7) MLS_VMW(8) MLS_VMW(9) MLS_VMW(10)
    MLS_VMW(11) MLS_VMW(12) MLS_VMW(13) MLS_VMW(14) MLS_VMW(15) MLS_VMW(16) MLS_VMW(17) MLS_VMW(18) MLS_VMW(19)
    MLS_VMW(20)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
#undef MLS_VMW
}

// LDS accesses of the ring kernel's epilogues as inline asm.  hipcc's waitcnt pass treats an LDS-DMA
// as a pending LDS write and puts s_waitcnt vmcnt(0) before every ds_write it can see (and before a
// ds_read of the same address): written in C++, pass 1's in-place y write drains the whole ring in
// every chunk, whatever the hand-placed counted wait allows (conv_chain_kernel above compiles that
// way: its stage j + 1 has to land before chunk j's pass 1 ends).  These it does not see; a batch of
// reads is issued, then lds_landed() ties each value to an lgkmcnt(0); the writes are retired by the
// lgkmcnt(0) before the barrier that publishes them.
MLS_DEV uint32_t lds_off(const void* p) { return (uint32_t)(uintptr_t)(LDS3 const char*)p; }
// HAZARD: between lds_ld*_issue() and lds_landed() the compiler believes the register already holds
// the value; a copy or spill of it placed there would read stale data.  Nothing orders that but
// register allocation: a batch is issued and landed back to back with no other code between, and
// every instantiation must keep 0 spills / 0 scratch (-Rpass-analysis=kernel-resource-usage; recheck
// the .s when a batch grows).
MLS_DEV uint2 lds_ld8_issue(uint32_t off) {  // the value is valid after lds_landed() on it
  uint2 v;
  asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(off) : "memory");
  return v;
}
MLS_DEV uint32_t lds_ld2_issue(uint32_t off) {
  uint32_t v;
  asm volatile("ds_read_u16 %0, %1" : "=v"(v) : "v"(off) : "memory");
  return v;
}
template <typename T>
MLS_DEV void lds_landed(T& v) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v)::"memory"); }
MLS_DEV u32x4v lds_ld16_issue(uint32_t off) {
  u32x4v v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(off) : "memory");
  return v;
}
MLS_DEV uint4 lds_ld16(uint32_t off) {
  uint4 v;
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(off) : "memory");
  return v;
}
MLS_DEV void lds_st8(uint32_t off, uint2 v) { asm volatile("ds_write_b64 %0, %1" ::"v"(off), "v"(v) : "memory"); }
MLS_DEV void lds_st2(uint32_t off, bf16 h) {
  const uint32_t v = __builtin_bit_cast(unsigned short, h);
  asm volatile("ds_write_b16 %0, %1" ::"v"(off), "v"(v) : "memory");
}

// The same chain with more bytes in flight per CU: an S-deep ring (S - 1 stages in flight) and,
// with PERS, a persistent block that walks the row tiles chain_sched.h gives it.
//
//   !PERS  one tile per block as above; a stage is {W3_j, W1_j, residual chunk j}.
//   PERS   W3 and W1 are loaded into LDS once per block (NJ chunk images each, the layout of a
//          stage's); a stage is the residual chunk alone (the y staging of the dual form, which has
//          no residual); the A1 image is double-buffered and t1 has its own staging tile.  The ring
//          runs on across tiles: at step (t, j) the stage of the step S - 1 later is issued, for the
//          block's next tile once j + S - 1 >= NJ, the next tile's A1 first when that stage is its
//          chunk 0.  Past the block's last tile the same loads are issued with every row out of
//          range (they write nothing that is read), so the counts below hold on every tile.
//
// The counted wait.  vmcnt retires in issue order, so at the top of step g = (t, j) stage g has
// landed once at most n(g) younger VMEM ops are outstanding.  A wave's order within step h is
// [stage h + S - 1 (A1 of the next tile first)] [Y_ST y stores] [T_ST t1 stores after a tile's last
// chunk]; stage g was issued in step g - S + 1, so the younger ops are
//     the stages g + 1 .. g + S - 2 that exist:  n_st each (this wave's DMA pieces of one stage),
//                                                + n_a1 if one of them is a tile's chunk 0 (PERS)
//     the y stores of steps g - S + 1 .. g - 1:   Y_ST each; only j of them on a block's first tile
//     the t1 stores of the previous tile (PERS):  T_ST if its last step is among those, j <= S - 2
// !PERS: n(j) = max(0, min(S - 2, NJ - 1 - j)) * n_st + min(j, S - 1) * Y_ST   (S = 2: the kernel above)
// PERS:  n(j) = (S - 2) * n_st + [j >= NJ - S + 2] * n_a1
//               + (first tile ? min(j, S - 1) * Y_ST : (S - 1) * Y_ST + [j <= S - 2] * T_ST)
// The DMA splits are strided over the waves (piece q = i * 8 + wave) and a piece type with fewer
// than 8 pieces is issued by the first waves only, so n_st and n_a1 are per-wave values.
template <int BM, int KS, int N1, int N2, int CW, int S, int OCC, bool SW, bool PERS, bool Y2 = false>
__global__ __launch_bounds__(512, OCC) void conv_chain_ring_kernel(const ChainArgs a, const int ntiles) {
  constexpr int NW = 8, NT = 512, WM = 4, WN = 2;
  constexpr int WTM = BM / WM, TM = WTM / 16;
  constexpr int TN = CW / WN / 16;
  constexpr int TN2 = N2 / WN / 16;
  constexpr int CPR = CW / 8;
  constexpr int RPP = 64 / CPR;
  constexpr int NJ = N1 / CW;
  constexpr int A1_BYTES = BM * KS * 128;
  constexpr int W3_BYTES = CW * KS * 128;
  constexpr int W1_BYTES = N2 * CW * 2;
  constexpr int R_BYTES = BM * CW * 2;
  constexpr int EPI_BYTES = BM * N2 * 2;
  constexpr int STAGE = PERS ? R_BYTES : W3_BYTES + W1_BYTES + R_BYTES;
  constexpr int OFF_W3 = (PERS ? 2 : 1) * A1_BYTES;         // PERS: resident W3, NJ chunk images
  constexpr int OFF_W1 = OFF_W3 + (PERS ? NJ * W3_BYTES : 0);  // PERS: resident W1
  constexpr int OFF_EPI = OFF_W1 + (PERS ? NJ * W1_BYTES : 0);  // PERS: t1 staging (!PERS: over the ring)
  constexpr int OFF_RING = OFF_EPI + (PERS ? EPI_BYTES : 0);
  constexpr int RING_END = OFF_RING + S * STAGE;
  constexpr int LDS_BYTES = RING_END > EPI_BYTES ? RING_END : EPI_BYTES;
  constexpr int A1_P = BM / 8 * KS, W3_P = CW / 8 * KS, W1_P = N2 / RPP, R_P = BM / RPP;  // 1-KiB DMA pieces
  constexpr int Y_ST = BM * CPR / NT;
  constexpr int T_ST = BM * N2 / 8 / NT;
  static_assert(TM >= 1 && TN >= 1 && TN2 >= 1 && (CW == 64 || CW == 32), "tile");
  static_assert(S >= 2 && S - 1 <= NJ && (!PERS || NJ % S == 0), "ring depth");
  static_assert(Y_ST * NT == BM * CPR && T_ST * NT == BM * N2 / 8, "epilogue split");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int fr = lane & 15, fq = lane >> 4;
  const int G = gridDim.x;
  int tile = chain_first_tile(blockIdx.x, G);
  if (tile >= ntiles) return;  // a forced grid larger than the tile count
  int m0 = tile * BM;
  const int K1 = a.Ka + a.Kb, KSA = a.Ka / 64;
  const bool has_res = a.res != nullptr;

  float b3v[SW ? 1 : NJ][TN], b1v[TN2];
  if constexpr (!SW) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) b3v[j][jn] = a.b3 ? a.b3[j * CW + wn * (CW / 2) + jn * 16 + fr] : 0.f;
#pragma unroll
    for (int jn = 0; jn < TN2; ++jn) b1v[jn] = a.b1 ? a.b1[wn * (N2 / 2) + jn * 16 + fr] : 0.f;
  }

  const int r8 = lane >> 3, lc = (lane & 7) ^ r8;
  const int rq = lane / CPR, lq = (lane % CPR) ^ row_swz<CPR>(rq);

  const rsrc_t a1r = make_rsrc(a.a1, a.a1_bytes);
  const rsrc_t a2r = make_rsrc(a.a2, a.a2_bytes);
  const rsrc_t w3r = make_rsrc(a.w3, a.w3_bytes);
  const rsrc_t w1r = make_rsrc(a.w1, a.w1_bytes);
  const rsrc_t rr = make_rsrc(a.res, a.res_bytes);
  const rsrc_t yr = make_rsrc(a.y, a.y_bytes);
  const rsrc_t tr = make_rsrc(a.t1, a.t1_bytes);

  // this wave's pieces of a P-piece image: q = i * NW + wid < P
  auto pieces = [&](int P) { return P / NW + (wid < P % NW ? 1 : 0); };
  const int n_a1 = pieces(A1_P);
  const int n_st = (PERS ? 0 : pieces(W3_P) + pieces(W1_P)) + (has_res ? pieces(R_P) : 0);

  auto issue_a1 = [&](int mt, char* dstA) {
#pragma unroll
    for (int i = 0; i < (A1_P + NW - 1) / NW; ++i) {
      const int q = i * NW + wid;
      if (A1_P % NW != 0 && q >= A1_P) break;
      const int s = q / (BM / 8), rb = q - s * (BM / 8);
      const int m = mt + rb * 8 + r8;
      char* dst = dstA + q * 1024;
      if (s < KSA) {
        glds16(a1r, dst, m < a.M ? (m * a.Ka + s * 64 + lc * 8) * 2 : OOB, 0);
      } else {
        int off = OOB;
        if (m < a.M) {
          const int b = fastdiv(m, a.fd_howo), rem = m - b * (a.Ho * a.Wo);
          const int oh = fastdiv(rem, a.fd_wo), ow = rem - oh * a.Wo;
          off = (((b * a.H2 + oh * a.stride2) * a.W2 + ow * a.stride2) * a.Kb + (s - KSA) * 64 + lc * 8) * 2;
        }
        glds16(a2r, dst, off, 0);
      }
    }
  };
  auto issue_w = [&](int j, char* sW3, char* sW1) {
#pragma unroll
    for (int i = 0; i < (W3_P + NW - 1) / NW; ++i) {
      const int q = i * NW + wid;
      if (W3_P % NW != 0 && q >= W3_P) break;
      const int s = q / (CW / 8), rb = q - s * (CW / 8);
      glds16(w3r, sW3 + q * 1024, ((j * CW + rb * 8 + r8) * K1 + s * 64 + lc * 8) * 2, 0);
    }
#pragma unroll
    for (int i = 0; i < (W1_P + NW - 1) / NW; ++i) {
      const int q = i * NW + wid;
      if (W1_P % NW != 0 && q >= W1_P) break;
      glds16(w1r, sW1 + q * 1024, ((q * RPP + rq) * N1 + j * CW + lq * 8) * 2, 0);
    }
  };
  auto issue_r = [&](int j, int mt, char* sR) {
    if (!has_res) return;
#pragma unroll
    for (int i = 0; i < (R_P + NW - 1) / NW; ++i) {
      const int q = i * NW + wid;
      if (R_P % NW != 0 && q >= R_P) break;
      const int m = mt + q * RPP + rq;
      glds16(rr, sR + q * 1024, m < a.M ? (m * N1 + j * CW + lq * 8) * 2 : OOB, 0);
    }
  };
  // chunk j's weight images and the ring slot's residual / y chunk
  auto w3_at = [&](int j, int slot) { return smem + (PERS ? OFF_W3 + j * W3_BYTES : OFF_RING + slot * STAGE); };
  auto w1_at = [&](int j, int slot) {
    return smem + (PERS ? OFF_W1 + j * W1_BYTES : OFF_RING + slot * STAGE + W3_BYTES);
  };
  auto r_at = [&](int slot) { return smem + OFF_RING + slot * STAGE + (PERS ? 0 : W3_BYTES + W1_BYTES); };
  auto issue_stage = [&](int j, int slot, int mt) {
    if constexpr (!PERS) issue_w(j, w3_at(j, slot), w1_at(j, slot));
    issue_r(j, mt, r_at(slot));
  };

  if constexpr (PERS) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) issue_w(j, w3_at(j, 0), w1_at(j, 0));
  }
  issue_a1(m0, smem);
#pragma unroll
  for (int s = 0; s < S - 1; ++s) issue_stage(s, s, m0);
  if constexpr (PERS) {
    // once per block: the weights, the first A1 and the first stages all landed (and the biases)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (!SW) {
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) asm volatile("" ::"v"(b3v[jj][jn]));
#pragma unroll
      for (int jn = 0; jn < TN2; ++jn) asm volatile("" ::"v"(b1v[jn]));
    }
  }

  f32x4 acc2[TM][TN2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int jn = 0; jn < TN2; ++jn) acc2[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

  int abuf = 0;         // PERS: the A1 buffer of the current tile
  bool first = true;    // PERS: the block's first tile (no older tile's stores in flight)
  for (;;) {
    int m0n = a.M;  // the block's next tile; none: every row out of range
    if constexpr (PERS) {
      const int next = chain_next_tile(tile, G);
      if (next < ntiles) m0n = next * BM;
    }
    char* const sA1 = smem + abuf * A1_BYTES;
    int yro[Y2 ? Y_ST : 1];  // (Y2) the compact y row of each of this thread's Y_ST store rows
    if constexpr (Y2) {
#pragma unroll
      for (int it = 0; it < Y_ST; ++it) yro[it] = y2_row_off(a, m0 + (tid + it * NT) / CPR, N1);
    }

#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      // ---- stage j landed (the count is derived above the kernel)
      if constexpr (PERS) {
        const int jm = j < S - 1 ? j : S - 1;
        const int ahead = (S - 2) * n_st + (j >= NJ - S + 2 ? n_a1 : 0);
        vm_wait(ahead + (first ? jm * Y_ST : (S - 1) * Y_ST + (j <= S - 2 ? T_ST : 0)));
      } else {
        const int left = NJ - 1 - j < S - 2 ? NJ - 1 - j : S - 2;
        const int jm = j < S - 1 ? j : S - 1;
        vm_wait(left * n_st + jm * Y_ST);
        if (!SW && j == 0) {  // the biases are older still: pin their first use here
#pragma unroll
          for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) asm volatile("" ::"v"(b3v[jj][jn]));
#pragma unroll
          for (int jn = 0; jn < TN2; ++jn) asm volatile("" ::"v"(b1v[jn]));
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave is done with step j - 1: its slot is free
      {
        const int jn = j + S - 1;  // (constants once the chunk loop is unrolled)
        if (jn < NJ) {
          issue_stage(jn, jn % S, m0);
        } else if (PERS) {
          if (jn == NJ) issue_a1(m0n, smem + (abuf ^ 1) * A1_BYTES);
          issue_stage(jn - NJ, jn % S, m0n);
        }
      }
      char* const sW3 = w3_at(j, j % S);
      char* const sW1 = w1_at(j, j % S);
      char* const sR = r_at(j % S);

      // ---- GEMM1: acc1[BM x CW] = A1 . W3_j^T
      f32x4 acc1[TM][TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) acc1[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
      const uint4* A1s = reinterpret_cast<const uint4*>(sA1);
      const uint4* W3s = reinterpret_cast<const uint4*>(sW3);
#pragma unroll
      for (int kk = 0; kk < 2 * KS; ++kk) {
        const int s = kk >> 1, ch = fq + 4 * (kk & 1);
        bf16x8 af[TM], bfv[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int r = wm * WTM + i * 16 + fr;
          af[i] = __builtin_bit_cast(bf16x8, A1s[s * BM * 8 + r * 8 + (ch ^ (r & 7))]);
        }
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
          const int n = wn * (CW / 2) + jn * 16 + fr;
          bfv[jn] = __builtin_bit_cast(bf16x8, W3s[s * CW * 8 + n * 8 + (ch ^ (n & 7))]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int jn = 0; jn < TN; ++jn)
            acc1[i][jn] = SW ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfv[jn], af[i], acc1[i][jn], 0, 0, 0)
                             : __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfv[jn], acc1[i][jn], 0, 0, 0);
      }

      // ---- pass 1: y = relu(acc1 + b3 (+ res)) -> bf16, in place over the residual chunk
      auto y_at = [&](int row, int col) {  // LDS offset of y[row][col] in the slot's swizzled image
        return lds_off(sR + row * (CW * 2) + (((col >> 3) ^ row_swz<CPR>(row)) << 4) + (col & 7) * 2);
      };
      if constexpr (SW) {
        uint2 rv[TN][TM];
        if (has_res) {
#pragma unroll
          for (int jn = 0; jn < TN; ++jn)
#pragma unroll
            for (int i = 0; i < TM; ++i)
              rv[jn][i] = lds_ld8_issue(y_at(wm * WTM + i * 16 + fr, wn * (CW / 2) + jn * 16 + fq * 4));
#pragma unroll
          for (int jn = 0; jn < TN; ++jn)
#pragma unroll
            for (int i = 0; i < TM; ++i) lds_landed(rv[jn][i]);
        }
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
          const int nt0 = wn * (CW / 2) + jn * 16, col = nt0 + fq * 4;  // col % 8 in {0, 4}: 8 B in one chunk
          const f32x4 bb = bias4(a.b3, j * CW + nt0, fq);
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const int row = wm * WTM + i * 16 + fr;
            float rs[4] = {0.f, 0.f, 0.f, 0.f};
            if (has_res) {
              const bf16x4 r4 = __builtin_bit_cast(bf16x4, rv[jn][i]);
#pragma unroll
              for (int r = 0; r < 4; ++r) rs[r] = (float)r4[r];
            }
            bf16x4 q;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float e = acc1[i][jn][r];  // through a named float (ext-vector element bit-cast hazard)
              q[r] = (bf16)fmaxf(e + bb[r] + rs[r], 0.f);
            }
            lds_st8(y_at(row, col), __builtin_bit_cast(uint2, q));
          }
        }
      } else {
        uint32_t rv[TN][TM][4];
        if (has_res) {
#pragma unroll
          for (int jn = 0; jn < TN; ++jn)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                rv[jn][i][r] = lds_ld2_issue(y_at(wm * WTM + i * 16 + fq * 4 + r, wn * (CW / 2) + jn * 16 + fr));
#pragma unroll
          for (int jn = 0; jn < TN; ++jn)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int r = 0; r < 4; ++r) lds_landed(rv[jn][i][r]);
        }
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
          const int col = wn * (CW / 2) + jn * 16 + fr;
          const float bb = b3v[j][jn];
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = wm * WTM + i * 16 + fq * 4 + r;
              const float e = acc1[i][jn][r];  // through a named float (ext-vector element bit-cast hazard)
              float v = e + bb;
              if (has_res) v += (float)__builtin_bit_cast(bf16, (unsigned short)rv[jn][i][r]);
              lds_st2(y_at(row, col), (bf16)fmaxf(v, 0.f));
            }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();

      // ---- y chunk -> HBM, issued before GEMM2
#pragma unroll
      for (int it = 0; it < Y_ST; ++it) {
        const int q = tid + it * NT;
        const int row = q / CPR, c = q % CPR;
        const uint4 v = lds_ld16(lds_off(sR + row * (CW * 2) + ((c ^ row_swz<CPR>(row)) << 4)));
        const int m = m0 + row;
        int off;
        if constexpr (Y2) {
          off = yro[it] >= 0 ? (yro[it] + j * CW + c * 8) * 2 : OOB;
        } else {
          off = m < a.M ? (m * N1 + j * CW + c * 8) * 2 : OOB;
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), yr, off, 0, 0);
      }

      // ---- GEMM2: acc2[BM x N2] += y_j . W1_j^T
      const uint4* Ys = reinterpret_cast<const uint4*>(sR);
      const uint4* W1s = reinterpret_cast<const uint4*>(sW1);
#pragma unroll
      for (int kk = 0; kk < CW / 32; ++kk) {
        const int ch = fq + 4 * kk;
        bf16x8 af[TM], bfv[TN2];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int r = wm * WTM + i * 16 + fr;
          af[i] = __builtin_bit_cast(bf16x8, Ys[r * CPR + (ch ^ row_swz<CPR>(r))]);
        }
#pragma unroll
        for (int jn = 0; jn < TN2; ++jn) {
          const int n = wn * (N2 / 2) + jn * 16 + fr;
          bfv[jn] = __builtin_bit_cast(bf16x8, W1s[n * CPR + (ch ^ row_swz<CPR>(n))]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int jn = 0; jn < TN2; ++jn)
            acc2[i][jn] = SW ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfv[jn], af[i], acc2[i][jn], 0, 0, 0)
                             : __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfv[jn], acc2[i][jn], 0, 0, 0);
      }
    }

    // ---- t1 = relu(acc2 + b1) -> bf16 tile in LDS -> 16-B stores
    constexpr int TPR = N2 / 8;
    bf16* to = reinterpret_cast<bf16*>(smem + (PERS ? OFF_EPI : 0));
    if constexpr (!PERS) {  // the staging tile lies over the ring: every wave must be done reading it
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    if constexpr (SW) {
#pragma unroll
      for (int jn = 0; jn < TN2; ++jn) {
        const int nt0 = wn * (N2 / 2) + jn * 16, col = nt0 + fq * 4;
        const f32x4 bb = bias4(a.b1, nt0, fq);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = wm * WTM + i * 16 + fr;
          bf16x4 q;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = acc2[i][jn][r];
            q[r] = (bf16)fmaxf(e + bb[r], 0.f);
          }
          lds_st8(lds_off(to + row * N2 + ((((col >> 3) ^ (row & 7))) << 3) + (col & 7)), __builtin_bit_cast(uint2, q));
        }
      }
    } else {
#pragma unroll
      for (int jn = 0; jn < TN2; ++jn) {
        const int col = wn * (N2 / 2) + jn * 16 + fr;
        const float bb = b1v[jn];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = wm * WTM + i * 16 + fq * 4 + r;
            const float e = acc2[i][jn][r];
            lds_st2(lds_off(to + row * N2 + ((((col >> 3) ^ (row & 7))) << 3) + (col & 7)), (bf16)fmaxf(e + bb, 0.f));
          }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int it = 0; it < T_ST; ++it) {
      const int q = tid + it * NT;
      const int row = q / TPR, c = q - (q / TPR) * TPR;
      const uint4 v = lds_ld16(lds_off(to + row * N2 + ((c ^ (row & 7)) << 3)));
      const int m = m0 + row;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), tr,
                                             m < a.M ? (m * a.N2 + c * 8) * 2 : OOB, 0, 0);
    }
    if constexpr (!PERS) break;
    tile = chain_next_tile(tile, G);
    if (tile >= ntiles) break;
    m0 = m0n;
    abuf ^= 1;
    first = false;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int jn = 0; jn < TN2; ++jn) acc2[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // the loads issued past the last tile target this block's LDS: retire them before it is released
  if constexpr (PERS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The ResNet-50 boundaries (BM = 128):          KS   N1   N2  CW
//   layer1.0 (dual) -> layer1.1                  2   256   64  64
//   layer1.1 -> layer1.2                         1   256   64  64
//   layer1.2 -> layer2.0                         1   256  128  64
//   layer2.1 -> 2.2, 2.2 -> 2.3                  2   512  128  64 (or 32: 80 KB, two blocks per CU)
//   layer2.3 -> layer3.0                         2   512  256  32
//   layer3.1 -> 3.2 ... layer3.4 -> 3.5          4  1024  256  32
template <int KS, int N1, int N2, int CW, int BM = 128, bool C2 = false, bool Y2 = false>
int launch_chain(const ChainArgs& a, hipStream_t st) {
  constexpr int LDS = BM * KS * 128 + 2 * (CW * KS * 128 + N2 * CW * 2 + BM * CW * 2);
  constexpr int OCC = LDS <= 80 * 1024 ? 4 : 2;
#ifdef MLS_CHAIN_SWAP
  constexpr bool SW = MLS_CHAIN_SWAP;
#else
  constexpr bool SW = KS == 1;
#endif
  hipLaunchKernelGGL((conv_chain_kernel<BM, KS, N1, N2, CW, OCC, SW, C2, Y2>), dim3((unsigned)((a.M + BM - 1) / BM)),
                     dim3(512), 0, st, a);
  return (int)hipGetLastError();
}

int g_chain_grid = 0;  // persistent form's block count (0 = one per CU; mls_chain_set_grid, tests)

// The ring kernel's instantiations.                         BM  KS   N1   N2  CW  S   LDS
//   layer1.0 (dual) -> layer1.1          PERS              64   2   256   64  64  2  152 KB
//   layer2.1 -> 2.2, 2.2 -> 2.3                           128   2   512  128  64  2  128 KB
//   layer2.3 -> layer3.0                                  128   2   512  256  32  3  128 KB
// PERS: 64-row tiles (1568 at B = 32, 6.1 per block of a 256-block grid where 784 tiles of 128 rows
// leave a 4-versus-3 imbalance); the grid is one block per CU, capped by the tile count.  The
// single-slab layer1 boundaries (1, 256, 64) and (1, 256, 128) measured no faster in either form
// (docs/PERF_NOTES.md) and stay with conv_chain_kernel under every variant.
// Only the second row is a default.  The other two are level with 4 copies co-running, which is how
// the engine normally runs, but faster alone (36.9 -> 29.0 us and 29.0 -> 27.5 us): they are kept
// for one-batch-at-a-time serving (bench.py --serial, an engine with inflight = 1), which selects
// them with MLS_CHAIN_VARIANT=2.
template <int BM, int KS, int N1, int N2, int CW, int S, bool PERS, bool Y2 = false>
int launch_ring(const ChainArgs& a, hipStream_t st) {
#ifdef MLS_CHAIN_SWAP
  constexpr bool SW = MLS_CHAIN_SWAP;
#else
  constexpr bool SW = KS == 1;
#endif
  constexpr int LDS = PERS ? 2 * BM * KS * 128 + N1 * KS * 128 + N2 * N1 * 2 + BM * N2 * 2 + S * BM * CW * 2
                            : BM * KS * 128 + S * (CW * KS * 128 + N2 * CW * 2 + BM * CW * 2);
  constexpr int OCC = LDS <= 80 * 1024 ? 4 : 2;
  const int ntiles = (a.M + BM - 1) / BM;
  int grid = ntiles;
  if (PERS) {
    const int cus = mls_num_cus();
    grid = g_chain_grid > 0 ? g_chain_grid : (ntiles < cus ? ntiles : cus);
  }
  hipLaunchKernelGGL((conv_chain_ring_kernel<BM, KS, N1, N2, CW, S, OCC, SW, PERS, Y2>), dim3((unsigned)grid), dim3(512), 0,
                     st, a, ntiles);
  return (int)hipGetLastError();
}

int g_chain_cw_l2 = 0;  // layer2 chunk width override (0 = default 64; mls_chain_set_l2_cw for A/B)
int g_chain_bm_l2 = 128;  // layer2 boundaries' row tile (64: 392 blocks instead of 196 at B = 32)
int g_chain_variant = 0;  // 0 = per-shape default, 1 = conv_chain_kernel, 2 = conv_chain_ring_kernel

// Per-shape default (variant 0): the ring / persistent form where it measured faster with 4 copies
// co-running (docs/PERF_NOTES.md, "conv_chain: deeper ring, persistent tiles").
constexpr bool RING_L1_DUAL = false, RING_L2 = true, RING_L2_OUT = false;

bool use_ring(bool shape_default) { return g_chain_variant == 2 || (g_chain_variant == 0 && shape_default); }

// bytes of y: [M][N1], or with y2 (the Y2 store, even Ho and Wo) [B][Ho / 2][Wo / 2][N1]
long y_size(int B, int Ho, int Wo, int N1, bool y2) {
  return y2 ? (long)B * (Ho / 2) * (Wo / 2) * N1 * 2 : (long)B * Ho * Wo * N1 * 2;
}

// mls_conv_chain (y2 = false) and mls_conv_chain_y2 (y2 = true: the Y2 store, below):
// y = relu(conv1x1([a1 | a2 strided]) + b3 (+ res)); t1 = relu(conv1x1(y, w1) + b1).
// a1 [M][Ka] (M = B*Ho*Wo), a2 [B][H2][W2][Kb] sampled at stride2 (Kb = 0: none), w3 [N1][Ka+Kb],
// res [M][N1] or null, w1 [N2][N1]; y [M][N1], t1 [M][N2].  (KS = (Ka + Kb) / 64, N1, N2) one of
// (1, 256, 64), (2, 256, 64), (1, 256, 128), (2, 512, 128), (2, 512, 256), (4, 1024, 256);
// anything else MLS_UNSUPPORTED.
int chain_impl(const void* a1, const void* a2, const void* w3, const float* b3, const void* res, void* y,
               const void* w1, const float* b1, void* t1, int B, int Ho, int Wo, int Ka, int H2, int W2, int Kb,
               int stride2, int N1, int N2, bool y2, void* stream) {
  if (B <= 0 || Ho <= 0 || Wo <= 0 || Ka <= 0 || Ka % 64 || Kb < 0 || Kb % 64 || N1 <= 0 || N1 % 64 || N2 <= 0)
    return MLS_BAD_ARG;
  if (Kb > 0 && (stride2 < 1 || (Ho - 1) * stride2 >= H2 || (Wo - 1) * stride2 >= W2 || res)) return MLS_BAD_ARG;
  if (y2 && (Ho % 2 || Wo % 2)) return MLS_UNSUPPORTED;
  ChainArgs a{};
  a.a1 = (const bf16*)a1;
  a.a2 = (const bf16*)a2;
  a.w3 = (const bf16*)w3;
  a.b3 = b3;
  a.res = (const bf16*)res;
  a.y = (bf16*)y;
  a.w1 = (const bf16*)w1;
  a.b1 = b1;
  a.t1 = (bf16*)t1;
  a.M = B * Ho * Wo;
  a.Ka = Ka;
  a.Kb = Kb;
  a.N1 = N1;
  a.N2 = N2;
  a.Ho = Ho, a.Wo = Wo, a.H2 = H2, a.W2 = W2, a.stride2 = stride2;
  a.fd_howo = fastdiv_make((uint32_t)(Ho * Wo));
  a.fd_wo = fastdiv_make((uint32_t)Wo);
  const long M = a.M;
  const long sizes[7] = {M * Ka * 2, (long)B * H2 * W2 * Kb * 2, (long)N1 * (Ka + Kb) * 2, res ? M * N1 * 2 : 0,
                         y_size(B, Ho, Wo, N1, y2), (long)N2 * N1 * 2, M * N2 * 2};
  for (long s : sizes)
    if (s >= 0x7fffffffL) return MLS_UNSUPPORTED;
  a.a1_bytes = (uint32_t)sizes[0];
  a.a2_bytes = (uint32_t)sizes[1];
  a.w3_bytes = (uint32_t)sizes[2];
  a.res_bytes = (uint32_t)sizes[3];
  a.y_bytes = (uint32_t)sizes[4];
  a.w1_bytes = (uint32_t)sizes[5];
  a.t1_bytes = (uint32_t)sizes[6];
  const hipStream_t st = (hipStream_t)stream;
  const int ks = (Ka + Kb) / 64;
  if (y2) {  // the stride-2 stage boundaries; the layer2 A/B overrides do not apply
    if (ks == 1 && N1 == 256 && N2 == 128) return launch_chain<1, 256, 128, 64, 128, false, true>(a, st);
    if (ks == 2 && N1 == 512 && N2 == 256)
      return use_ring(RING_L2_OUT) ? launch_ring<128, 2, 512, 256, 32, 3, false, true>(a, st)
                                   : launch_chain<2, 512, 256, 32, 128, false, true>(a, st);
    return MLS_UNSUPPORTED;
  }
  if (ks == 1 && N1 == 256 && N2 == 64) return launch_chain<1, 256, 64, 64>(a, st);
  if (ks == 2 && N1 == 256 && N2 == 64)
    return use_ring(RING_L1_DUAL) ? launch_ring<64, 2, 256, 64, 64, 2, true>(a, st)
                                  : launch_chain<2, 256, 64, 64>(a, st);
  if (ks == 1 && N1 == 256 && N2 == 128) return launch_chain<1, 256, 128, 64>(a, st);
  // the layer2 A/B overrides keep selecting conv_chain_kernel's instantiations under variant 0
  const bool l2_override = g_chain_variant == 0 && (g_chain_bm_l2 == 64 || g_chain_cw_l2 != 0);
  if (ks == 2 && N1 == 512 && N2 == 128) {
    if (!l2_override && use_ring(RING_L2)) return launch_ring<128, 2, 512, 128, 64, 2, false>(a, st);
    if (g_chain_bm_l2 == 64) return launch_chain<2, 512, 128, 64, 64>(a, st);
    return g_chain_cw_l2 == 32 ? launch_chain<2, 512, 128, 32>(a, st) : launch_chain<2, 512, 128, 64>(a, st);
  }
  if (ks == 2 && N1 == 512 && N2 == 256) {
    if (!l2_override && use_ring(RING_L2_OUT)) return launch_ring<128, 2, 512, 256, 32, 3, false>(a, st);
    return g_chain_bm_l2 == 64 ? launch_chain<2, 512, 256, 64, 64>(a, st) : launch_chain<2, 512, 256, 32>(a, st);
  }
  if (ks == 4 && N1 == 1024 && N2 == 256) return launch_chain<4, 1024, 256, 32>(a, st);
  return MLS_UNSUPPORTED;
}

// mls_conv_chain_conv2 / mls_conv_chain_conv2_y2: mls_conv_chain with the bottleneck's conv2 in the
// same kernel:
//   t2 = relu(conv3x3(t1_in, w2) + b2)   (stride 1, pad 1; never written to memory)
//   y  = relu(conv1x1([t2 | a2 strided]) + b3 (+ res)); t1 = relu(conv1x1(y, w1) + b1).
// t1_in [B][H][W][64], w2 [64][3][3][64] (the packed conv weight), b2 [64] or null; the rest as
// mls_conv_chain with a1 = t2 (Ka = 64, Ho = H, Wo = W).  (KS, N1, N2) one of the layer1 boundaries
// (1, 256, 64), (2, 256, 64), (1, 256, 128) and W <= 63 (the tile's pixel strip with its halo of
// W + 1 on both sides is staged as 256 LDS rows); anything else MLS_UNSUPPORTED.
int chain_conv2_impl(const void* t1_in, const void* w2, const float* b2, const void* a2, const void* w3,
                     const float* b3, const void* res, void* y, const void* w1, const float* b1, void* t1, int B, int H,
                     int W, int Ka, int H2, int W2, int Kb, int stride2, int N1, int N2, bool y2, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || Ka <= 0 || Kb < 0 || Kb % 64 || N1 <= 0 || N1 % 64 || N2 <= 0) return MLS_BAD_ARG;
  if (Kb > 0 && (stride2 < 1 || (H - 1) * stride2 >= H2 || (W - 1) * stride2 >= W2 || res)) return MLS_BAD_ARG;
  if (Ka != 64 || 2 * (W + 1) + 128 > 256) return MLS_UNSUPPORTED;
  if (y2 && (H % 2 || W % 2)) return MLS_UNSUPPORTED;
  ChainArgs a{};
  a.t1in = (const bf16*)t1_in;
  a.w2 = (const bf16*)w2;
  a.b2 = b2;
  a.a2 = (const bf16*)a2;
  a.w3 = (const bf16*)w3;
  a.b3 = b3;
  a.res = (const bf16*)res;
  a.y = (bf16*)y;
  a.w1 = (const bf16*)w1;
  a.b1 = b1;
  a.t1 = (bf16*)t1;
  a.Ka = Ka;
  a.Kb = Kb;
  a.N1 = N1;
  a.N2 = N2;
  a.Ho = H, a.Wo = W, a.H2 = H2, a.W2 = W2, a.stride2 = stride2;
  a.fd_howo = fastdiv_make((uint32_t)(H * W));
  a.fd_wo = fastdiv_make((uint32_t)W);
  const long M = (long)B * H * W;
  const long sizes[7] = {M * Ka * 2, (long)B * H2 * W2 * Kb * 2, (long)N1 * (Ka + Kb) * 2, res ? M * N1 * 2 : 0,
                         y_size(B, H, W, N1, y2), (long)N2 * N1 * 2, M * N2 * 2};
  for (long s : sizes)
    if (s >= 0x7fffffffL) return MLS_UNSUPPORTED;
  a.M = (int)M;
  a.t1in_bytes = (uint32_t)sizes[0];
  a.a2_bytes = (uint32_t)sizes[1];
  a.w3_bytes = (uint32_t)sizes[2];
  a.res_bytes = (uint32_t)sizes[3];
  a.y_bytes = (uint32_t)sizes[4];
  a.w1_bytes = (uint32_t)sizes[5];
  a.t1_bytes = (uint32_t)sizes[6];
  a.w2_bytes = 64 * 9 * 64 * 2;
  const hipStream_t st = (hipStream_t)stream;
  const int ks = (Ka + Kb) / 64;
  if (y2) return ks == 1 && N1 == 256 && N2 == 128 ? launch_chain<1, 256, 128, 64, 128, true, true>(a, st) : MLS_UNSUPPORTED;
  if (ks == 1 && N1 == 256 && N2 == 64) return launch_chain<1, 256, 64, 64, 128, true>(a, st);
  if (ks == 2 && N1 == 256 && N2 == 64) return launch_chain<2, 256, 64, 64, 128, true>(a, st);
  if (ks == 1 && N1 == 256 && N2 == 128) return launch_chain<1, 256, 128, 64, 128, true>(a, st);
  return MLS_UNSUPPORTED;
}

}  // namespace

extern "C" {

// chain_impl / chain_conv2_impl above, y stored in full
int mls_conv_chain(const void* a1, const void* a2, const void* w3, const float* b3, const void* res, void* y,
                   const void* w1, const float* b1, void* t1, int B, int Ho, int Wo, int Ka, int H2, int W2, int Kb,
                   int stride2, int N1, int N2, void* stream) {
  return chain_impl(a1, a2, w3, b3, res, y, w1, b1, t1, B, Ho, Wo, Ka, H2, W2, Kb, stride2, N1, N2, false, stream);
}

int mls_conv_chain_conv2(const void* t1_in, const void* w2, const float* b2, const void* a2, const void* w3,
                         const float* b3, const void* res, void* y, const void* w1, const float* b1, void* t1, int B,
                         int H, int W, int Ka, int H2, int W2, int Kb, int stride2, int N1, int N2, void* stream) {
  return chain_conv2_impl(t1_in, w2, b2, a2, w3, b3, res, y, w1, b1, t1, B, H, W, Ka, H2, W2, Kb, stride2, N1, N2,
                          false, stream);
}

// The same two with the Y2 store: y is [B][Ho / 2][Wo / 2][N1], the pixels (2i, 2j) of the block
// output -- all that a stride-2 downsample projection reads of it.  t1 is unchanged.  Ho and Wo
// even and (KS, N1, N2) one of the stride-2 stage boundaries, (1, 256, 128) (both entry points) and
// (2, 512, 256) (mls_conv_chain_y2); anything else MLS_UNSUPPORTED, nothing launched.
int mls_conv_chain_y2(const void* a1, const void* a2, const void* w3, const float* b3, const void* res, void* y,
                      const void* w1, const float* b1, void* t1, int B, int Ho, int Wo, int Ka, int H2, int W2, int Kb,
                      int stride2, int N1, int N2, void* stream) {
  return chain_impl(a1, a2, w3, b3, res, y, w1, b1, t1, B, Ho, Wo, Ka, H2, W2, Kb, stride2, N1, N2, true, stream);
}

int mls_conv_chain_conv2_y2(const void* t1_in, const void* w2, const float* b2, const void* a2, const void* w3,
                            const float* b3, const void* res, void* y, const void* w1, const float* b1, void* t1,
                            int B, int H, int W, int Ka, int H2, int W2, int Kb, int stride2, int N1, int N2,
                            void* stream) {
  return chain_conv2_impl(t1_in, w2, b2, a2, w3, b3, res, y, w1, b1, t1, B, H, W, Ka, H2, W2, Kb, stride2, N1, N2,
                          true, stream);
}

// A/B switch for the layer2 boundaries' chunk width (64 = 128 KB of LDS, one block per CU; 32 =
// 80 KB, two per CU).
void mls_chain_set_l2_cw(int cw) { g_chain_cw_l2 = (cw == 32 || cw == 64) ? cw : 0; }

// A/B switch for the layer2 boundaries' row tile: 128 (default) or 64 (twice the blocks).
void mls_chain_set_l2_bm(int bm) { g_chain_bm_l2 = bm == 64 ? 64 : 128; }


// Which kernel a boundary runs: 0 = the per-shape default, 1 = conv_chain_kernel everywhere, 2 =
// conv_chain_ring_kernel wherever it is instantiated (the dual layer1 boundary and layer2).
void mls_chain_set_variant(int v) { g_chain_variant = (v == 1 || v == 2) ? v : 0; }

// Test hook: the persistent form's block count (0 = automatic).  Any count is correct; blocks
// beyond the tile count find no tile and leave.
void mls_chain_set_grid(int g) { g_chain_grid = g > 0 ? g : 0; }

}  // extern "C"

MLS_DEBUG_EXPORT(conv_chain)
