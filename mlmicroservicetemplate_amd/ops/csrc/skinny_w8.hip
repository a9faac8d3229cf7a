// W8A8 skinny GEMM for decode (M <= 16) on ops.pack_w8's row-major [N][K] e4m3 codes as they are:
//     out[M][N] = act((Hq[M][K] . Wq[N][K]^T) * hs[m] (* rstd[m]) * ws[n] + bias[N]) (+ residual[M][N])
// on v_mfma_scale_f32_16x16x128_f8f6f4 with every E8M0 block scale 2^0, as gemm_w8a8.hip -- but with no LDS
// ring and no K split across blocks: the weights stream global -> VGPR, once, and the launch is deterministic.
//
// Work split: a block owns NT 16-channel tiles (the last block's may run past N: those rows read as zero
// through the buffer range check and are not stored) and all of K.  Its NWV waves take the 128-k steps
// round-robin (wave w: steps w, w + NWV, ...: neighbouring waves read neighbouring cache lines, and 17 steps
// over 8 waves is 3 2 2 ... not 3 3 3 3 3 2 0 0) and their partial tiles meet in LDS (sk_reduce_store).
//
// Operands: the weight tile is the MFMA's FIRST operand, so lane (fr = lane & 15, fq = lane >> 4) ends up with
// the 4 channels n0 + 4 fq .. + 3 of row fr.  Per step that lane reads the 32 bytes k = 32 fq .. + 32 of weight
// row n0 + fr -- two non-temporal 16-B buffer loads, sixteen rows x 128 B = sixteen whole cache lines per tile and
// step -- and the SAME 32 bytes of activation row fr: the instruction pairs byte b of k group fq of one operand
// with byte b of k group fq of the other, so any choice works as long as both operands make it
// (tests/test_skinny_w8_gpu.py pins it with one-hot rows).  gemm_w8a8.hip reads 16 fq and 64 + 16 fq instead,
// which suits its LDS rows; the contiguous 32 suit row-major global reads.
//
// k loop: UN steps x NT tiles of weight fragments per trip, register double-buffered (the next trip's loads are
// issued before this trip's MFMAs); steps past a wave's last are loads at the out-of-range offset, not branches
// (skinny_tiles.h: a runtime branch in the unrolled body drains vmcnt per step).  One activation fragment
// feeds the NT MFMAs of its step.
//
// Activations, one kernel text (FUSED):
//  * fused: bf16 rows x (+ delta).  Prologue, every block: h = bf16(x + delta) in registers (block 0 writes it
//    to resid_out), max|h| and the square sum reduced per row in a fixed order (16-lane DPP, then 16 lanes per
//    row over the partials in LDS), the e4m3 codes of h by w8_quant.h's rule into an LDS image [M][K + 16] (the
//    16-B pad puts the 16 rows of a fragment read on 16 different bank groups), fragments read from there.  Only
//    the one-byte image lives in LDS; the bf16 rows stay in registers between the two passes, which bounds
//    M K at 32768 (8 chunks of 8 per thread at 512 threads).
//  * codes: (xq, xs) of mls_quant_rows_fp8, fragments global -> VGPR beside the weights (few rows, L2-resident),
//    any K.
#include "skinny_tiles.h"
#include "w8_quant.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int S8_PAD = 16;             // bytes between the rows of the LDS code image
constexpr int S8_FUSED_ELEMS = 32768;  // M K the fused prologue holds in registers

struct S8Args {
  const void* x;       // fused: bf16 [M][K]; codes: e4m3 [M][K]
  const bf16* delta;   // fused, optional: bf16 [M][K] added to x
  bf16* resid_out;     // fused, optional: <- bf16(x + delta), written by block 0
  const float* xs;     // codes: [M] row scales
  const uint8_t* w;    // [N][K] e4m3
  const float* wsc;    // [N]
  SkEpi e;             // bias, res, out, M, N, K, ldo, act, eps
  uint32_t x_bytes, w_bytes;
  int norm;            // fused: row scale *= rsqrt(mean(h^2) + eps)
  FastDiv fd_kch;      // K / 8 chunks per row
};

MLS_DEV float group_max16(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  return fmaxf(v, dpp_f<0x140>(v));
}

MLS_DEV float absmax8(uint4 v) {
  float x[8];
  unpack8(v, x);
  float r = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) r = fmaxf(r, fabsf(x[e]));
  return r;
}

// a barrier behind LDS writes alone: __syncthreads would also drain the weight trip in flight
MLS_DEV void s8_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

MLS_DEV i32x8 s8_frag(uint4 lo, uint4 hi) {
  return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

template <int NT, int UN, int NWV, bool FUSED>
__global__ __launch_bounds__(NWV * 64) void skinny_w8_kernel(const S8Args s) {
  extern __shared__ __attribute__((aligned(16))) char img[];  // FUSED: [M][K + S8_PAD] e4m3 codes of h
  __shared__ float red[NWV][16][NT * 16 + 1];
  __shared__ float row_scale[16];
  constexpr int T = NWV * 64;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * NT * 16;
  const int M = s.e.M, N = s.e.N, K = s.e.K;
  const int nk = K >> 7;
  const int cnt = wid < nk ? (nk - wid + NWV - 1) / NWV : 0;  // this wave's steps: wid + NWV i, i < cnt
  const rsrc_t wr = make_rsrc(s.w, s.w_bytes);
  const rsrc_t xr = make_rsrc(s.x, s.x_bytes);
  int wbase[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) wbase[j] = n0 + 16 * j + fr < N ? (n0 + 16 * j + fr) * K + 32 * fq : OOB;
  const bool arow = fr < M;
  const int abase = arow ? fr * K + 32 * fq : OOB;  // codes form

  struct Trip {
    uint4 w[UN][NT][2];
    uint4 a[FUSED ? 1 : UN][2];
  };
  auto load_trip = [&](int i0, Trip& tr) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const bool in = i0 + u < cnt;
      const int kb = (wid + NWV * (i0 + u)) * 128;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int off = (in && wbase[j] != OOB) ? wbase[j] + kb : OOB;
        tr.w[u][j][0] = bload16_pol<1>(wr, off);
        tr.w[u][j][1] = bload16_pol<1>(wr, off == OOB ? OOB : off + 16);
      }
      if constexpr (!FUSED) {
        const int off = (in && arow) ? abase + kb : OOB;
        tr.a[u][0] = bload16(xr, off);
        tr.a[u][1] = bload16(xr, off == OOB ? OOB : off + 16);
      }
    }
  };

  Trip nxt;
  const int pitch = K + S8_PAD;
  if constexpr (FUSED) {
    __shared__ float pmax[S8_FUSED_ELEMS / 128], pssq[S8_FUSED_ELEMS / 128];  // one per 16 chunks of 8
    __shared__ float row_inv[16];
    constexpr int HC = S8_FUSED_ELEMS / 8 / T;  // chunks per thread
    const int kch = K >> 3, nq = M * kch;
    const rsrc_t dr = make_rsrc(s.delta, s.delta ? s.x_bytes : 0);
    const bool wr_res = s.resid_out && blockIdx.x == 0;
    // x is contiguous: chunk q = tid + j T is bytes 16 q; the rows' loads go out before the first weight trip
    // (the vector memory counter retires in order, so consuming them does not wait for the weights)
    uint4 h[HC], d[HC];
#pragma unroll
    for (int j = 0; j < HC; ++j) {
      const int q = tid + j * T;
      h[j] = bload16(xr, q < nq ? q * 16 : OOB);
      if (s.delta) d[j] = bload16(dr, q < nq ? q * 16 : OOB);
    }
    load_trip(0, nxt);
#pragma unroll
    for (int j = 0; j < HC; ++j) {
      const int q = tid + j * T;
      if (s.delta) {
        h[j] = add_round(h[j], d[j]);
        if (wr_res && q < nq) st16(s.resid_out + (size_t)q * 8, h[j]);
      }
      // K % 128 == 0: the 16 lanes of a group hold 16 chunks of one row
      const float am = group_max16(absmax8(h[j])), sq = group_sum<16>(sumsq8(h[j]));
      if (fr == 0 && q < nq) {
        pmax[q >> 4] = am;
        pssq[q >> 4] = sq;
      }
    }
    s8_lds_barrier();
    if (tid < 256) {  // 16 lanes per row over its K / 128 partials, in a fixed order
      const int m = tid >> 4, k16 = kch >> 4;
      float am = 0.f, sq = 0.f;
      if (m < M)
        for (int g = fr; g < k16; g += 16) {
          am = fmaxf(am, pmax[m * k16 + g]);
          sq += pssq[m * k16 + g];
        }
      am = group_max16(am);
      sq = group_sum<16>(sq);
      if (fr == 0 && m < M) {
        const float sc = w8_row_scale(am);
        row_inv[m] = 1.f / sc;
        row_scale[m] = s.norm ? sc * sk_rstd(sq, s.e) : sc;
      }
    }
    s8_lds_barrier();
#pragma unroll
    for (int j = 0; j < HC; ++j) {
      const int q = tid + j * T;
      if (q < nq) {
        const int m = fastdiv(q, s.fd_kch), c = q - m * kch;
        *reinterpret_cast<int2*>(img + m * pitch + c * 8) = w8_codes8(h[j], row_inv[m]);
      }
    }
    s8_lds_barrier();
  } else {
    load_trip(0, nxt);
    if (tid < M) row_scale[tid] = s.xs[tid];
  }

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* arow_lds = img + fr * pitch + 32 * fq;

  for (int i = 0; i < cnt; i += UN) {
    Trip cur = nxt;
    if (i + UN < cnt) load_trip(i + UN, nxt);
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      i32x8 af;
      if constexpr (FUSED) {
        const bool rd = arow && i + u < cnt;  // lanes of rows >= M read nothing
        const char* p = arow_lds + (wid + NWV * (i + u)) * 128;
        const uint4 z = make_uint4(0, 0, 0, 0);
        af = s8_frag(rd ? *reinterpret_cast<const uint4*>(p) : z, rd ? *reinterpret_cast<const uint4*>(p + 16) : z);
      } else {
        af = s8_frag(cur.a[u][0], cur.a[u][1]);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(s8_frag(cur.w[u][j][0], cur.w[u][j][1]), af, acc[j], 0,
                                                                  0, 0, W8_E8M0_ONE, 0, W8_E8M0_ONE);
    }
  }

  // acc[j][i] = sum over this wave's steps of out[m = fr][n = n0 + 16 j + 4 fq + i]
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wid][fr][16 * j + 4 * fq + i] = acc[j][i];
  __syncthreads();
  sk_reduce_store<NWV, 16, NT * 16, false, true>(
      red, s.e, n0, [&](int m) { return row_scale[m]; }, [&](int n) { return s.wsc[n]; });
}

// launch shapes: (column tiles per block, k-steps per trip, waves)
struct S8Shape {
  int nt, un, nw;
};
constexpr S8Shape S8_SHAPES[] = {
    {0, 0, 0},   // 0: by shape
    {2, 2, 8},   // 1
    {2, 2, 16},  // 2
    {4, 1, 8},   // 3
    {4, 2, 8},   // 4
    {1, 4, 8},   // 5
    {1, 2, 16},  // 6
};
constexpr int S8_NVARIANTS = sizeof(S8_SHAPES) / sizeof(S8_SHAPES[0]);

// by shape, measured on the Llama-3-8B projections (profiles/w8a8_skinny_ab.jsonl): one tile per block until the
// tiles outnumber the CUs 1.5 times (o, down: 256 tiles -- two tiles per block would leave half the CUs idle, 22.8
// against 14.8 us on down), 16 waves where 8 would walk more than 8 steps each; two tiles on 16 waves up to 4
// tiles per CU (qkv), four tiles and one step per trip above (gate_up: 27.2 against 30.4 us with two steps)
int s8_pick(int N, int K) {
  const int tiles = N / 16, cus = mls_num_cus(), nk = K / 128;
  if (tiles >= 4 * cus) return 3;
  if (2 * tiles >= 3 * cus) return 2;
  return nk > 64 ? 6 : 5;
}

// the fused form's limit (ops.skinny_w8_fused_fits): the prologue keeps the bf16 rows in registers
bool s8_fused_fits(int M, int K) { return (long long)M * K <= S8_FUSED_ELEMS; }

template <int NT, int UN, int NWV>
void s8_launch(const S8Args& s, bool fused, hipStream_t st) {
  const dim3 grid((s.e.N / 16 + NT - 1) / NT), block(NWV * 64);
  if (fused)
    hipLaunchKernelGGL((skinny_w8_kernel<NT, UN, NWV, true>), grid, block, (size_t)s.e.M * (s.e.K + S8_PAD), st, s);
  else
    hipLaunchKernelGGL((skinny_w8_kernel<NT, UN, NWV, false>), grid, block, 0, st, s);
}

}  // namespace

extern "C" {

int mls_skinny_w8_num_variants() { return S8_NVARIANTS; }

// W8A8 decode GEMM, M <= 16, N % 16 == 0, K % 128 == 0, on pack_w8's [N][K] codes.  xs == nullptr: the fused
// form, x bf16 [M][K] (+ delta, -> resid_out; norm), with M K <= 32768; else the codes form, x the
// e4m3 codes and xs the row scales of mls_quant_rows_fp8 (delta / resid_out / norm must be unset).
// variant: an index into S8_SHAPES, 0: by shape.
int mls_skinny_w8(const void* x, const void* xs, const void* delta, void* resid_out, const void* Wq, const void* wsc,
                  const float* bias, const void* res, void* out, int M, int N, int K, int act, int norm, float eps,
                  int variant, void* stream) {
  if (M <= 0 || M > 16 || N <= 0 || N % 16 || K <= 0 || K % 128) return MLS_BAD_ARG;
  if (!x || !Wq || !wsc || !out || variant < 0 || variant >= S8_NVARIANTS) return MLS_BAD_ARG;
  if (act != ACT_NONE && act != ACT_SILU_MUL) return MLS_BAD_ARG;
  if (res && act == ACT_SILU_MUL) return MLS_BAD_ARG;
  const bool fused = xs == nullptr;
  if (!fused && (delta || resid_out || norm)) return MLS_BAD_ARG;
  if (resid_out && (!delta || resid_out == x || resid_out == delta)) return MLS_BAD_ARG;
  if (fused && !s8_fused_fits(M, K)) return MLS_UNSUPPORTED;
  const size_t wb = (size_t)N * K;
  if (wb >= 0x7FFFFFFFull) return MLS_UNSUPPORTED;  // operand offsets are 32-bit
  S8Args s{};
  s.x = x;
  s.delta = (const bf16*)delta;
  s.resid_out = (bf16*)resid_out;
  s.xs = (const float*)xs;
  s.w = (const uint8_t*)Wq;
  s.wsc = (const float*)wsc;
  s.e = sk_epi(bias, res, out, M, N, K, act, eps);
  s.x_bytes = (uint32_t)((size_t)M * K * (fused ? 2 : 1));
  s.w_bytes = (uint32_t)wb;
  s.norm = norm;
  s.fd_kch = fastdiv_make((uint32_t)(K >> 3));
  const S8Shape sh = S8_SHAPES[variant ? variant : s8_pick(N, K)];
  hipStream_t st = (hipStream_t)stream;
  if (sh.nt == 4) {
    if (sh.un == 2) s8_launch<4, 2, 8>(s, fused, st);
    else s8_launch<4, 1, 8>(s, fused, st);
  } else if (sh.nt == 2) {
    if (sh.nw == 16) s8_launch<2, 2, 16>(s, fused, st);
    else s8_launch<2, 2, 8>(s, fused, st);
  } else {
    if (sh.nw == 16) s8_launch<1, 2, 16>(s, fused, st);
    else s8_launch<1, 4, 8>(s, fused, st);
  }
  return hipGetLastError() == hipSuccess ? MLS_OK : MLS_BAD_ARG;
}

}  // extern "C"
