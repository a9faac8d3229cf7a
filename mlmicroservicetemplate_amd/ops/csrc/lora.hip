// Per-request LoRA on the fused q/k/v projection: qkv[m, seg_p] += s_p * B_p (A_p . RMSNorm(r[m]) * gain)
// for the adapter a = lora_slot[slot of m's sequence], p in {q, k, v}; a = -1 rows are the base model's and
// are neither read nor written.  Two launches per layer, both reading device arrays only (capturable):
//
//  mls_lora_shrink   t[m][0:R] = sum_k r[m][k] A'[a][j][k], A' = bf16(A diag(gain)) packed [adapter][rcap][K]
//                    with the q, k, v ranks padded to LORA_GRAN zero rows and laid end to end (R = their
//                    sum <= rcap), plus the row's square sum, from the same pass over r.  A work tile is <= 16
//                    consecutive rows of ONE sequence (they share an adapter): one 16-row MFMA operand; a
//                    decode row is one lane column of it, the other 15 load nothing (buffer range check).
//                    Split-K over blockIdx.y, 64 columns of t per blockIdx.z; the block's 4 waves take
//                    every 4th k-step of the slice and meet in LDS.  Partials: fp32 slabs
//                    [split][row][rcap + 1] (square sum in the last column), plain stores, no atomics.
//  mls_lora_expand   sums the slabs in split order, rstd = rsqrt(ssq / K + eps), and per 16-column tile of
//                    qkv (a wave each) multiplies t's slice of the tile's segment (bf16 operand) by
//                    B[a] [N][rb] (zero-padded ranks), scales the fp32 accumulator by s_p * rstd and adds
//                    into qkv in place.
//
// v_mfma_f32_16x16x32_bf16 operand maps as in mgemm.hip: lane (fr = lane & 15, fq = lane >> 4) holds
// X[row fr][k 8 fq ..] and W[col fr][k 8 fq ..]; acc[i] is D[row 4 fq + i][col fr].
#include "common.h"
#include "skinny_tiles.h"

namespace {

constexpr int LORA_GRAN = 16;     // rank padding: one MFMA column tile of t
constexpr int LORA_MAX_RANK = 64;
constexpr int LORA_BN = 64;       // columns per block (4 waves x 16), both kernels
constexpr int LORA_KG = 128;      // K granule of a split: 4 waves x one k-step of 32

struct LoraArgs {
  const bf16* r;         // [rows][ldr] post-add residual stream
  const bf16* A;         // [n_adapt][rcap][K]
  const bf16* Bw;        // [n_adapt][N][rb]
  const int* seg;        // [n_adapt][4] padded ranks of q, k, v (0: module absent / adapter not loaded)
  const float* scale;    // [n_adapt][4] s_q, s_k, s_v
  const int* lora_slot;  // [n_slots] adapter of a cache slot, -1: base
  const int* slot_ids;   // [B] cache slot of a sequence, or null: b itself
  float* ws;             // [nsplit][rows][rcap + 1]
  bf16* qkv;             // [rows][ldq]
  int B, S, K, ldr, ldq, rcap, rb, n_adapt, n_slots, nsplit, kchunk, tps, nq, nk, nv;
  float eps;
};

// adapter of sequence b, -1 (base) for anything out of range
MLS_DEV int lora_adapter(const LoraArgs& g, int b) {
  const int slot = g.slot_ids ? g.slot_ids[b] : b;
  MLS_CHECK(slot >= 0 && slot < g.n_slots, 501);
  if (slot < 0 || slot >= g.n_slots) return -1;
  const int a = g.lora_slot[slot];
  MLS_CHECK(a >= -1 && a < g.n_adapt, 502);
  return (a < 0 || a >= g.n_adapt) ? -1 : a;
}

// the adapter's padded ranks; false (serve the row as base) unless they fit the pack
MLS_DEV bool lora_ranks(const LoraArgs& g, int a, int (&rk)[3]) {
  bool ok = true;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    rk[p] = g.seg[a * 4 + p];
    ok = ok && rk[p] >= 0 && rk[p] <= g.rb && rk[p] % LORA_GRAN == 0;
  }
  ok = ok && rk[0] + rk[1] + rk[2] <= g.rcap;
  MLS_CHECK(ok, 503);
  return ok;
}

__global__ __launch_bounds__(256) void lora_shrink_kernel(const LoraArgs g) {
  __shared__ float red[4][16][LORA_BN + 1];
  __shared__ float ssq_red[4][16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int b = blockIdx.x / g.tps, c = blockIdx.x % g.tps;
  const int a = lora_adapter(g, b);
  if (a < 0) return;
  int rk[3];
  if (!lora_ranks(g, a, rk)) return;
  const int rtot = rk[0] + rk[1] + rk[2];
  const int c0 = blockIdx.z * LORA_BN;
  if (c0 >= rtot) return;
  const int row0 = b * g.S + c * 16, nrows = min(16, g.S - c * 16);
  const int split = blockIdx.y, kbeg = split * g.kchunk;

  const rsrc_t rr = make_rsrc(g.r + (size_t)row0 * g.ldr, (uint32_t)(((size_t)(nrows - 1) * g.ldr + g.K) * 2));
  const rsrc_t ar = make_rsrc(g.A + (size_t)a * g.rcap * g.K, (uint32_t)((size_t)rtot * g.K * 2));
  const int x_off = fr < nrows ? (fr * g.ldr + kbeg + fq * 8) * 2 : OOB;
  int w_off[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = c0 + j * 16 + fr;
    w_off[j] = col < rtot ? (col * g.K + kbeg + fq * 8) * 2 : OOB;
  }

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ssq = 0.f;
  const int nk = g.kchunk / 32;  // a multiple of 4: every wave runs nk / 4 steps
  for (int kt = wid; kt < nk; kt += 4) {
    const uint4 xv = bload16(rr, x_off == OOB ? OOB : x_off + kt * 64);
    uint4 wv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wv[j] = bload16(ar, w_off[j] == OOB ? OOB : w_off[j] + kt * 64);
    ssq += sumsq8(xv);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xv), __builtin_bit_cast(bf16x8, wv[j]),
                                                       acc[j], 0, 0, 0);
  }
  // the row's square sum over this wave's k-steps: the 4 k groups of row fr sit 16 lanes apart
  ssq += xor16_f(ssq);
  ssq += xor32_f(ssq);
  if (fq == 0) ssq_red[wid][fr] = ssq;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float e = acc[j][i];
      red[wid][fq * 4 + i][j * 16 + fr] = e;
    }
  __syncthreads();

  const size_t ldt = (size_t)g.rcap + 1;
  float* slab = g.ws + ((size_t)split * g.B * g.S + row0) * ldt;
  for (int q = tid; q < 16 * LORA_BN; q += 256) {
    const int m = q / LORA_BN, cc = q % LORA_BN;
    if (m >= nrows || c0 + cc >= rtot) continue;
    slab[m * ldt + c0 + cc] = red[0][m][cc] + red[1][m][cc] + red[2][m][cc] + red[3][m][cc];
  }
  if (blockIdx.z == 0 && tid < nrows)
    slab[tid * ldt + g.rcap] = ssq_red[0][tid] + ssq_red[1][tid] + ssq_red[2][tid] + ssq_red[3][tid];
}

__global__ __launch_bounds__(256) void lora_expand_kernel(const LoraArgs g) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int N = g.nq + g.nk + g.nv;
  const int n0 = blockIdx.y * LORA_BN + wid * 16;
  if (n0 >= N) return;
  const int b = blockIdx.x / g.tps, c = blockIdx.x % g.tps;
  const int a = lora_adapter(g, b);
  if (a < 0) return;
  int rk[3];
  if (!lora_ranks(g, a, rk)) return;
  const int p = n0 < g.nq ? 0 : n0 < g.nq + g.nk ? 1 : 2;  // segment widths are multiples of 16
  const int rp = rk[p];
  if (rp == 0) return;
  const int off = p == 0 ? 0 : p == 1 ? rk[0] : rk[0] + rk[1];
  const int row0 = b * g.S + c * 16, nrows = min(16, g.S - c * 16);
  const size_t ldt = (size_t)g.rcap + 1, rows = (size_t)g.B * g.S;
  const rsrc_t br = make_rsrc(g.Bw + (size_t)a * N * g.rb, (uint32_t)((size_t)N * g.rb * 2));

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < rp; k0 += 32) {
    const int kk = k0 + fq * 8;
    float tv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (kk < rp && fr < nrows) {
      for (int s = 0; s < g.nsplit; ++s) {  // split order: bit-identical repeats
        const float* src = g.ws + (s * rows + row0 + fr) * ldt + off + kk;
#pragma unroll
        for (int e = 0; e < 8; ++e) tv[e] += src[e];
      }
    }
    const uint4 bw = bload16(br, kk < rp ? ((n0 + fr) * g.rb + kk) * 2 : OOB);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pack8(tv)), __builtin_bit_cast(bf16x8, bw),
                                                  acc, 0, 0, 0);
  }
  const float sp = g.scale[a * 4 + p];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = fq * 4 + i;
    if (m >= nrows) continue;
    float ss = 0.f;
    for (int s = 0; s < g.nsplit; ++s) ss += g.ws[(s * rows + row0 + m) * ldt + g.rcap];
    const float rstd = rsqrtf(ss / (float)g.K + g.eps);
    const float d = acc[i];
    bf16* o = g.qkv + (size_t)(row0 + m) * g.ldq + n0 + fr;
    *o = (bf16)((float)*o + d * (sp * rstd));
  }
}

bool lora_geometry_ok(int B, int S, int K, int rcap, int nsplit) {
  return B > 0 && S > 0 && K > 0 && K % LORA_KG == 0 && K <= (1 << 20) && rcap > 0 && rcap % LORA_GRAN == 0 &&
         rcap <= 3 * LORA_MAX_RANK && nsplit >= 1 && nsplit <= 64 && K % (nsplit * LORA_KG) == 0 &&
         (long)B * S < (1l << 24);
}

}  // namespace

MLS_DEBUG_EXPORT(lora)

extern "C" {

// The K slices of a shrink launch, from host values alone: the most (a power of two dividing K / 128, at
// most 16, each slice >= 256 wide) that keep the grid within 256 blocks (one per CU).  A batch-1 decode step
// then streams a rank-16 q/k/v adapter of the 8B model (393 KB) through 16 blocks instead of one.
int mls_lora_split(int B, int S, int K, int rcap) {
  if (B <= 0 || S <= 0 || K <= 0 || K % LORA_KG || rcap <= 0) return 1;
  const long tiles = (long)B * ((S + 15) / 16) * ((rcap + LORA_BN - 1) / LORA_BN);
  int best = 1;
  for (int s = 2; s <= 16; s *= 2) {
    if ((K / LORA_KG) % s || K / s < 256) break;
    if (tiles * s <= 256) best = s;
  }
  return best;
}

// r [B*S][ldr] bf16; A [n_adapt][rcap][K] bf16; seg [n_adapt][4] int32; lora_slot [n_slots] int32; slot_ids [B]
// int32 or null; ws >= nsplit * B * S * (rcap + 1) floats.  K % (nsplit * 128) == 0.
int mls_lora_shrink(const void* r, int ldr, const void* A, const int* seg, const int* lora_slot, const int* slot_ids,
                    void* ws, size_t ws_bytes, int B, int S, int K, int rcap, int n_adapt, int n_slots, int nsplit,
                    void* stream) {
  if (!r || !A || !seg || !lora_slot || !ws || n_adapt <= 0 || n_slots <= 0 || ldr < K || ldr % 8 ||
      !lora_geometry_ok(B, S, K, rcap, nsplit))
    return MLS_BAD_ARG;
  if (!slot_ids && B > n_slots) return MLS_BAD_ARG;
  if (ws_bytes < (size_t)nsplit * B * S * (rcap + 1) * 4) return MLS_BAD_ARG;
  if ((size_t)16 * ldr * 2 >= 0x80000000ull) return MLS_UNSUPPORTED;
  LoraArgs g{};
  g.r = (const bf16*)r, g.A = (const bf16*)A, g.seg = seg, g.lora_slot = lora_slot, g.slot_ids = slot_ids;
  g.ws = (float*)ws;
  g.B = B, g.S = S, g.K = K, g.ldr = ldr, g.rcap = rcap, g.rb = LORA_MAX_RANK, g.n_adapt = n_adapt, g.n_slots = n_slots;
  g.nsplit = nsplit, g.kchunk = K / nsplit, g.tps = (S + 15) / 16;
  hipLaunchKernelGGL(lora_shrink_kernel, dim3(B * g.tps, nsplit, (rcap + LORA_BN - 1) / LORA_BN), dim3(256), 0,
                     (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

// qkv [B*S][ldq] bf16, updated in place; Bw [n_adapt][nq + nk + nv][rb] bf16 (rb 32 or 64, ranks zero-padded);
// scale [n_adapt][4] fp32; ws: what mls_lora_shrink wrote with the same B, S, K, rcap, nsplit.
int mls_lora_expand(void* qkv, int ldq, const void* Bw, const int* seg, const float* scale, const int* lora_slot,
                    const int* slot_ids, const void* ws, size_t ws_bytes, int B, int S, int K, float eps, int nq, int nk,
                    int nv, int rcap, int rb, int n_adapt, int n_slots, int nsplit, void* stream) {
  if (!qkv || !Bw || !seg || !scale || !lora_slot || !ws || n_adapt <= 0 || n_slots <= 0 ||
      !lora_geometry_ok(B, S, K, rcap, nsplit))
    return MLS_BAD_ARG;
  if (nq < 0 || nk < 0 || nv < 0 || nq % 16 || nk % 16 || nv % 16 || nq + nk + nv <= 0 || ldq < nq + nk + nv)
    return MLS_BAD_ARG;
  if ((rb != 32 && rb != 64) || rcap > 3 * rb) return MLS_BAD_ARG;
  if (!slot_ids && B > n_slots) return MLS_BAD_ARG;
  if (ws_bytes < (size_t)nsplit * B * S * (rcap + 1) * 4) return MLS_BAD_ARG;
  const int N = nq + nk + nv;
  if ((size_t)N * rb * 2 >= 0x80000000ull) return MLS_UNSUPPORTED;
  LoraArgs g{};
  g.qkv = (bf16*)qkv, g.Bw = (const bf16*)Bw, g.seg = seg, g.scale = scale, g.lora_slot = lora_slot, g.slot_ids = slot_ids;
  g.ws = (float*)const_cast<void*>(ws);
  g.B = B, g.S = S, g.K = K, g.ldq = ldq, g.rcap = rcap, g.rb = rb, g.n_adapt = n_adapt, g.n_slots = n_slots;
  g.nsplit = nsplit, g.kchunk = K / nsplit, g.tps = (S + 15) / 16, g.nq = nq, g.nk = nk, g.nv = nv, g.eps = eps;
  hipLaunchKernelGGL(lora_expand_kernel, dim3(B * g.tps, (N + LORA_BN - 1) / LORA_BN), dim3(256), 0,
                     (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

}  // extern "C"
