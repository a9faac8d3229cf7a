// K13: FP8 (OCP e4m3) KV cache for Llama decode on gfx950 -- half the cache bytes, half the bytes
// the decode-attention kernel streams.
//
// Layout (head-major only, D = 128): caches uint8 [blocks][Hkv][R][D], one fp32 scale per
// (cache row, KV head) in [blocks][Hkv][R]; blocks = sequences (R = max_seq) or 64-row pages.
// The rule (ops/reference.py kv_quant_fp8): scale = max(max|x|, 2^-40) / 448, q = e4m3(x * (1 / scale)).
//
// (1) rope_kv_fp8_kernel: the prefill writer.  RoPE on Q and K in place in the bf16 QKV rows exactly
//     as rope_kv_kernel (norm_ops.hip) -- prefill attention keeps reading unquantised bf16 -- then
//     the quantised K / V rows and their scales go to the cache slot.
// (2) decode_attn_fp8_kernel: matrix-core decode attention on the fp8 cache, the structure of
//     decode_attn_mfma_kernel (attention.hip).  e4m3 converts to bf16 exactly, so K bytes go through
//     v_cvt_pk_f32_fp8 into the same v_mfma_f32_16x16x32_bf16; the per-key K scale multiplies the
//     fp32 S^T row, the per-key V scale is folded into P.  The kernel's own: the cache addressing and
//     its bounds, RoPE in the prefill writer's rounding, the K loads and their dimension
//     permutation, the scaled softmax and the V image fill.  Shared with the bf16 kernel through
//     attn_tiles.h: the prologue's operand loads, O = P . V, the cross-wave merge with the direct /
//     partial write, and the empty-split exit.  Partials (m, l, O) therefore have one format: the
//     combine kernel here and the fused combine of mls_skinny_packed_combine[_ar] consume them.
// Both writers (prefill, and the rope-mode prologue of decode) quantise through kv_fp8_quant_store:
// identical bytes for identical input, so a token's logits do not depend on who wrote its row.
#include "attn_tiles.h"

namespace {

constexpr int D = 128;
constexpr float KV_FP8_MAX = 448.f;
constexpr float KV_FP8_AMAX_FLOOR = 0x1p-40f;

// rotate-half RoPE of one pair (the expressions of rope_kv_kernel; shared so both writers round alike)
MLS_DEV float rope_lo(float x0, float x1, float c, float s) { return x0 * c - x1 * s; }
MLS_DEV float rope_hi(float x0, float x1, float c, float s) { return x1 * c + x0 * s; }

// max over an aligned group of 16 lanes (one DPP row), every lane gets it
MLS_DEV float group_max16(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));   // lane ^ 1
  v = fmaxf(v, dpp_f<0x4E>(v));   // lane ^ 2
  v = fmaxf(v, dpp_f<0x141>(v));  // row_half_mirror
  v = fmaxf(v, dpp_f<0x140>(v));  // row_mirror
  return v;
}

// The one quantiser.  A head row is held by 16 aligned lanes, lane c the (bf16-valued) dims
// 8c .. 8c + 7.  Returns the row's scale and this lane's 8 bytes; with `store` the bytes go to
// row + 8c and lane 0 writes the scale.
MLS_DEV float kv_fp8_quant_store(const float (&x)[8], int c, uint8_t* row, float* scale_p, bool store, uint2& q) {
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(x[e]));
  amax = group_max16(amax);
  const float scale = fmaxf(amax, KV_FP8_AMAX_FLOOR) / KV_FP8_MAX;
  const float inv = 1.f / scale;
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] * inv, x[5] * inv, 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] * inv, x[7] * inv, hi, true);
  q = make_uint2((uint32_t)lo, (uint32_t)hi);
  if (store) {
    *reinterpret_cast<uint2*>(row + c * 8) = q;
    if (c == 0) *scale_p = scale;
  }
  return scale;
}

// 8 e4m3 bytes -> 8 bf16 (exact)
MLS_DEV bf16x8 fp8x8_to_bf16(uint32_t d0, uint32_t d1) {
  const f32x2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)d0, false);
  const f32x2 f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)d0, true);
  const f32x2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)d1, false);
  const f32x2 f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)d1, true);
  bf16x8 r;
  r[0] = (bf16)f0[0]; r[1] = (bf16)f0[1]; r[2] = (bf16)f1[0]; r[3] = (bf16)f1[1];
  r[4] = (bf16)f2[0]; r[5] = (bf16)f2[1]; r[6] = (bf16)f3[0]; r[7] = (bf16)f3[1];
  return r;
}

// ------------------------------------------------------------------------------- prefill writer
// Block = one token.  Phase 1 is rope_kv_kernel's rotation; phase 2 gives each of the token's
// 2 Hkv head rows to 16 lanes (8 dims each): |max| by DPP, convert, 8-B stores.
__global__ __launch_bounds__(256) void rope_kv_fp8_kernel(bf16* __restrict__ qkv, const int* __restrict__ positions,
                                                          const float* __restrict__ cos_t,
                                                          const float* __restrict__ sin_t, int row_stride, int Hq,
                                                          int Hkv, const int* __restrict__ slots,
                                                          uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                          float* __restrict__ ksc, float* __restrict__ vsc,
                                                          const int* __restrict__ lens, int S, int max_seq,
                                                          long cache_rows, int max_pos, int hm_rows) {
  const long t = blockIdx.x;
  constexpr int half = D >> 1, quads = half >> 2;
  const int p = positions[t];
  const bool p_ok = p >= 0 && p < max_pos;
  MLS_CHECK(p_ok, 102);
  if (!p_ok) return;  // no RoPE row for this position: leave the token untouched
  bf16* row = qkv + t * row_stride;
  const int nrot = Hq + Hkv;
  for (int q = threadIdx.x; q < nrot * quads; q += blockDim.x) {
    const int h = q / quads, i = (q % quads) * 4;
    bf16* base = row + (long)h * D;
    const bf16x4 a = __builtin_bit_cast(bf16x4, *reinterpret_cast<const uint2*>(base + i));
    const bf16x4 b = __builtin_bit_cast(bf16x4, *reinterpret_cast<const uint2*>(base + half + i));
    const float4 c = *reinterpret_cast<const float4*>(cos_t + (long)p * half + i);
    const float4 sn = *reinterpret_cast<const float4*>(sin_t + (long)p * half + i);
    const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {sn.x, sn.y, sn.z, sn.w};
    bf16x4 oa, ob;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x0 = (float)a[e], x1 = (float)b[e];
      oa[e] = (bf16)rope_lo(x0, x1, cc[e], ss[e]);
      ob[e] = (bf16)rope_hi(x0, x1, cc[e], ss[e]);
    }
    *reinterpret_cast<uint2*>(base + i) = __builtin_bit_cast(uint2, oa);
    *reinterpret_cast<uint2*>(base + half + i) = __builtin_bit_cast(uint2, ob);
  }
  // cache slot: explicit, or derived (token t = batch t / S, position p; written while p < lens[b])
  int slot = -1;
  if (slots) {
    slot = slots[t];
  } else if (max_seq > 0) {
    const int b = (int)(t / S);
    if (p < max_seq && (!lens || p < lens[b])) slot = b * max_seq + p;
  }
  if (slot < 0 || !kc) return;
  MLS_CHECK(slot < cache_rows, 101);
  if (slot >= cache_rows) return;
  __syncthreads();  // rotated K visible to the reads below (same block, global memory)
  __threadfence_block();
  const int ntask = 2 * Hkv * 16;  // a multiple of 16: the 16 lanes of a row stay together
  for (int q = threadIdx.x; q < ntask; q += blockDim.x) {
    const int task = q >> 4, c = q & 15;
    const int which = task / Hkv, h = task % Hkv;
    float x[8];
    unpack8(ld16(row + (long)(Hq + which * Hkv + h) * D + c * 8), x);
    const long srow = ((long)(slot / hm_rows) * Hkv + h) * hm_rows + slot % hm_rows;
    uint2 qb;
    kv_fp8_quant_store(x, c, (which ? vc : kc) + srow * D, (which ? vsc : ksc) + srow, true, qb);
  }
}

// ------------------------------------------------------------------------------- decode
struct DecodeFp8Args {
  const bf16* q;   // [B][q_stride], head h at h*D (rope mode: the fused QKV row, K at Hq*D, V at (Hq+Hkv)*D)
  uint8_t* kc;     // [blocks][Hkv][R][D] e4m3
  uint8_t* vc;
  float* ksc;      // [blocks][Hkv][R]
  float* vsc;
  bf16* o;         // [B][o_stride]
  float* ws;       // [B][Hq][nsplit][D]
  float* ws_ml;    // [B][Hq][nsplit][2]
  int q_stride, o_stride;
  const int* lens;
  const int* page_table;  // paged: [B][pages_per_seq] page ids, a page = one split's CHUNK rows
  int pages_per_seq;
  int blocks;             // cache blocks (sequences, or pages): the bound on b / page ids
  int hm_rows;            // R
  const int* positions;   // rope mode: query position per sequence (== lens[b] - 1)
  const float* cos_t;     // [max_pos][D/2]
  const float* sin_t;
  int Hq, Hkv, nsplit, max_pos;
  float scale_log2;
};

// grid (Hkv, splits, B), WAVES waves of 32 keys: see decode_attn_mfma_kernel.  What differs:
//   K: a key row is 128 B; lane (fr, g) of key tile t2 loads bytes [64 jj + 16 g, +16) of key
//      w0 + 16 t2 + fr (jj = 0, 1): 16-B loads, and k-slice kk = 2 jj + h takes the load's h-th 8
//      bytes -- a permutation of D over the MFMA k index that Q's fragment reads back identically
//      (columns 64 (kk >> 1) + 16 g + 8 (kk & 1) + 0..7 of the roped head in LDS).
//   scales: keys w0 + 16 t2 + 4 g + 0..3 sit on the lane's four accumulator rows and their scales
//      are contiguous: one 16-B load each for K and V.
//   V: lane loads 16 B (16 dims) of key w0 + 8 i + lane / 8, converts to bf16 and writes 32 B of
//      the same padded row-major image that ds_read_b64_tr_b16 reads.
template <int G, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void decode_attn_fp8_kernel(const DecodeFp8Args a) {
  using T = DecodeTile<G, WAVES>;
  static_assert(T::D == D, "the shared decode pieces are D = 128");
  constexpr int KK = T::KK, NT = T::NT, CHUNK = T::CHUNK, VST = T::VST, NPRO = T::NPRO, PIT = T::PIT;
  __shared__ __attribute__((aligned(16))) char vs[WAVES][32 * VST];
  __shared__ __attribute__((aligned(16))) bf16 qimg[G][D];      // roped q heads
  __shared__ __attribute__((aligned(16))) uint8_t newq[2][D];   // the new token's quantised K, V rows
  __shared__ float newsc[2];                                    // ... and their scales
  __shared__ float sm_m[WAVES][G], sm_l[WAVES][G];
  __shared__ __attribute__((aligned(16))) float sm_o[WAVES][G][D];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = lane >> 4, fr = lane & 15;
  const int b = blockIdx.z, hk = blockIdx.x, sp = blockIdx.y;
  const int L0 = a.lens[b];
  // rows a sequence can hold: its page-table entries, or its block of the cache
  const int cap = a.page_table ? a.nsplit * CHUNK : min(a.nsplit * CHUNK, a.hm_rows);
  MLS_CHECK(sp != 0 || L0 <= cap, 201);
  const int L = min(L0, cap);
  const int start = sp * CHUNK;
  if (decode_split_empty<G, NT>(start, L, sp, a.o, a.o_stride, b, hk, tid)) return;
  const int end = min(L, start + CHUNK);
  const bool rope = a.positions != nullptr;
  const int pos = rope ? a.positions[b] : 0;
  const bool pos_ok = !rope || (pos >= 0 && pos < a.max_pos && pos == L0 - 1);
  MLS_CHECK(pos_ok, 202);
  const int blk = a.page_table ? a.page_table[b * a.pages_per_seq + sp] : b;
  const bool blk_ok = blk >= 0 && blk < a.blocks;
  MLS_CHECK(blk_ok, 203);
  if (!blk_ok || (rope && (pos < 0 || pos >= a.max_pos))) return;  // block-uniform, before any barrier
  const bf16* qrow = a.q + (long)b * a.q_stride;
  // cache row of key r: rowbase + r (bytes: * D; scale index: as is)
  const long rowbase = ((long)blk * a.Hkv + hk) * a.hm_rows - (a.page_table ? start : 0);
  const bool has_new = rope && L - 1 >= start && L - 1 < end;
  const int w0 = start + wid * 32;  // this wave's first key

  // small operands first (so their vmcnt waits leave the cache rows in flight), then the rows
  uint4 px[PIT], pxp[PIT], pv[PIT];
  float4 pcs[PIT][4];
  decode_pro_load<G, WAVES>(px, pxp, pv, pcs, qrow, rope, a.cos_t, a.sin_t, pos, hk, a.Hq, a.Hkv, tid);
  uint4 kraw[2][2], vraw[4];
  float4 ksv[2], vsv[2];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    const int key = w0 + 16 * t2 + fr;
    const bool ok = key < end && !(rope && key == L - 1);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
      kraw[t2][jj] = ok ? ld16(a.kc + (rowbase + key) * D + 64 * jj + 16 * g) : make_uint4(0, 0, 0, 0);
    // keys kf .. kf + 3: kf % 4 == 0 and kf < end <= cap with cap % 4 == 0, so all four are in the block
    const int kf = w0 + 16 * t2 + 4 * g;
    ksv[t2] = kf < end ? *reinterpret_cast<const float4*>(a.ksc + rowbase + kf) : make_float4(0.f, 0.f, 0.f, 0.f);
    vsv[t2] = kf < end ? *reinterpret_cast<const float4*>(a.vsc + rowbase + kf) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = w0 + 8 * i + (lane >> 3);
    const bool ok = key < end && !(rope && key == L - 1);
    vraw[i] = ok ? ld16(a.vc + (rowbase + key) * D + (lane & 7) * 16) : make_uint4(0, 0, 0, 0);
  }

  // prologue: RoPE'd q heads (bf16, as the cache path rounds them) -> LDS; the new token's roped K
  // and its V are quantised by the shared writer (bytes + scales -> LDS), and the block holding
  // row L-1 stores them: the attention below sees the row exactly as the cache now holds it
#pragma unroll
  for (int it = 0; it < PIT; ++it) {
    const int t = tid + it * NT, r = t >> 4, c = t & 15;
    if (t < NPRO && (r < G || rope)) {
      float x[8];
      unpack8(px[it], x);
      if (rope) {
        float xp[8];
        unpack8(pxp[it], xp);
        const float cc[8] = {pcs[it][0].x, pcs[it][0].y, pcs[it][0].z, pcs[it][0].w,
                             pcs[it][1].x, pcs[it][1].y, pcs[it][1].z, pcs[it][1].w};
        const float sn[8] = {pcs[it][2].x, pcs[it][2].y, pcs[it][2].z, pcs[it][2].w,
                             pcs[it][3].x, pcs[it][3].y, pcs[it][3].z, pcs[it][3].w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          x[e] = c < 8 ? rope_lo(x[e], xp[e], cc[e], sn[e]) : rope_hi(xp[e], x[e], cc[e], sn[e]);
      }
      const uint4 xb = pack8(x);
      if (r < G) {
        *reinterpret_cast<uint4*>(&qimg[r < G ? r : 0][c * 8]) = xb;
      } else {  // r == G (rope mode): 16 aligned lanes
        float kx[8], vx[8];
        unpack8(xb, kx);
        unpack8(pv[it], vx);
        const long nrow = rowbase + (L - 1);
        uint2 kq, vq;
        const float ksn = kv_fp8_quant_store(kx, c, a.kc + nrow * D, a.ksc + nrow, has_new, kq);
        const float vsn = kv_fp8_quant_store(vx, c, a.vc + nrow * D, a.vsc + nrow, has_new, vq);
        *reinterpret_cast<uint2*>(&newq[0][c * 8]) = kq;
        *reinterpret_cast<uint2*>(&newq[1][c * 8]) = vq;
        if (c == 0) {
          newsc[0] = ksn;
          newsc[1] = vsn;
        }
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  bf16x8 qf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk)
    qf[kk] = fr < G ? __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(
                          &qimg[fr < G ? fr : 0][64 * (kk >> 1) + 16 * g + 8 * (kk & 1)]))
                    : __builtin_bit_cast(bf16x8, make_uint4(0, 0, 0, 0));
  const float ks_new = rope ? newsc[0] : 0.f, vs_new = rope ? newsc[1] : 0.f;
  f32x4 s[2];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    if (rope && w0 + 16 * t2 + fr == L - 1) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) kraw[t2][jj] = *reinterpret_cast<const uint4*>(&newq[0][64 * jj + 16 * g]);
    }
    s[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      s[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16(kraw[t2][jj].x, kraw[t2][jj].y), qf[2 * jj],
                                                      s[t2], 0, 0, 0);
      s[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16(kraw[t2][jj].z, kraw[t2][jj].w), qf[2 * jj + 1],
                                                      s[t2], 0, 0, 0);
    }
  }
  // softmax over the wave's 32 keys (key = w0 + 16 t2 + 4g + j on accumulator row, head fr on the
  // lane); the key's K scale first, then the softmax scale
  float vscale[2][4];
  float mt = -INFINITY;
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    const float kq[4] = {ksv[t2].x, ksv[t2].y, ksv[t2].z, ksv[t2].w};
    const float vq[4] = {vsv[t2].x, vsv[t2].y, vsv[t2].z, vsv[t2].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = w0 + 16 * t2 + 4 * g + j;
      const bool isnew = rope && key == L - 1;
      const float x = key < end ? s[t2][j] * (isnew ? ks_new : kq[j]) * a.scale_log2 : -INFINITY;
      vscale[t2][j] = key < end ? (isnew ? vs_new : vq[j]) : 0.f;
      s[t2][j] = x;
      mt = fmaxf(mt, x);
    }
  }
  mt = fmaxf(mt, xor16_f(mt));
  mt = fmaxf(mt, xor32_f(mt));
  float ls = 0.f;
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = mt == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(s[t2][j] - mt);
      s[t2][j] = p;
      ls += p;  // the denominator takes the unscaled P
    }
  ls += xor16_f(ls);
  ls += xor32_f(ls);

  // V rows -> this wave's LDS image (row-major bf16, padded); the new row from the prologue image
  char* V = vs[wid];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int krow = 8 * i + (lane >> 3), cch = lane & 7;
    uint4 v = vraw[i];
    if (rope && w0 + krow == L - 1) v = *reinterpret_cast<const uint4*>(&newq[1][cch * 16]);
    *reinterpret_cast<uint4*>(V + krow * VST + cch * 32) = __builtin_bit_cast(uint4, fp8x8_to_bf16(v.x, v.y));
    *reinterpret_cast<uint4*>(V + krow * VST + cch * 32 + 16) = __builtin_bit_cast(uint4, fp8x8_to_bf16(v.z, v.w));
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's image, read back by the same wave
  bf16x8 pf;  // P with the key's V scale folded in (a masked key: p = 0 and scale 0)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    pf[j] = (bf16)(s[0][j] * vscale[0][j]);
    pf[4 + j] = (bf16)(s[1][j] * vscale[1][j]);
  }
  f32x4 o[T::DT];
  decode_pv(o, pf, V, g, fr);
  // O rows = heads 4g + j, columns d = 16 dt + fr
  if (g == 0 && fr < G) {
    sm_m[wid][fr] = mt;
    sm_l[wid][fr] = ls;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int h = 4 * g + j;
    if (h < G) {
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt) sm_o[wid][h < G ? h : 0][16 * dt + fr] = o[dt][j];
    }
  }
  const DecodeMerge<G, WAVES> merge{sm_m,       sm_l, sm_o,     a.o, a.ws, a.ws_ml,
                                    a.o_stride, a.Hq, a.nsplit, b,   hk,   sp,      tid};
  merge(L <= CHUNK);
}

// merge the splits of one (b, q-head): block of D threads; every split's (m, l) once into LDS.  The
// arithmetic of decode_combine_kernel (attention.hip) in its plain-loop form, kept on purpose: on this
// path the one-round-trip form measured 2.8 % slower at batch 8 x 8192 (128 splits of 64) and its
// differently contracted sums moved output bits (docs/PERF_NOTES.md).
__global__ __launch_bounds__(D) void decode_combine_fp8_kernel(const DecodeFp8Args a, int chunk) {
  __shared__ float sw[1024];
  __shared__ float s_inv;
  __shared__ float red[D / 64];
  const int bh = blockIdx.x;  // b * Hq + h
  const int b = bh / a.Hq, h = bh % a.Hq;
  const int d = threadIdx.x;
  const int cap = a.page_table ? a.nsplit * chunk : min(a.nsplit * chunk, a.hm_rows);
  const int L = min(a.lens[b], cap);
  const int ns = min(a.nsplit, (L + chunk - 1) / chunk);
  if (ns <= 1) return;  // the split kernel wrote this row directly
  const long rec = (long)bh * a.nsplit;
  float mloc = -INFINITY;
  for (int s = d; s < ns; s += D) mloc = fmaxf(mloc, a.ws_ml[(rec + s) * 2]);
  mloc = wave_max(mloc);
  if ((d & 63) == 0) red[d >> 6] = mloc;
  __syncthreads();
  float M = red[0];
#pragma unroll
  for (int w = 1; w < D / 64; ++w) M = fmaxf(M, red[w]);
  float lloc = 0.f;
  for (int s = d; s < ns; s += D) {
    const float w = M == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(a.ws_ml[(rec + s) * 2] - M);
    sw[s] = w;
    lloc += a.ws_ml[(rec + s) * 2 + 1] * w;
  }
  lloc = wave_sum(lloc);
  __syncthreads();
  if ((d & 63) == 0) red[d >> 6] = lloc;
  __syncthreads();
  if (d == 0) {
    float Ls = 0.f;
#pragma unroll
    for (int w = 0; w < D / 64; ++w) Ls += red[w];
    s_inv = Ls > 0.f ? 1.f / Ls : 0.f;
  }
  __syncthreads();
  float O = 0.f;
  int s = 0;
  for (; s + 8 <= ns; s += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = a.ws[(rec + s + j) * D + d];
#pragma unroll
    for (int j = 0; j < 8; ++j) O += v[j] * sw[s + j];
  }
  for (; s < ns; ++s) O += a.ws[(rec + s) * D + d] * sw[s];
  a.o[(long)b * a.o_stride + (long)h * D + d] = (bf16)(O * s_inv);
}

}  // namespace

extern "C" {

// mls_rope_kv's arguments plus the two scale tensors.  The FP8 cache is head-major, D = 128:
// k_cache / v_cache uint8 [cache_rows / hm_rows][Hkv][hm_rows][128], scales fp32 without the last dim.
int mls_rope_kv_fp8(void* qkv, const int* positions, const float* cos_t, const float* sin_t, long tokens,
                    int row_stride, int Hq, int Hkv, int Dh, const int* slots, void* k_cache, void* v_cache,
                    float* k_scale, float* v_scale, const int* lens, int S, int max_seq, long cache_rows, int max_pos,
                    int hm_rows, void* stream) {
  if (Dh != D || hm_rows <= 0) return MLS_UNSUPPORTED;
  if (tokens <= 0 || row_stride % 8 || Hq <= 0 || Hkv <= 0 || (!slots && max_seq > 0 && S <= 0)) return MLS_BAD_ARG;
  if (cache_rows % hm_rows || !k_cache || !v_cache || !k_scale || !v_scale) return MLS_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) & 7) return MLS_BAD_ARG;
  hipLaunchKernelGGL(rope_kv_fp8_kernel, dim3((unsigned)tokens), dim3(256), 0, (hipStream_t)stream, (bf16*)qkv,
                     positions, cos_t, sin_t, row_stride, Hq, Hkv, slots, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale,
                     v_scale, lens, S, max_seq, cache_rows, max_pos, hm_rows);
  return (int)hipGetLastError();
}

// mls_decode_attention on the FP8 cache (head-major only).  blocks: sequences in the cache (>= B), or
// pages in the pool when page_table is given; hm_rows: rows per block (paged: == chunk).  Workspace,
// counters, skip_combine and rope mode as mls_decode_attention.
int mls_decode_attention_fp8(const void* q, void* k_cache, void* v_cache, float* k_scale, float* v_scale, void* o,
                             float* ws, float* ws_ml, int* counters, int q_stride, int o_stride, int blocks,
                             const int* lens, const int* positions, const float* cos_t, const float* sin_t,
                             int max_pos, int B, int Hq, int Hkv, int Dh, int max_len, int chunk, float scale,
                             const int* page_table, int pages_per_seq, int skip_combine, int hm_rows, void* stream) {
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || max_len <= 0 || blocks <= 0) return MLS_BAD_ARG;
  const int G = Hq / Hkv;
  if (Dh != D || hm_rows <= 0 || (chunk != 64 && chunk != 128) || (G != 1 && G != 2 && G != 4 && G != 8))
    return MLS_UNSUPPORTED;
  if (hm_rows % 4) return MLS_BAD_ARG;  // 16-B scale loads
  if (page_table ? (hm_rows != chunk || (long)pages_per_seq * chunk < max_len) : (max_len > hm_rows || blocks < B))
    return MLS_BAD_ARG;
  if (!k_cache || !v_cache || !k_scale || !v_scale || !lens) return MLS_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache) |
       reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale) | reinterpret_cast<uintptr_t>(q)) & 15)
    return MLS_BAD_ARG;
  if (q_stride % 8) return MLS_BAD_ARG;
  if (positions && (!cos_t || !sin_t)) return MLS_BAD_ARG;
  (void)counters;  // reserved, as in mls_decode_attention: the combine runs as its own launch
  DecodeFp8Args a{};
  a.q = (const bf16*)q;
  a.kc = (uint8_t*)k_cache;
  a.vc = (uint8_t*)v_cache;
  a.ksc = k_scale;
  a.vsc = v_scale;
  a.o = (bf16*)o;
  a.ws = ws;
  a.ws_ml = ws_ml;
  a.q_stride = q_stride;
  a.o_stride = o_stride;
  a.lens = lens;
  a.page_table = page_table;
  a.pages_per_seq = pages_per_seq;
  a.blocks = blocks;
  a.hm_rows = hm_rows;
  a.positions = positions;
  a.cos_t = cos_t;
  a.sin_t = sin_t;
  a.max_pos = max_pos;
  a.Hq = Hq;
  a.Hkv = Hkv;
  a.nsplit = (max_len + chunk - 1) / chunk;
  a.scale_log2 = scale * 1.4426950408889634f;
  if (a.nsplit > 1024) return MLS_UNSUPPORTED;  // combine keeps one weight per split in LDS
  dim3 grid(Hkv, a.nsplit, B);
  hipStream_t st = (hipStream_t)stream;
#define DEC8(GG)                                                                                       \
  if (chunk == 64) hipLaunchKernelGGL((decode_attn_fp8_kernel<GG, 2>), grid, dim3(128), 0, st, a);    \
  else hipLaunchKernelGGL((decode_attn_fp8_kernel<GG, 4>), grid, dim3(256), 0, st, a);
  if (G == 1) { DEC8(1) }
  else if (G == 2) { DEC8(2) }
  else if (G == 4) { DEC8(4) }
  else { DEC8(8) }
#undef DEC8
  if (a.nsplit > 1 && !skip_combine)
    hipLaunchKernelGGL(decode_combine_fp8_kernel, dim3(B * Hq), dim3(D), 0, st, a, chunk);
  return (int)hipGetLastError();
}

}  // extern "C"

MLS_DEBUG_EXPORT(kv_fp8)
