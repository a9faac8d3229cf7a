// K8w (speculative decoding past 3 drafts): the verify step's attention for 16 < T * G <= 64 query columns.
//
// The contract is mls_decode_attention_multi's (decode_verify.hip): query t of batch row b (t < lens[b] -
// past[b]) sits at position past[b] + t and attends cache rows 0 .. past[b] + t of slot slot_ids[b]; Q is
// read in place from the step's fused, RoPE'd qkv, K and V only from the head-major bf16 cache (per-slot
// with 64- or 128-row splits, or 64-row pages through the page table); past / lens / slot_ids / the page
// table are device arrays, the launch is capturable; partials go out per (b, t, head, split) in decode_attn's
// layout, so mls_decode_combine merges them unchanged.
//
// decode_verify_wide_kernel<G, WAVES, NC>: column c = t * G + h lies on lane column c % 16 of column tile
// c / 16, NC = 2 or 4 tiles.  Grid (Hkv, nsplit, B), a wave per 32 keys as in the narrow kernel.  Its own
// design -- not the narrow kernel run NC times:
//   * a wave loads its 32 keys' K fragments (2 x KK uint4) and V rows (8 uint4) from global memory ONCE and
//     holds the K fragments in registers across all NC tiles: the split's K / V stream is read once for up
//     to 64 columns, 8 NC + 8 NC MFMAs per 32 loaded keys against 8 + 8;
//   * the Q^T fragments of all NC tiles (KK x NC bf16x8, 64 VGPRs at NC = 4) are loaded before the K / V
//     rows and stay in registers, so the cache rows' latency covers them;
//   * the V image goes to this wave's LDS once, before the scores; mask and softmax run per column tile and
//     leave only P (one bf16x8) and (m, l) per tile live;
//   * a tile none of whose columns is a valid query of this batch row (16 nc >= n * G: ragged n, or T * G
//     short of 16 NC) runs no MFMA and leaves (-inf, 0, 0), a block-uniform branch.
// Registers and LDS -- the decision: P . V runs tile by tile and each tile's O (DT f32x4 = 32 VGPRs) is
// retired to the cross-wave merge before the next tile's P . V starts.  Keeping NC x DT accumulators live
// would hold 128 registers at NC = 4 on top of Q^T (64) and K (32) and leave one wave per SIMD; retiring them
// the compiler keeps one tile's O in 32 AGPRs and the instantiations take 148 (NC = 2) to 188 (NC = 4)
// registers in all, under the 256 at which two waves share a SIMD, with scratch 0
// (profiles/verify_wide_kernel_resources.txt).  The merge image is staged per column tile for the same
// reason: 16 columns x WAVES x D fp32 = 32 KiB at 4 waves against 128 KiB for all 64 columns, so with the V
// images (36 KiB) a block takes 68.5 KiB and two blocks share a CU -- the other block's loads hide this
// block's two barriers per tile.  DecodeMerge<G, WAVES, 16, TILED> merges columns c0 .. c0 + 15 per call.
// No RoPE / KV-append prologue and no fp8 cache, as in the narrow kernel.
#include "attn_tiles.h"

extern "C" int mls_decode_combine(void* o, float* ws, float* ws_ml, int o_stride, const int* lens, int B, int Hq,
                                  int nsplit, int chunk, void* stream);
extern "C" int mls_decode_attention_multi(const void* qkv, const void* k_cache, const void* v_cache, void* o, float* ws,
                                          float* ws_ml, int q_stride, int o_stride, const int* past, const int* lens,
                                          const int* slot_ids, const int* page_table, int pages_per_seq, int slots,
                                          int B, int T, int Hq, int Hkv, int D, long blocks, int hm_rows, int max_len,
                                          int chunk, float scale, void* stream);

namespace {

struct WideArgs {
  const bf16* q;   // head 0 of token 0 of the step's fused qkv
  const bf16* kc;  // head-major cache [blocks][Hkv][block_rows][128]
  const bf16* vc;
  bf16* o;         // [B*T][Hq*128]
  float* ws;       // [B*T][Hq][nsplit][128] partial O
  float* ws_ml;    // [B*T][Hq][nsplit][2] partial (m, l)
  int q_stride, o_stride;
  const int* past;        // [B] rows already in the cache
  const int* lens;        // [B] absolute end after this step
  const int* slot_ids;    // [B] cache slot of batch row b (nullptr: b)
  const int* page_table;  // [slots][pages_per_seq] (nullptr: per-slot cache)
  int pages_per_seq;
  int T, Hq, Hkv, nsplit;
  int blocks;      // cache blocks: slots (per-slot) or pages (paged)
  int block_rows;  // rows per block: max_seq (per-slot) or 64 (paged)
  int slots;       // rows of the page table (paged) or == blocks
  int rows_cap;    // rows one slot can hold: max_seq, or pages_per_seq * 64
  float scale_log2;
};

template <int G, int WAVES, int NC>
__global__ __launch_bounds__(WAVES * 64) void decode_verify_wide_kernel(const WideArgs a) {
  using TD = DecodeTile<G, WAVES>;
  constexpr int D = TD::D, KK = TD::KK, NT = TD::NT, CHUNK = TD::CHUNK, VST = TD::VST;
  constexpr int C = 16;  // columns of one tile: the MFMA's lane columns
  __shared__ __attribute__((aligned(16))) char vs[WAVES][32 * VST];
  __shared__ float sm_m[WAVES][C], sm_l[WAVES][C];
  __shared__ __attribute__((aligned(16))) float sm_o[WAVES][C][D];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = lane >> 4, fr = lane & 15;
  const int b = blockIdx.z, hk = blockIdx.x, sp = blockIdx.y;

  // block-uniform geometry of this batch row: decode_verify_kernel's.  In release builds the guards keep
  // every access in range (MLS_CHECK only reports): lens is clamped to what a slot and the split grid hold,
  // a slot or page id out of range reads no key and leaves (-inf, 0, 0) partials / zero rows.
  const int slot = a.slot_ids ? a.slot_ids[b] : b;
  const int L0 = a.lens[b], P0 = a.past[b];
  const bool slot_ok = slot >= 0 && slot < a.slots;
  const int cap = min(a.rows_cap, a.nsplit * CHUNK);
  MLS_CHECK(slot_ok, 328);
  MLS_CHECK(P0 >= 0 && P0 <= L0 && L0 <= cap, 327);
  const int L = min(L0, cap);        // keys of this sequence after the step
  const int P = max(0, min(P0, L));  // position of the step's first query
  const int n = min(L - P, a.T);     // valid queries of this batch row
  const int start = sp * CHUNK;
  if (start >= L) {  // a split wholly past the sequence; the first one zeroes the rows of an empty sequence
    if (L <= 0 && sp == 0)
      for (int idx = tid; idx < a.T * G * D; idx += NT)
        a.o[((long)b * a.T + idx / (G * D)) * a.o_stride + (long)hk * G * D + idx % (G * D)] = (bf16)0.f;
    return;
  }
  long cbase;  // element offset of (this split's block, head hk, key 0 of the sequence)
  bool blk_ok = slot_ok;
  if (a.page_table) {  // one page = one split; sp < ceil(L / 64) <= pages_per_seq: L <= rows_cap
    const int pg = slot_ok ? a.page_table[(long)slot * a.pages_per_seq + sp] : 0;
    blk_ok = slot_ok && pg >= 0 && pg < a.blocks;
    MLS_CHECK(!slot_ok || blk_ok, 329);
    cbase = (((long)(blk_ok ? pg : 0) * a.Hkv + hk) * CHUNK - start) * D;
  } else {
    cbase = ((long)(slot_ok ? slot : 0) * a.Hkv + hk) * a.block_rows * D;
  }
  const int end = blk_ok ? min(L, start + CHUNK) : start;  // keys [start, end) are read: end <= L <= rows_cap
  const int w0 = start + wid * 32;                         // this wave's first key
  const int ncol = n * G;                                  // valid columns: 0 .. ncol - 1 (n <= T: ncol <= 16 NC)

  // Q^T fragments of every live tile (B operand of S^T = K Q^T): tile nc, lane column fr = column 16 nc + fr
  // = query tq, head hq; zeros off the valid columns.  tq < n <= T keeps the row inside this batch row's T.
  bf16x8 qf[NC][KK];
#pragma unroll
  for (int nc = 0; nc < NC; ++nc) {
    const int c = 16 * nc + fr, tq = c / G, hq = c % G;
    const bool colv = c < ncol;
    const bf16* qp = a.q + ((long)b * a.T + (colv ? tq : 0)) * a.q_stride + (long)(hk * G + hq) * D + 8 * g;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      qf[nc][kk] = __builtin_bit_cast(bf16x8, colv ? ld16(qp + 32 * kk) : make_uint4(0, 0, 0, 0));
  }
  // the wave's 32 keys, once: K fragments stay in registers for all NC tiles, V rows go to LDS below
  uint4 kraw[2][KK], vraw[8];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    const int key = w0 + 16 * t2 + fr;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      kraw[t2][kk] = key < end ? ld16(a.kc + cbase + (long)key * D + 32 * kk + 8 * g) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int key = w0 + 4 * i + g;
    vraw[i] = key < end ? ld16(a.vc + cbase + (long)key * D + fr * 8) : make_uint4(0, 0, 0, 0);
  }
  // V rows -> this wave's LDS image (row-major, padded), once for all tiles and before the scores: their 32
  // VGPRs are free while the tiles' softmax runs
  char* V = vs[wid];
#pragma unroll
  for (int i = 0; i < 8; ++i) *reinterpret_cast<uint4*>(V + (4 * i + g) * VST + fr * 16) = vraw[i];

  // scores, mask and softmax per column tile over the wave's 32 keys (key = w0 + 16 t2 + 4g + j on the
  // accumulator row, column 16 nc + fr on the lane); only P, m and l of a tile stay live
  bf16x8 pf[NC];
  float mt[NC], ls[NC];
#pragma unroll
  for (int nc = 0; nc < NC; ++nc) {
    mt[nc] = -INFINITY;
    ls[nc] = 0.f;
    pf[nc] = __builtin_bit_cast(bf16x8, make_uint4(0, 0, 0, 0));
    if (16 * nc >= ncol) continue;  // block-uniform: no valid query on this tile
    f32x4 s[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      s[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        s[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kraw[t2][kk]), qf[nc][kk], s[t2],
                                                        0, 0, 0);
    }
    // lim = the last key column c sees in this split (below start: none)
    const int c = 16 * nc + fr;
    const int lim = c < ncol ? min(end - 1, P + c / G) : -1;
    float m = -INFINITY;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x = w0 + 16 * t2 + 4 * g + j <= lim ? s[t2][j] * a.scale_log2 : -INFINITY;
        s[t2][j] = x;
        m = fmaxf(m, x);
      }
    m = fmaxf(m, xor16_f(m));
    m = fmaxf(m, xor32_f(m));
    float l = 0.f;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(s[t2][j] - m);
        s[t2][j] = p;
        l += p;
      }
    l += xor16_f(l);
    l += xor32_f(l);
    mt[nc] = m;
    ls[nc] = l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pf[nc][j] = (bf16)s[0][j];
      pf[nc][4 + j] = (bf16)s[1][j];
    }
  }

  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's image, read back by the same wave

  // P . V tile by tile; each tile's O is retired to the merge image before the next tile's P . V.  Every
  // tile with a column of the step (16 nc < T * G) is merged -- rows t >= n get (-inf, 0, 0) / zeros, as the
  // narrow kernel leaves them -- and the trip count is block-uniform, so the barriers match.
  const DecodeMerge<G, WAVES, C, true> merge{sm_m,       sm_l, sm_o,     a.o, a.ws, a.ws_ml,
                                             a.o_stride, a.Hq, a.nsplit, b,   hk,   sp,      tid};
#pragma unroll
  for (int nc = 0; nc < NC; ++nc) {
    if (16 * nc >= a.T * G) break;
    if (nc) __syncthreads();  // the previous tile's merge has read the image
    if (g == 0) {
      sm_m[wid][fr] = mt[nc];
      sm_l[wid][fr] = ls[nc];
    }
    if (16 * nc < ncol) {  // a tile without a valid query has m = -inf: the merge never reads its O
      f32x4 o[TD::DT];
      decode_pv(o, pf[nc], V, g, fr);
      // O rows = columns 16 nc + 4g + j, O columns d = 16 dt + fr
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int dt = 0; dt < TD::DT; ++dt) sm_o[wid][4 * g + j][16 * dt + fr] = o[dt][j];
    }
    merge(L <= CHUNK, a.T, 16 * nc);
  }
}

}  // namespace

extern "C" {

// mls_decode_attention_multi's arguments and rules (decode_verify.hip) with T * Hq / Hkv <= 64 and T <= 16;
// T * Hq / Hkv <= 16 forwards to it (bit-identical there).  hm_rows = 0 (a row-major cache), D != 128,
// Hq / Hkv outside 1, 2, 4, 8, T * Hq / Hkv > 64, T > 16, pages of other than 64 rows and more than 1024
// splits are unsupported.
int mls_decode_attention_wide(const void* qkv, const void* k_cache, const void* v_cache, void* o, float* ws,
                              float* ws_ml, int q_stride, int o_stride, const int* past, const int* lens,
                              const int* slot_ids, const int* page_table, int pages_per_seq, int slots, int B, int T,
                              int Hq, int Hkv, int D, long blocks, int hm_rows, int max_len, int chunk, float scale,
                              void* stream) {
  if (B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || blocks <= 0 || slots <= 0 || max_len <= 0) return MLS_BAD_ARG;
  if (!qkv || !k_cache || !v_cache || !o || !ws || !ws_ml || !past || !lens) return MLS_BAD_ARG;
  if (D != 128) return MLS_UNSUPPORTED;
  if (hm_rows <= 0) return MLS_UNSUPPORTED;  // row-major caches: the matrix-core route reads head-major runs
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return MLS_UNSUPPORTED;
  if ((long)T * G > 64 || T > 16) return MLS_UNSUPPORTED;  // four 16-column tiles; G = 1, 2 stop at 16 queries
  if (T * G <= 16)
    return mls_decode_attention_multi(qkv, k_cache, v_cache, o, ws, ws_ml, q_stride, o_stride, past, lens, slot_ids,
                                      page_table, pages_per_seq, slots, B, T, Hq, Hkv, D, blocks, hm_rows, max_len,
                                      chunk, scale, stream);
  if (page_table && (hm_rows != 64 || pages_per_seq <= 0)) return MLS_UNSUPPORTED;  // a split = one page
  if (chunk != 64 && chunk != 128) return MLS_BAD_ARG;
  if (page_table && chunk != 64) return MLS_BAD_ARG;
  if (!page_table && slots != blocks) return MLS_BAD_ARG;
  if (q_stride % 8 || q_stride < Hq * D || o_stride != Hq * D) return MLS_BAD_ARG;  // the combine's row indexing
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) & 15)
    return MLS_BAD_ARG;  // 16-B loads
  if (blocks > 0x7FFFFFFFl || B > 65535 || (long)B * T * Hq > 0x7FFFFFFFl) return MLS_BAD_ARG;
  const long cap = page_table ? (long)pages_per_seq * 64 : (long)hm_rows;
  const int rows_cap = (int)(cap > 0x7FFFFFC0l ? 0x7FFFFFC0l : cap);
  if (max_len > rows_cap) max_len = rows_cap;
  const int nsplit = (max_len + chunk - 1) / chunk;
  if (nsplit > 1024) return MLS_UNSUPPORTED;  // combine keeps one weight per split in LDS
  WideArgs a{};
  a.q = (const bf16*)qkv;
  a.kc = (const bf16*)k_cache;
  a.vc = (const bf16*)v_cache;
  a.o = (bf16*)o;
  a.ws = ws;
  a.ws_ml = ws_ml;
  a.q_stride = q_stride;
  a.o_stride = o_stride;
  a.past = past;
  a.lens = lens;
  a.slot_ids = slot_ids;
  a.page_table = page_table;
  a.pages_per_seq = pages_per_seq;
  a.T = T; a.Hq = Hq; a.Hkv = Hkv; a.nsplit = nsplit;
  a.blocks = (int)blocks;
  a.block_rows = hm_rows;
  a.slots = slots;
  a.rows_cap = rows_cap;
  a.scale_log2 = scale * 1.4426950408889634f;
  dim3 grid(Hkv, nsplit, B);
  hipStream_t st = (hipStream_t)stream;
#define WIDE_W(GG, NCC)                                                                                     \
  if (chunk == 64) hipLaunchKernelGGL((decode_verify_wide_kernel<GG, 2, NCC>), grid, dim3(128), 0, st, a);  \
  else hipLaunchKernelGGL((decode_verify_wide_kernel<GG, 4, NCC>), grid, dim3(256), 0, st, a);
#define WIDE(GG)                        \
  if (T * GG <= 32) { WIDE_W(GG, 2) }   \
  else { WIDE_W(GG, 4) }
  // G = 1: T <= 16 columns always forward; G = 2: T <= 16 gives at most 32 columns
  if (G == 2) { WIDE_W(2, 2) }
  else if (G == 4) { WIDE(4) }
  else { WIDE(8) }
#undef WIDE
#undef WIDE_W
  const int rc = (int)hipGetLastError();
  if (rc != 0 || nsplit <= 1) return rc;
  // the partials of row b are those of T * Hq heads: [b][t][h] = [b][t * Hq + h], output row stride T * Hq * D
  return mls_decode_combine(o, ws, ws_ml, T * o_stride, lens, B, T * Hq, nsplit, chunk, stream);
}

}  // extern "C"

MLS_DEBUG_EXPORT(decode_verify_wide)
