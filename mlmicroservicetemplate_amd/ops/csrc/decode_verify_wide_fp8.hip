// K8w on K13's cache (speculative decoding past 3 drafts with the FP8 KV cache): the verify step's attention
// for 16 < T * G <= 64 query columns against the e4m3 cache.
//
// The contract is mls_decode_attention_multi's (decode_verify.hip): query t of batch row b (t < lens[b] -
// past[b]) sits at position past[b] + t and attends cache rows 0 .. past[b] + t of slot slot_ids[b]; Q is
// read in place from the step's fused, RoPE'd qkv, K and V only from the head-major e4m3 cache with the fp32
// (row, KV head) scales of kv_fp8.hip (per-slot with 64- or 128-row splits, or 64-row pages through the page
// table); past / lens / slot_ids / the page table are device arrays, the launch is capturable; partials go
// out per (b, t, head, split) in decode_attn's layout, so mls_decode_combine merges them unchanged.
//
// decode_verify_wide_fp8_kernel<G, WAVES, NC>: decode_verify_wide_kernel's block (grid (Hkv, nsplit, B), a
// wave per 32 keys, column c = t * G + h on lane column c % 16 of column tile c / 16, NC = 2 or 4 tiles)
// reading the cache as decode_verify_fp8_kernel does.  Per wave:
//   * Q^T: the fragments of all NC tiles (KK x NC bf16x8) are loaded first, from global memory at K's
//     permuted columns 64 (kk >> 1) + 16 g + 8 (kk & 1) + 0..7, and stay in registers: no LDS image of Q;
//   * K: lane (fr, g) of key tile t2 loads bytes [64 jj + 16 g, +16) of key w0 + 16 t2 + fr (jj = 0, 1): a
//     128-B row by 16-B loads, 4 uint4 per lane for the wave's 32 keys, ONCE for all tiles;
//   * scales: the four K and four V scales of the lane's accumulator rows (keys w0 + 16 t2 + 4 g + 0..3) by
//     scales4's rule, once per key tile, reused by every column tile.  The K scale multiplies the fp32 S^T
//     row, the V scale is folded into P before P is rounded to bf16; a masked key's scales are never used
//     (its S is replaced by -inf and its P by 0 through selects);
//   * V: 16 B (16 dims) of key w0 + 8 i + lane / 8, converted into the per-wave padded bf16 image that
//     ds_read_b64_tr_b16 reads (decode_v_fill_fp8), once and before the scores;
//   * mask, softmax and P . V tile by tile; each tile's O is retired to DecodeMerge<.., TILED>, staged per
//     16-column tile, before the next tile starts; a tile none of whose columns is a valid query of this
//     batch row runs no MFMA and leaves (-inf, 0, 0), a block-uniform branch.
// Registers and LDS -- the decision: the K bytes are converted e4m3 -> bf16 (exact) once, right after the
// loads, and the 2 x KK bf16x8 fragments (32 VGPRs) are held across the NC tiles.  The alternative keeps the
// 16 VGPRs of raw bytes and converts inside each tile: 16 fewer registers, but 64 v_cvt_pk_f32_fp8 + 64
// packs per wave and tile, 4 x that at NC = 4, on the VALU that the softmax of the same tile is waiting for --
// against 8 MFMAs.  16 registers do not change the occupancy here: with Q^T (64 at NC = 4), K (32), the
// scales (16), one tile's O (32 AGPRs) and the softmax temporaries every instantiation stays under the 256
// registers at which two waves share a SIMD, with no scratch (profiles/verify_wide_fp8_kernel_resources.txt),
// so the conversion is paid once.  The raw K / V bytes (16 + 16 VGPRs) die before the first tile.  As in the
// bf16 kernel each tile's O is retired before the next P . V, and the merge image is staged per tile: 34.25 /
// 68.5 KiB of LDS (2 / 4 waves), two blocks per CU at least.
#include "attn_tiles.h"

extern "C" int mls_decode_combine(void* o, float* ws, float* ws_ml, int o_stride, const int* lens, int B, int Hq,
                                  int nsplit, int chunk, void* stream);
extern "C" int mls_decode_attention_multi_fp8(const void* qkv, const void* k_cache, const void* v_cache,
                                              const float* k_scale, const float* v_scale, void* o, float* ws,
                                              float* ws_ml, int q_stride, int o_stride, const int* past,
                                              const int* lens, const int* slot_ids, const int* page_table,
                                              int pages_per_seq, int slots, int B, int T, int Hq, int Hkv, int D,
                                              long blocks, int hm_rows, int max_len, int chunk, float scale,
                                              void* stream);

namespace {

struct WideFp8Args {
  const bf16* q;       // head 0 of token 0 of the step's fused qkv
  const uint8_t* kc;   // head-major e4m3 cache [blocks][Hkv][block_rows][128]
  const uint8_t* vc;
  const float* ksc;    // [blocks][Hkv][block_rows]
  const float* vsc;
  bf16* o;             // [B*T][Hq*128]
  float* ws;           // [B*T][Hq][nsplit][128] partial O
  float* ws_ml;        // [B*T][Hq][nsplit][2] partial (m, l)
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
__global__ __launch_bounds__(WAVES * 64) void decode_verify_wide_fp8_kernel(const WideFp8Args a) {
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
  // a slot or page id out of range reads no key and no scale and leaves (-inf, 0, 0) partials / zero rows.
  const int slot = a.slot_ids ? a.slot_ids[b] : b;
  const int L0 = a.lens[b], P0 = a.past[b];
  const bool slot_ok = slot >= 0 && slot < a.slots;
  const int cap = min(a.rows_cap, a.nsplit * CHUNK);
  MLS_CHECK(slot_ok, 331);
  MLS_CHECK(P0 >= 0 && P0 <= L0 && L0 <= cap, 330);
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
  long rowbase;  // cache row of (this split's block, head hk, key 0 of the sequence): bytes * D, scales as is
  bool blk_ok = slot_ok;
  if (a.page_table) {  // one page = one split; sp < ceil(L / 64) <= pages_per_seq: L <= rows_cap
    const int pg = slot_ok ? a.page_table[(long)slot * a.pages_per_seq + sp] : 0;
    blk_ok = slot_ok && pg >= 0 && pg < a.blocks;
    MLS_CHECK(!slot_ok || blk_ok, 332);
    rowbase = ((long)(blk_ok ? pg : 0) * a.Hkv + hk) * CHUNK - start;
  } else {
    rowbase = ((long)(slot_ok ? slot : 0) * a.Hkv + hk) * a.block_rows;
  }
  const int end = blk_ok ? min(L, start + CHUNK) : start;  // keys [start, end) are read: end <= L <= rows_cap
  const int w0 = start + wid * 32;                         // this wave's first key
  const int ncol = n * G;                                  // valid columns: 0 .. ncol - 1 (n <= T: ncol <= 16 NC)

  // Q^T fragments of every tile (B operand of S^T = K Q^T) at K's permuted dims: tile nc, lane column fr =
  // column 16 nc + fr = query tq, head hq; zeros off the valid columns.  tq < n <= T keeps the row inside
  // this batch row's T.
  bf16x8 qf[NC][KK];
#pragma unroll
  for (int nc = 0; nc < NC; ++nc) {
    const int c = 16 * nc + fr, tq = c / G, hq = c % G;
    const bool colv = c < ncol;
    const bf16* qp = a.q + ((long)b * a.T + (colv ? tq : 0)) * a.q_stride + (long)(hk * G + hq) * D + 16 * g;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      qf[nc][kk] =
          __builtin_bit_cast(bf16x8, colv ? ld16(qp + 64 * (kk >> 1) + 8 * (kk & 1)) : make_uint4(0, 0, 0, 0));
  }
  // the wave's 32 keys, once: K bytes, the scales of the lane's accumulator rows, V bytes
  uint4 kraw[2][2], vraw[4];
  float4 ksv[2], vsv[2];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    const int key = w0 + 16 * t2 + fr;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
      kraw[t2][jj] = key < end ? ld16(a.kc + (rowbase + key) * D + 64 * jj + 16 * g) : make_uint4(0, 0, 0, 0);
    const int kf = w0 + 16 * t2 + 4 * g;
    ksv[t2] = scales4(a.ksc, rowbase, kf, end);
    vsv[t2] = scales4(a.vsc, rowbase, kf, end);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = w0 + 8 * i + (lane >> 3);
    vraw[i] = key < end ? ld16(a.vc + (rowbase + key) * D + (lane & 7) * 16) : make_uint4(0, 0, 0, 0);
  }
  // K bytes -> bf16 fragments (exact), once for all NC tiles: k-slice kk = 2 jj + h is the load's h-th 8 bytes
  bf16x8 kb[2][KK];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      kb[t2][2 * jj] = fp8x8_to_bf16(kraw[t2][jj].x, kraw[t2][jj].y);
      kb[t2][2 * jj + 1] = fp8x8_to_bf16(kraw[t2][jj].z, kraw[t2][jj].w);
    }
  // V rows -> this wave's LDS image (row-major bf16, padded), once for all tiles and before the scores
  char* V = vs[wid];
#pragma unroll
  for (int i = 0; i < 4; ++i) decode_v_fill_fp8(V, 8 * i + (lane >> 3), lane & 7, vraw[i]);

  // scores, mask and softmax per column tile over the wave's 32 keys (key = w0 + 16 t2 + 4g + j on the
  // accumulator row, column 16 nc + fr on the lane): the key's K scale, then the softmax scale; only P (with
  // the key's V scale folded in), m and l of a tile stay live
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
        s[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kb[t2][kk], qf[nc][kk], s[t2], 0, 0, 0);
    }
    // lim = the last key column c sees in this split (below start: none).  A key past lim keeps neither its
    // score nor its V scale.
    const int c = 16 * nc + fr;
    const int lim = c < ncol ? min(end - 1, P + c / G) : -1;
    float m = -INFINITY;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const float kq[4] = {ksv[t2].x, ksv[t2].y, ksv[t2].z, ksv[t2].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x = w0 + 16 * t2 + 4 * g + j <= lim ? s[t2][j] * kq[j] * a.scale_log2 : -INFINITY;
        s[t2][j] = x;
        m = fmaxf(m, x);
      }
    }
    m = fmaxf(m, xor16_f(m));
    m = fmaxf(m, xor32_f(m));
    float l = 0.f;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const float vq[4] = {vsv[t2].x, vsv[t2].y, vsv[t2].z, vsv[t2].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool vis = w0 + 16 * t2 + 4 * g + j <= lim;
        const float p = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(s[t2][j] - m);
        l += p;  // the denominator takes the unscaled P
        pf[nc][4 * t2 + j] = (bf16)(p * (vis ? vq[j] : 0.f));
      }
    }
    l += xor16_f(l);
    l += xor32_f(l);
    mt[nc] = m;
    ls[nc] = l;
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

// mls_decode_attention_multi_fp8's arguments and rules (decode_verify_fp8.hip) with T * Hq / Hkv <= 64 and
// T <= 16; T * Hq / Hkv <= 16 forwards to it (bit-identical there).  hm_rows = 0 (a row-major cache), D != 128,
// Hq / Hkv outside 1, 2, 4, 8, T * Hq / Hkv > 64, T > 16, pages of other than 64 rows and more than 1024
// splits are unsupported.
int mls_decode_attention_wide_fp8(const void* qkv, const void* k_cache, const void* v_cache, const float* k_scale,
                                  const float* v_scale, void* o, float* ws, float* ws_ml, int q_stride, int o_stride,
                                  const int* past, const int* lens, const int* slot_ids, const int* page_table,
                                  int pages_per_seq, int slots, int B, int T, int Hq, int Hkv, int D, long blocks,
                                  int hm_rows, int max_len, int chunk, float scale, void* stream) {
  if (B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || blocks <= 0 || slots <= 0 || max_len <= 0) return MLS_BAD_ARG;
  if (!qkv || !k_cache || !v_cache || !k_scale || !v_scale || !o || !ws || !ws_ml || !past || !lens) return MLS_BAD_ARG;
  if (D != 128) return MLS_UNSUPPORTED;
  if (hm_rows <= 0) return MLS_UNSUPPORTED;  // the e4m3 cache is head-major only
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return MLS_UNSUPPORTED;
  if ((long)T * G > 64 || T > 16) return MLS_UNSUPPORTED;  // four 16-column tiles; G = 1, 2 stop at 16 queries
  if (T * G <= 16)
    return mls_decode_attention_multi_fp8(qkv, k_cache, v_cache, k_scale, v_scale, o, ws, ws_ml, q_stride, o_stride,
                                          past, lens, slot_ids, page_table, pages_per_seq, slots, B, T, Hq, Hkv, D,
                                          blocks, hm_rows, max_len, chunk, scale, stream);
  if (page_table && (hm_rows != 64 || pages_per_seq <= 0)) return MLS_UNSUPPORTED;  // a split = one page
  if (chunk != 64 && chunk != 128) return MLS_BAD_ARG;
  if (page_table && chunk != 64) return MLS_BAD_ARG;
  if (!page_table && slots != blocks) return MLS_BAD_ARG;
  if (q_stride % 8 || q_stride < Hq * D || o_stride != Hq * D) return MLS_BAD_ARG;  // the combine's row indexing
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache) |
       reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 15)
    return MLS_BAD_ARG;  // 16-B loads
  if (blocks > 0x7FFFFFFFl || B > 65535 || (long)B * T * Hq > 0x7FFFFFFFl) return MLS_BAD_ARG;
  const long cap = page_table ? (long)pages_per_seq * 64 : (long)hm_rows;
  const int rows_cap = (int)(cap > 0x7FFFFFC0l ? 0x7FFFFFC0l : cap);
  if (max_len > rows_cap) max_len = rows_cap;
  const int nsplit = (max_len + chunk - 1) / chunk;
  if (nsplit > 1024) return MLS_UNSUPPORTED;  // combine keeps one weight per split in LDS
  WideFp8Args a{};
  a.q = (const bf16*)qkv;
  a.kc = (const uint8_t*)k_cache;
  a.vc = (const uint8_t*)v_cache;
  a.ksc = k_scale;
  a.vsc = v_scale;
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
#define WIDE8_W(GG, NCC)                                                                                        \
  if (chunk == 64) hipLaunchKernelGGL((decode_verify_wide_fp8_kernel<GG, 2, NCC>), grid, dim3(128), 0, st, a);  \
  else hipLaunchKernelGGL((decode_verify_wide_fp8_kernel<GG, 4, NCC>), grid, dim3(256), 0, st, a);
#define WIDE8(GG)                        \
  if (T * GG <= 32) { WIDE8_W(GG, 2) }   \
  else { WIDE8_W(GG, 4) }
  // G = 1: T <= 16 columns always forward; G = 2: T <= 16 gives at most 32 columns
  if (G == 2) { WIDE8_W(2, 2) }
  else if (G == 4) { WIDE8(4) }
  else { WIDE8(8) }
#undef WIDE8
#undef WIDE8_W
  const int rc = (int)hipGetLastError();
  if (rc != 0 || nsplit <= 1) return rc;
  // the partials of row b are those of T * Hq heads: [b][t][h] = [b][t * Hq + h], output row stride T * Hq * D
  return mls_decode_combine(o, ws, ws_ml, T * o_stride, lens, B, T * Hq, nsplit, chunk, stream);
}

}  // extern "C"

MLS_DEBUG_EXPORT(decode_verify_wide_fp8)
