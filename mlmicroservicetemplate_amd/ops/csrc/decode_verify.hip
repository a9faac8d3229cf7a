// K8 (speculative decoding): a few queries per sequence against the KV cache, split-KV, on the matrix
// cores -- the verify step's attention.
//
// The contract is mls_flash_attention_ctx's: query t of batch row b (t < lens[b] - past[b]) sits at
// position past[b] + t and attends cache rows 0 .. past[b] + t of slot slot_ids[b] (b when null).  Q is
// read in place from the step's fused, already-RoPE'd qkv [B*T, (Hq+2Hkv)*D]; K and V come ONLY from
// the cache -- the step's own rows are appended first (mls_rope_kv).  past / lens / slot_ids / the page
// table are device arrays, nothing is read on the host: the launch is capturable.
//
// decode_verify_kernel<G, WAVES> is decode_attn_mfma_kernel (attention.hip) with the lane columns that
// kernel pads with zeros put to work: column c = t * G + h holds query t of head h of the KV head, T * G
// <= 16, so one block streams a split's K / V rows once for all T positions and all G heads.  Grid
// (Hkv, nsplit, B), a wave per 32 keys, 8 + 8 MFMAs per wave as there; DecodeDims, decode_pv and the
// merge (DecodeMerge with C = 16 columns) are that kernel's, from attn_tiles.h.  What is this kernel's
// own:
//   * the mask: key j is visible to column c iff j <= past[b] + c / G and c / G < lens[b] - past[b]; a
//     column with no visible key in a split leaves (m, l, O) = (-inf, 0, 0), which the merges weigh 0;
//   * no RoPE / KV-append prologue and no fp8 cache (docs/PERF_NOTES.md, "Speculative decoding");
//   * partials are written per (b, t, head, split) -- to the combine they are the partials of T * Hq heads
//     of row b, so decode_combine_kernel merges them unchanged (mls_decode_combine).
#include "attn_tiles.h"

// attention.hip: decode_combine_kernel<128> over partials in decode_attn's layout
extern "C" int mls_decode_combine(void* o, float* ws, float* ws_ml, int o_stride, const int* lens, int B, int Hq,
                                  int nsplit, int chunk, void* stream);

namespace {

struct VerifyArgs {
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

template <int G, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void decode_verify_kernel(const VerifyArgs a) {
  using TD = DecodeTile<G, WAVES>;
  constexpr int D = TD::D, KK = TD::KK, NT = TD::NT, CHUNK = TD::CHUNK, VST = TD::VST;
  constexpr int C = 16;  // lane columns: T * G of them in use
  __shared__ __attribute__((aligned(16))) char vs[WAVES][32 * VST];
  __shared__ float sm_m[WAVES][C], sm_l[WAVES][C];
  __shared__ __attribute__((aligned(16))) float sm_o[WAVES][C][D];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = lane >> 4, fr = lane & 15;
  const int b = blockIdx.z, hk = blockIdx.x, sp = blockIdx.y;

  // block-uniform geometry of this batch row.  In release builds the guards keep every access in range
  // (MLS_CHECK only reports): lens is clamped to what a slot and the split grid hold -- the combine, which
  // sees the raw lens[b], then counts exactly the splits that ran -- and a slot or page id out of range
  // reads no key, so its splits leave (-inf, 0, 0) partials / zero rows like any split without a visible key.
  const int slot = a.slot_ids ? a.slot_ids[b] : b;
  const int L0 = a.lens[b], P0 = a.past[b];
  const bool slot_ok = slot >= 0 && slot < a.slots;
  const int cap = min(a.rows_cap, a.nsplit * CHUNK);
  MLS_CHECK(slot_ok, 322);
  MLS_CHECK(P0 >= 0 && P0 <= L0 && L0 <= cap, 321);
  const int L = min(L0, cap);                // keys of this sequence after the step
  const int P = max(0, min(P0, L));          // position of the step's first query
  const int n = min(L - P, a.T);             // valid queries of this batch row
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
    MLS_CHECK(!slot_ok || blk_ok, 323);
    cbase = (((long)(blk_ok ? pg : 0) * a.Hkv + hk) * CHUNK - start) * D;
  } else {
    cbase = ((long)(slot_ok ? slot : 0) * a.Hkv + hk) * a.block_rows * D;
  }
  const int end = blk_ok ? min(L, start + CHUNK) : start;  // keys [start, end) are read: end <= L <= rows_cap
  const int w0 = start + wid * 32;                         // this wave's first key

  // Q^T fragments (B operand of S^T = K Q^T): column fr = query tq, head hq; zeros off the valid columns
  const int tq = fr / G, hq = fr % G;
  const bool colv = fr < a.T * G && tq < n;
  bf16x8 qf[KK];
  {
    const bf16* qp = a.q + ((long)b * a.T + tq) * a.q_stride + (long)(hk * G + hq) * D + 8 * g;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      qf[kk] = __builtin_bit_cast(bf16x8, colv ? ld16(qp + 32 * kk) : make_uint4(0, 0, 0, 0));
  }
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

  f32x4 s[2];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    s[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      s[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kraw[t2][kk]), qf[kk], s[t2], 0, 0, 0);
  }
  // softmax over the wave's 32 keys (key = w0 + 16 t2 + 4g + j on the accumulator row, column fr on the
  // lane); lim = the last key column fr sees in this split (below start: none)
  const int lim = colv ? min(end - 1, P + tq) : -1;
  float mt = -INFINITY;
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x = w0 + 16 * t2 + 4 * g + j <= lim ? s[t2][j] * a.scale_log2 : -INFINITY;
      s[t2][j] = x;
      mt = fmaxf(mt, x);
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
      ls += p;
    }
  ls += xor16_f(ls);
  ls += xor32_f(ls);

  // V rows -> this wave's LDS image (row-major, padded)
  char* V = vs[wid];
#pragma unroll
  for (int i = 0; i < 8; ++i) *reinterpret_cast<uint4*>(V + (4 * i + g) * VST + fr * 16) = vraw[i];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's image, read back by the same wave
  bf16x8 pf;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    pf[j] = (bf16)s[0][j];
    pf[4 + j] = (bf16)s[1][j];
  }
  f32x4 o[TD::DT];
  decode_pv(o, pf, V, g, fr);
  // O rows = columns 4g + j, O columns d = 16 dt + fr
  if (g == 0) {
    sm_m[wid][fr] = mt;
    sm_l[wid][fr] = ls;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int dt = 0; dt < TD::DT; ++dt) sm_o[wid][4 * g + j][16 * dt + fr] = o[dt][j];
  const DecodeMerge<G, WAVES, C> merge{sm_m,       sm_l, sm_o,     a.o, a.ws, a.ws_ml,
                                       a.o_stride, a.Hq, a.nsplit, b,   hk,   sp,      tid};
  merge(L <= CHUNK, a.T);
}

}  // namespace

extern "C" {

// qkv: the step's fused projection [B*T][q_stride] (Q heads first, already RoPE'd); o [B*T][Hq*D],
// contiguous; caches head-major [blocks][Hkv][hm_rows][D] (hm_rows = max_seq per slot, or 64 when paged
// through page_table [slots][pages_per_seq]); past / lens / slot_ids int32 [B] on the device.
// max_len: a host bound on lens (sizes the split grid), chunk: rows per split, 64 or 128 (paged: 64).
// ws >= B*T*Hq*nsplit*D floats, ws_ml >= B*T*Hq*nsplit*2 floats, nsplit = ceil(max_len / chunk).
// hm_rows = 0 (a row-major cache), D != 128, Hq / Hkv outside 1, 2, 4, 8, T * Hq / Hkv > 16, pages of
// other than 64 rows and more than 1024 splits are unsupported.
int mls_decode_attention_multi(const void* qkv, const void* k_cache, const void* v_cache, void* o, float* ws,
                               float* ws_ml, int q_stride, int o_stride, const int* past, const int* lens,
                               const int* slot_ids, const int* page_table, int pages_per_seq, int slots, int B, int T,
                               int Hq, int Hkv, int D, long blocks, int hm_rows, int max_len, int chunk, float scale,
                               void* stream) {
  if (B <= 0 || T <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || blocks <= 0 || slots <= 0 || max_len <= 0) return MLS_BAD_ARG;
  if (!qkv || !k_cache || !v_cache || !o || !ws || !ws_ml || !past || !lens) return MLS_BAD_ARG;
  if (D != 128) return MLS_UNSUPPORTED;
  if (hm_rows <= 0) return MLS_UNSUPPORTED;  // row-major caches: the fp8-free matrix-core route reads head-major runs
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return MLS_UNSUPPORTED;
  if ((long)T * G > 16) return MLS_UNSUPPORTED;  // the MFMA's 16 lane columns
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
  VerifyArgs a{};
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
#define VER(GG)                                                                                      \
  if (chunk == 64) hipLaunchKernelGGL((decode_verify_kernel<GG, 2>), grid, dim3(128), 0, st, a);     \
  else hipLaunchKernelGGL((decode_verify_kernel<GG, 4>), grid, dim3(256), 0, st, a);
  if (G == 1) { VER(1) }
  else if (G == 2) { VER(2) }
  else if (G == 4) { VER(4) }
  else { VER(8) }
#undef VER
  const int rc = (int)hipGetLastError();
  if (rc != 0 || nsplit <= 1) return rc;
  // the partials of row b are those of T * Hq heads: [b][t][h] = [b][t * Hq + h], output row stride T * Hq * D
  return mls_decode_combine(o, ws, ws_ml, T * o_stride, lens, B, T * Hq, nsplit, chunk, stream);
}

}  // extern "C"

MLS_DEBUG_EXPORT(decode_verify)
