// K8 (chunked prefill): causal attention of a chunk of new queries against the KV cache.
//
// Query i of batch row b (i < lens[b] - past[b]) sits at position past[b] + i and attends to cache
// rows 0 .. past[b] + i of slot slot_ids[b] (b when null).  Q is read in place from the fused,
// already-RoPE'd qkv [B*S, (Hq+2Hkv)*D] of the chunk; K and V come ONLY from the cache -- the chunk's
// own rows are appended first (mls_rope_kv) and read back like any other context row.  past / lens /
// slot_ids / the page table are device arrays, nothing is read on the host: the launch is capturable.
//
// flash_ctx_kernel runs the v2 flash tile of attn_tiles.h -- the 64-key LDS tile layout (FlashTile) and
// the tile body (Flash2Tile: S^T = K . Q^T with the key on the accumulator row, O^T += V^T . P^T,
// masks on edge tiles only) -- which it shares with flash_fwd2_kernel<128> of attention.hip; the
// staging loop and the epilogue are that kernel's text (attn_tiles.h says why they are not shared).
// What is this kernel's own:
//   * the causal diagonal is offset by past[b] (the tile body gets the position past[b] + qw of the
//     wave's first query): a block's 64 queries span up to two key tiles, so the last tile can be
//     wholly above an early wave's diagonal (all of its MFMAs are skipped);
//   * a K / V tile is one contiguous 64 x 256 B run of a head-major cache: rows kt*64 .. of
//     [slot][Hkv][max_seq][D], or (paged) the whole block [page][Hkv][64][D] the table maps tile kt
//     to.  Each run gets its own buffer descriptor -- a 64-bit base and the run's valid bytes -- so
//     caches beyond 4 GiB are addressed exactly, rows >= lens[b] (and anything past the slot's rows)
//     read as zero through the hardware range check, and lane offsets stay 16-bit constants.
#include "attn_tiles.h"

namespace {

struct CtxArgs {
  const bf16* q;   // head 0 of token 0 of the chunk's fused qkv
  const bf16* kc;  // head-major cache [blocks][Hkv][block_rows][128]
  const bf16* vc;
  bf16* o;         // [B*S][o_stride]
  int q_stride, o_stride;
  uint32_t q_bytes;
  const int* past;        // [B] rows already in the cache
  const int* lens;        // [B] absolute end after this chunk
  const int* slot_ids;    // [B] cache slot of batch row b (nullptr: b)
  const int* page_table;  // [slots][pages_per_seq] (nullptr: per-slot cache)
  int pages_per_seq;
  int B, S, Hq, Hkv;
  int blocks;      // cache blocks: slots (per-slot) or pages (paged)
  int block_rows;  // rows per block: max_seq (per-slot) or 64 (paged)
  int slots;       // rows of the page table (paged) or == blocks
  int rows_cap;    // rows one slot can hold: max_seq, or pages_per_seq * 64
  float scale_log2;
};

__global__ __launch_bounds__(256, 3) void flash_ctx_kernel(const CtxArgs a) {
  constexpr int D = 128, NW = 4;
  using T = FlashTile<D>;
  constexpr int NT = 64 * NW;
  constexpr int BQ = 16 * NW, BKV = T::BKV, CPR = T::CPR;
  __shared__ __attribute__((aligned(16))) char smem[T::K_BYTES + T::V_BYTES];
  char* Ks = smem;
  char* Vs = smem + T::K_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, fr = lane & 15;
  const int b = blockIdx.z, h = blockIdx.y;
  const int hk = h / (a.Hq / a.Hkv);
  const int q0 = blockIdx.x * BQ;
  const int qw = q0 + wid * 16;
  const bool paged = a.page_table != nullptr;

  // block-uniform geometry of this batch row (guards hold in release builds, MLS_CHECK reports)
  const int slot = __builtin_amdgcn_readfirstlane(a.slot_ids ? a.slot_ids[b] : b);
  const int L0 = __builtin_amdgcn_readfirstlane(a.lens[b]);
  const int P0 = __builtin_amdgcn_readfirstlane(a.past[b]);
  const bool slot_ok = slot >= 0 && slot < a.slots;
  MLS_CHECK(slot_ok, 312);
  MLS_CHECK(P0 >= 0 && P0 <= L0 && L0 <= a.rows_cap, 311);
  const int L = slot_ok ? min(L0, a.rows_cap) : 0;  // keys of this sequence after the chunk
  const int P = max(0, min(P0, L));                 // position of the chunk's first query
  const int n = min(L - P, a.S);                    // valid queries of this batch row
  const long tokq = (long)b * a.S;

  if (q0 >= n) {  // no valid query in this tile: zero rows (finite padding for the GEMMs that follow)
    for (int c = tid; c < BQ * CPR; c += NT) {
      const int q = q0 + c / CPR;
      if (q < a.S) st16(a.o + (tokq + q) * a.o_stride + (long)h * D + (c % CPR) * 8, make_uint4(0, 0, 0, 0));
    }
    return;
  }

  const rsrc_t qr = make_rsrc(a.q, a.q_bytes);
  bf16x8 qf[T::KK];  // Q^T fragments (B operand of S^T = K Q^T): Q[q = qw + fr][d = 32kk + 8g .. +7]
  {
    const int q = qw + fr;
#pragma unroll
    for (int kk = 0; kk < T::KK; ++kk) {
      const int off = q < a.S ? (int)(((tokq + q) * a.q_stride + (long)h * D + 32 * kk + 8 * g) * 2) : OOB;
      qf[kk] = __builtin_bit_cast(bf16x8, bload16(qr, off));
    }
  }

  f32x4 acc_o[T::DT];
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt) acc_o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;

  const int kv_end = min(L, P + q0 + BQ);  // one past the last key any query of the block sees
  const int ntiles = (kv_end + BKV - 1) / BKV;
  const int pw = P + qw;  // position of the wave's first query

  constexpr int NI = T::ni(NT);
  const int* tab = paged ? a.page_table + (long)slot * a.pages_per_seq : nullptr;
  // ntiles <= ceil(L / 64) <= pages_per_seq: L <= rows_cap = pages_per_seq * 64
  auto page_of = [&](int kt) { return paged && kt < ntiles ? __builtin_amdgcn_readfirstlane(tab[kt]) : 0; };
  uint4 kreg[NI], vreg[NI];
  // tile kt's run: 64-bit base of its first row, valid bytes = its rows below L (the rest reads 0)
  auto load_tile = [&](int kt, int pg) {
    const bool blk_ok = !paged || (pg >= 0 && pg < a.blocks);
    MLS_CHECK(blk_ok, 313);
    const long row0 = paged ? ((long)(blk_ok ? pg : 0) * a.Hkv + hk) * BKV
                            : ((long)slot * a.Hkv + hk) * a.block_rows + (long)kt * BKV;
    const uint32_t bytes = blk_ok ? (uint32_t)(min(BKV, L - kt * BKV) * D * 2) : 0u;
    const rsrc_t kr = make_rsrc(a.kc + row0 * D, bytes);
    const rsrc_t vr = make_rsrc(a.vc + row0 * D, bytes);
#pragma unroll
    for (int i = 0; i < NI; ++i) {  // chunk idx = tid + NT i of the run, 16 B each
      kreg[i] = bload16(kr, (tid + NT * i) * 16);
      vreg[i] = bload16(vr, (tid + NT * i) * 16);
    }
  };
  const float c = a.scale_log2;
  const int causal = 1;  // (unused: the rule is the template argument)
  const Flash2Tile<D, true> tile_body{acc_o, m_run, l_run, qf, Ks, Vs, causal, pw, L, c, g, fr};
  // the page id of tile kt + 1 is read one tile early, so its K / V loads do not wait on the table
  int pg_next = page_of(1);
  load_tile(0, page_of(0));
  for (int kt = 0; kt < ntiles; ++kt) {
    const int kv0 = kt * BKV;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int idx = tid + NT * i;
      const int row = idx / CPR, ch = idx % CPR;
      *reinterpret_cast<uint4*>(Ks + row * (D * 2) + ((ch ^ (row & (CPR - 1))) * 16)) = kreg[i];
      *reinterpret_cast<uint4*>(Vs + row * T::VST + ch * 16) = vreg[i];
    }
    __syncthreads();
    if (kt + 1 < ntiles) {
      load_tile(kt + 1, pg_next);
      pg_next = page_of(kt + 2);
    }
    // keys kv0 + 16t + 4g + j against the query at position pw + fr; the mask (and the sub-tile
    // skip) only where the tile crosses the key range end or the wave's diagonal
    tile_body(kv0, kv0 + BKV > L || kv0 + BKV - 1 > pw);
    __syncthreads();
  }

  // ---- normalise (lane-local 1 / l of query fr) and store through LDS as 16-B row stores
  float l = l_run + xor16_f(l_run);
  l += xor32_f(l);
  const float inv_l = l > 0.f ? 1.f / l : 0.f;
  constexpr int OST = T::OST;
  bf16* Os = reinterpret_cast<bf16*>(smem) + wid * 16 * OST;  // K / V tile space: past the last barrier
  static_assert(NW * 16 * OST * 2 <= T::K_BYTES + T::V_BYTES, "output tiles fit the K / V tiles");
#pragma unroll
  for (int dt = 0; dt < T::DT; ++dt) {
    bf16x4 o4;
#pragma unroll
    for (int j = 0; j < 4; ++j) o4[j] = (bf16)(acc_o[dt][j] * inv_l);
    *reinterpret_cast<bf16x4*>(Os + fr * OST + 16 * dt + 4 * g) = o4;
  }
  __syncthreads();
#pragma unroll
  for (int cc = lane; cc < 16 * CPR; cc += 64) {
    const int r = cc / CPR, ch = cc % CPR;
    const int q = qw + r;
    if (q < a.S) st16(a.o + (tokq + q) * a.o_stride + (long)h * D + ch * 8, ld16(Os + r * OST + ch * 8));
  }
}

}  // namespace

extern "C" {

// qkv: the chunk's fused projection [B*S][q_stride] (Q heads first, already RoPE'd); caches head-major
// [blocks][Hkv][hm_rows][D] (hm_rows = max_seq per slot, or 64 when paged through page_table
// [slots][pages_per_seq]); past / lens / slot_ids int32 [B] on the device.  hm_rows = 0 (a row-major
// cache), D != 128 and pages of other than 64 rows are unsupported.
int mls_flash_attention_ctx(const void* qkv, const void* k_cache, const void* v_cache, void* o, int q_stride,
                            int o_stride, const int* past, const int* lens, const int* slot_ids,
                            const int* page_table, int pages_per_seq, int slots, int B, int S, int Hq, int Hkv, int D,
                            long blocks, int hm_rows, float scale, void* stream) {
  if (B <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || blocks <= 0 || slots <= 0) return MLS_BAD_ARG;
  if (!qkv || !k_cache || !v_cache || !o || !past || !lens) return MLS_BAD_ARG;
  if (D != 128) return MLS_UNSUPPORTED;
  if (hm_rows <= 0) return MLS_UNSUPPORTED;  // row-major caches: a tile would be 64 slices, not one run
  if (page_table && (hm_rows != 64 || pages_per_seq <= 0)) return MLS_UNSUPPORTED;  // a tile = one page
  if (!page_table && slots != blocks) return MLS_BAD_ARG;
  if (q_stride % 8 || o_stride % 8 || q_stride < Hq * D || o_stride < Hq * D) return MLS_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(o) | reinterpret_cast<uintptr_t>(k_cache) |
       reinterpret_cast<uintptr_t>(v_cache)) & 15)
    return MLS_BAD_ARG;  // 16-B loads / row stores
  if (blocks > 0x7FFFFFFFl || (long)B * S > 0x7FFFFFFFl) return MLS_BAD_ARG;
  const size_t qb = ((size_t)((long)B * S - 1) * q_stride + (size_t)Hq * D) * 2;
  if (qb >= 0x7FFFFFFFull) return MLS_UNSUPPORTED;
  CtxArgs a{};
  a.q = (const bf16*)qkv;
  a.kc = (const bf16*)k_cache;
  a.vc = (const bf16*)v_cache;
  a.o = (bf16*)o;
  a.q_stride = q_stride;
  a.o_stride = o_stride;
  a.q_bytes = (uint32_t)qb;
  a.past = past;
  a.lens = lens;
  a.slot_ids = slot_ids;
  a.page_table = page_table;
  a.pages_per_seq = pages_per_seq;
  a.B = B; a.S = S; a.Hq = Hq; a.Hkv = Hkv;
  a.blocks = (int)blocks;
  a.block_rows = hm_rows;
  a.slots = slots;
  const long cap = page_table ? (long)pages_per_seq * 64 : (long)hm_rows;
  a.rows_cap = (int)(cap > 0x7FFFFFC0l ? 0x7FFFFFC0l : cap);
  a.scale_log2 = scale * 1.4426950408889634f;
  dim3 grid((S + 63) / 64, Hq, B);
  hipLaunchKernelGGL(flash_ctx_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"

MLS_DEBUG_EXPORT(flash_ctx)
