// K8 (chunked prefill): causal attention of a chunk of new queries against the KV cache.
//
// Query i of batch row b (i < lens[b] - past[b]) sits at position past[b] + i and attends to cache
// rows 0 .. past[b] + i of slot slot_ids[b] (b when null).  Q is read in place from the fused,
// already-RoPE'd qkv [B*S, (Hq+2Hkv)*D] of the chunk; K and V come ONLY from the cache -- the chunk's
// own rows are appended first (mls_rope_kv) and read back like any other context row.  past / lens /
// slot_ids / the page table are device arrays, nothing is read on the host: the launch is capturable.
// Rows at or past a batch row's valid length (padding rows) are written as zeros: the GEMMs that
// follow read them.
//
// One kernel text, flash_ctx_kernel<FP8, SPLIT>, for the two cache types and the two launches.  It runs
// the v2 flash tile of attn_tiles.h -- the 64-key LDS tile layout (FlashTile) and the tile body
// (Flash2Tile: S^T = K . Q^T with the key on the accumulator row, O^T += V^T . P^T, masks on edge tiles
// only) -- which it shares with flash_fwd2_kernel<128> of attention.hip; the staging loop and the
// epilogue are that kernel's text (attn_tiles.h says why they are not shared), and for the same reason
// the parts that differ between the instantiations stand in place as `if constexpr`, not in helpers.
// What is this kernel's own:
//   * the causal diagonal is offset by past[b] (the tile body gets the position past[b] + qw of the
//     wave's first query): a block's 64 queries span up to two key tiles, so the last tile can be
//     wholly above an early wave's diagonal (all of its MFMAs are skipped);
//   * a K / V tile is one contiguous run of a head-major cache: rows kt*64 .. of
//     [slot][Hkv][max_seq][D], or (paged) the whole block [page][Hkv][64][D] the table maps tile kt
//     to.  Each run gets its own buffer descriptor -- a 64-bit base and the run's valid bytes -- so
//     caches beyond 4 GiB are addressed exactly, rows >= lens[b] (and anything past the slot's rows)
//     read as zero through the hardware range check, and lane offsets stay 16-bit constants.
//
// FP8: e4m3 caches (kv_fp8.hip's layout), the chunk path of kv_prefill="cache" -- uint8
// [blocks][Hkv][R][128] with one fp32 scale per (row, KV head) in [blocks][Hkv][R].  A 64-key tile of a
// head is one 8 KiB run of bytes and one 256-B run of scales; each of the four runs (K, V, their scales)
// gets its own descriptor.  Dequantisation is in the staging step: a 16-B load is 16 dims of one row,
// converted exactly (e4m3 -> fp32), the fp32 product with the row's scale is rounded to bf16 (RNE) into
// the same LDS images -- so the MFMAs see bf16(e4m3 * scale), one rounding of relative 2^-9 per element
// on top of what the cache holds (the reference attends the unrounded fp32 product).  The alternative of
// decode_attn_fp8_kernel (K scale on the S^T row, V scale folded into P) would need the scales inside
// Flash2Tile, which the bf16 instantiations share: not taken.  A row past lens[b] reads zero bytes and a
// zero scale: a zero row, as on the bf16 cache.
//
// SPLIT: a few queries against a long cached context (a prefix-cache hit, a verify step).  The unsplit
// grid is (q tiles, Hq, B): 32 new tokens against 4064 cached rows is Hq blocks that each walk 64 key
// tiles.  The split launch cuts every (b, q tile)'s key tiles into nsplit runs of tiles_per_split tiles
// -- both from the HOST bound on past + n, so every block of a launch cuts at the same tile boundaries
// whatever lens[] holds, per-slot and paged alike -- and stores the unnormalised partial (O, m, l) of its
// run to an fp32 workspace; flash_ctx_combine_kernel merges the partials of a (token, q head) in split
// order and writes the bf16 row.
#include "attn_tiles.h"

namespace {

struct CtxArgs {
  const bf16* q;   // head 0 of token 0 of the chunk's fused qkv
  const bf16* kc;  // head-major cache [blocks][Hkv][block_rows][128] (null when FP8)
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
  // SPLIT (and the combine)
  float* ws_o;   // [nsplit][B*S][Hq][128] unnormalised O
  float* ws_ml;  // [nsplit][B*S][Hq][2]   m (log2 domain, as m_run) and l
  int nsplit, tiles_per_split;
  // FP8: the caches as e4m3 bytes, same shape, and the rows' scales [blocks][Hkv][block_rows]
  const uint8_t* k8;
  const uint8_t* v8;
  const float* ksc;
  const float* vsc;
};

MLS_DEV float bload_f32(rsrc_t r, int byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}

// 8 e4m3 bytes of a row times the row's scale -> 8 bf16: e4m3 -> fp32 is exact (what fp8x8_to_bf16 of
// kv_fp8.hip yields, without its detour through bf16), one fp32 product, one rounding
MLS_DEV uint4 fp8x8_dequant(uint32_t d0, uint32_t d1, float sc) {
  const f32x2 s2 = {sc, sc};
  const f32x2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)d0, false) * s2;
  const f32x2 f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)d0, true) * s2;
  const f32x2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)d1, false) * s2;
  const f32x2 f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)d1, true) * s2;
  bf16x8 r;
  r[0] = (bf16)f0[0]; r[1] = (bf16)f0[1]; r[2] = (bf16)f1[0]; r[3] = (bf16)f1[1];
  r[4] = (bf16)f2[0]; r[5] = (bf16)f2[1]; r[6] = (bf16)f3[0]; r[7] = (bf16)f3[1];
  return __builtin_bit_cast(uint4, r);
}

// c ? a : b per dword (v_cndmask; a select of the whole vector went through scratch)
MLS_DEV uint4 sel16(int c, uint4 a, uint4 b) {
  return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

template <bool FP8, bool SPLIT>
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
  const int nsplit = SPLIT ? a.nsplit : 1;
  const int b = blockIdx.z / nsplit, sp = blockIdx.z % nsplit, h = blockIdx.y;
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

  if (q0 >= n) {  // no valid query in this tile: zero rows here, or (SPLIT) from the combine, which reads no partial
    if constexpr (!SPLIT)
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
  // the host bound on past + n covers every tile (else the tail tiles would be dropped silently)
  MLS_CHECK(!SPLIT || ntiles <= a.nsplit * a.tiles_per_split, 314);
  const int kt0 = SPLIT ? sp * a.tiles_per_split : 0;  // this block's run of key tiles: [kt0, kt1)
  const int kt1 = SPLIT ? min(kt0 + a.tiles_per_split, ntiles) : ntiles;  // kt0 >= kt1: an empty split (O = 0, l = 0)
  const int pw = P + qw;  // position of the wave's first query

  // a tile is 64 rows of 16-B chunks, chunk idx = tid + NT i per thread: 16 per row of 8 bf16, or (FP8) 8
  // per row of 16 e4m3 -- bytes [16 (idx & 7), +16) of row idx >> 3
  constexpr int NI = T::ni(NT) / (FP8 ? 2 : 1);
  const int* tab = paged ? a.page_table + (long)slot * a.pages_per_seq : nullptr;
  // kt < kt1 <= ntiles <= ceil(L / 64) <= pages_per_seq: L <= rows_cap = pages_per_seq * 64
  auto page_of = [&](int kt) { return paged && kt < kt1 ? __builtin_amdgcn_readfirstlane(tab[kt]) : 0; };
  uint4 kreg[NI], vreg[NI];
  [[maybe_unused]] float ksr[NI], vsr[NI];  // FP8: the scale of each chunk's row
  // tile kt's run: 64-bit base of its first row, valid bytes = its rows below L (the rest reads 0)
  auto load_tile = [&](int kt, int pg) {
    const bool blk_ok = !paged || (pg >= 0 && pg < a.blocks);
    MLS_CHECK(blk_ok, 313);
    const long row0 = paged ? ((long)(blk_ok ? pg : 0) * a.Hkv + hk) * BKV
                            : ((long)slot * a.Hkv + hk) * a.block_rows + (long)kt * BKV;
    if constexpr (FP8) {
      const uint32_t rows = blk_ok ? (uint32_t)min(BKV, L - kt * BKV) : 0u;
      const rsrc_t kr = make_rsrc(a.k8 + row0 * D, rows * D);
      const rsrc_t vr = make_rsrc(a.v8 + row0 * D, rows * D);
      const rsrc_t ksd = make_rsrc(a.ksc + row0, rows * 4);
      const rsrc_t vsd = make_rsrc(a.vsc + row0, rows * 4);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int idx = tid + NT * i;
        kreg[i] = bload16(kr, idx * 16);
        vreg[i] = bload16(vr, idx * 16);
        ksr[i] = bload_f32(ksd, (idx >> 3) * 4);
        vsr[i] = bload_f32(vsd, (idx >> 3) * 4);
      }
    } else {
      const uint32_t bytes = blk_ok ? (uint32_t)(min(BKV, L - kt * BKV) * D * 2) : 0u;
      const rsrc_t kr = make_rsrc(a.kc + row0 * D, bytes);
      const rsrc_t vr = make_rsrc(a.vc + row0 * D, bytes);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        kreg[i] = bload16(kr, (tid + NT * i) * 16);
        vreg[i] = bload16(vr, (tid + NT * i) * 16);
      }
    }
  };
  const float c = a.scale_log2;
  const int causal = 1;  // (unused: the rule is the template argument)
  const Flash2Tile<D, true> tile_body{acc_o, m_run, l_run, qf, Ks, Vs, causal, pw, L, c, g, fr};
  // (a tile at or past ntiles has no valid byte count: never described.  An unsplit block that got here
  // has a tile, q0 < n; the bf16 unsplit instantiation leaves the test out, because with it the compiler
  // keeps the per-slot row offset's 64-bit multiply inside the tile loop -- docs/PERF_NOTES.md)
  if ((!FP8 && !SPLIT) || kt0 < kt1) {
    // the page id of tile kt + 1 is read one tile early, so its K / V loads do not wait on the table
    int pg_next = page_of(kt0 + 1);
    load_tile(kt0, page_of(kt0));
    for (int kt = kt0; kt < kt1; ++kt) {
      const int kv0 = kt * BKV;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int idx = tid + NT * i;
        if constexpr (FP8) {
          const int row = idx >> 3, ch = (idx & 7) * 2;  // the load's dims are the row's 16-B chunks ch, ch + 1
          const uint4 k0 = fp8x8_dequant(kreg[i].x, kreg[i].y, ksr[i]), k1 = fp8x8_dequant(kreg[i].z, kreg[i].w, ksr[i]);
          const uint4 v0 = fp8x8_dequant(vreg[i].x, vreg[i].y, vsr[i]), v1 = fp8x8_dequant(vreg[i].z, vreg[i].w, vsr[i]);
          // 16 lanes (two rows, an even and an odd one) per 256-B LDS pass: the K swizzle already puts the
          // odd row's even chunks on odd 16-B bank groups; in the V image (row stride 256 + 32 B) the odd
          // row writes its second chunk first for the same effect
          const int od = row & 1;
          const int ca = ch + od, cb = ch + 1 - od;
          *reinterpret_cast<uint4*>(Ks + row * (D * 2) + ((ch ^ (row & (CPR - 1))) * 16)) = k0;
          *reinterpret_cast<uint4*>(Vs + row * T::VST + ca * 16) = sel16(od, v1, v0);
          *reinterpret_cast<uint4*>(Ks + row * (D * 2) + (((ch + 1) ^ (row & (CPR - 1))) * 16)) = k1;
          *reinterpret_cast<uint4*>(Vs + row * T::VST + cb * 16) = sel16(od, v0, v1);
        } else {
          const int row = idx / CPR, ch = idx % CPR;
          *reinterpret_cast<uint4*>(Ks + row * (D * 2) + ((ch ^ (row & (CPR - 1))) * 16)) = kreg[i];
          *reinterpret_cast<uint4*>(Vs + row * T::VST + ch * 16) = vreg[i];
        }
      }
      __syncthreads();
      if (kt + 1 < kt1) {
        load_tile(kt + 1, pg_next);
        pg_next = page_of(kt + 2);
      }
      // keys kv0 + 16t + 4g + j against the query at position pw + fr; the mask (and the sub-tile
      // skip) only where the tile crosses the key range end or the wave's diagonal
      tile_body(kv0, kv0 + BKV > L || kv0 + BKV - 1 > pw);
      __syncthreads();
    }
  }

  float l = l_run + xor16_f(l_run);
  l += xor32_f(l);
  if constexpr (SPLIT) {
    // ---- the partial as it stands: lane (g, fr) holds O[q = qw + fr][16 dt + 4 g .. + 3]; a query with
    // no visible key in this run keeps m = -1e30, l = 0, O = 0 (2^(m - M) is 0 in the combine)
    const int q = qw + fr;
    if (q < a.S) {
      const long row = ((long)sp * a.B * a.S + tokq + q) * a.Hq + h;
      float* po = a.ws_o + row * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < T::DT; ++dt)
        *reinterpret_cast<float4*>(po + 16 * dt) = make_float4(acc_o[dt][0], acc_o[dt][1], acc_o[dt][2], acc_o[dt][3]);
      if (g == 0) *reinterpret_cast<float2*>(a.ws_ml + row * 2) = make_float2(m_run, l);
    }
  } else {
    // ---- normalise (lane-local 1 / l of query fr) and store through LDS as 16-B row stores
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
      // rows at or past the batch row's valid length: zeros, as on the split route
      if (q < a.S)
        st16(a.o + (tokq + q) * a.o_stride + (long)h * D + ch * 8,
             q < n ? ld16(Os + r * OST + ch * 8) : make_uint4(0, 0, 0, 0));
    }
  }
}

// valid queries of batch row b (flash_ctx_kernel's clamps), for the combine's padding rows
MLS_DEV int ctx_valid_queries(const CtxArgs& a, int b) {
  const int slot = a.slot_ids ? a.slot_ids[b] : b;
  const bool slot_ok = slot >= 0 && slot < a.slots;
  const int L = slot_ok ? min(a.lens[b], a.rows_cap) : 0;
  const int P = max(0, min(a.past[b], L));
  return min(L - P, a.S);
}

// one (token, q head) per 32 lanes, 4 output columns per lane; splits summed in split order
__global__ __launch_bounds__(256) void flash_ctx_combine_kernel(const CtxArgs a) {
  constexpr int D = 128;
  const long rows = (long)a.B * a.S * a.Hq;
  const long row = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (row >= rows) return;
  const int d = (threadIdx.x & 31) * 4;
  const int h = (int)(row % a.Hq);
  const long tok = row / a.Hq;
  const int b = (int)(tok / a.S), q = (int)(tok % a.S);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  float l = 0.f;
  if (q < ctx_valid_queries(a, b)) {
    float M = -1e30f;
    for (int s = 0; s < a.nsplit; ++s) M = fmaxf(M, a.ws_ml[(s * rows + row) * 2]);
    for (int s = 0; s < a.nsplit; ++s) {
      const float2 ml = *reinterpret_cast<const float2*>(a.ws_ml + (s * rows + row) * 2);
      const float w = exp2f(ml.x - M);
      const float4 p = *reinterpret_cast<const float4*>(a.ws_o + (s * rows + row) * D + d);
      o.x = fmaf(w, p.x, o.x);
      o.y = fmaf(w, p.y, o.y);
      o.z = fmaf(w, p.z, o.z);
      o.w = fmaf(w, p.w, o.w);
      l = fmaf(w, ml.y, l);
    }
  }
  const float inv_l = l > 0.f ? 1.f / l : 0.f;  // padding rows and tokens with no visible key: zeros
  bf16x4 o4;
  o4[0] = (bf16)(o.x * inv_l);
  o4[1] = (bf16)(o.y * inv_l);
  o4[2] = (bf16)(o.z * inv_l);
  o4[3] = (bf16)(o.w * inv_l);
  *reinterpret_cast<bf16x4*>(a.o + tok * a.o_stride + (long)h * D + d) = o4;
}

}  // namespace

// Every launch of this file: the argument checks, CtxArgs and the kernels.  fp8: e4m3 caches with their
// scales (else bf16 caches, the scales unused); split: the split-KV kernel over `workspace` + the combine
// (else the unsplit kernel; workspace, ws_elems, max_ctx and nsplit unused).
static int ctx_launch(bool fp8, bool split, const void* qkv, const void* k_cache, const void* v_cache,
                      const float* k_scale, const float* v_scale, void* o, void* workspace, long ws_elems,
                      int q_stride, int o_stride, const int* past, const int* lens, const int* slot_ids,
                      const int* page_table, int pages_per_seq, int slots, int B, int S, int Hq, int Hkv, int D,
                      long blocks, int hm_rows, int max_ctx, int nsplit, float scale, void* stream) {
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
  if (fp8 && (!k_scale || !v_scale)) return MLS_BAD_ARG;
  if (fp8 && ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3)) return MLS_BAD_ARG;
  CtxArgs a{};
  a.q = (const bf16*)qkv;
  if (fp8) {
    a.k8 = (const uint8_t*)k_cache;
    a.v8 = (const uint8_t*)v_cache;
    a.ksc = k_scale;
    a.vsc = v_scale;
  } else {
    a.kc = (const bf16*)k_cache;
    a.vc = (const bf16*)v_cache;
  }
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
  a.nsplit = 1;
  const long rows = (long)B * S * Hq;
  if (split) {
    if (nsplit < 1 || nsplit > 64 || max_ctx < 1 || !workspace) return MLS_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return MLS_BAD_ARG;  // 16-B partial stores
    if ((long)B * nsplit > 65535 || rows > 0x7FFFFFFFl / 8) return MLS_BAD_ARG;  // grid z; the combine's grid x
    if (ws_elems < (long)nsplit * rows * (D + 2)) return MLS_BAD_ARG;
    const int ntiles = ((max_ctx < a.rows_cap ? max_ctx : a.rows_cap) + 63) / 64;
    a.nsplit = nsplit;
    a.tiles_per_split = (ntiles + nsplit - 1) / nsplit;
    a.ws_o = (float*)workspace;
    a.ws_ml = a.ws_o + (long)nsplit * rows * D;
  }
  void (*const kernel)(const CtxArgs) =
      fp8 ? (split ? flash_ctx_kernel<true, true> : flash_ctx_kernel<true, false>)
          : (split ? flash_ctx_kernel<false, true> : flash_ctx_kernel<false, false>);
  dim3 grid((S + 63) / 64, Hq, B * a.nsplit);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  if (split)
    hipLaunchKernelGGL(flash_ctx_combine_kernel, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, (hipStream_t)stream,
                       a);
  return (int)hipGetLastError();
}

extern "C" {

// qkv: the chunk's fused projection [B*S][q_stride] (Q heads first, already RoPE'd); caches head-major
// [blocks][Hkv][hm_rows][D] (hm_rows = max_seq per slot, or 64 when paged through page_table
// [slots][pages_per_seq]); past / lens / slot_ids int32 [B] on the device.  hm_rows = 0 (a row-major
// cache), D != 128 and pages of other than 64 rows are unsupported.
int mls_flash_attention_ctx(const void* qkv, const void* k_cache, const void* v_cache, void* o, int q_stride,
                            int o_stride, const int* past, const int* lens, const int* slot_ids,
                            const int* page_table, int pages_per_seq, int slots, int B, int S, int Hq, int Hkv, int D,
                            long blocks, int hm_rows, float scale, void* stream) {
  return ctx_launch(false, false, qkv, k_cache, v_cache, nullptr, nullptr, o, nullptr, 0, q_stride, o_stride, past,
                    lens, slot_ids, page_table, pages_per_seq, slots, B, S, Hq, Hkv, D, blocks, hm_rows, 0, 0, scale,
                    stream);
}

// Split-KV launch of the same contract + the combine.  max_ctx: a host bound on lens[] (past + n); it and
// nsplit fix tiles_per_split = ceil(ceil(min(max_ctx, slot rows) / 64) / nsplit) for every block.
// workspace: fp32, nsplit * B*S*Hq * (D + 2) elements (ws_elems: what the caller holds).
int mls_flash_attention_ctx_split(const void* qkv, const void* k_cache, const void* v_cache, void* o, void* workspace,
                                  long ws_elems, int q_stride, int o_stride, const int* past, const int* lens,
                                  const int* slot_ids, const int* page_table, int pages_per_seq, int slots, int B,
                                  int S, int Hq, int Hkv, int D, long blocks, int hm_rows, int max_ctx, int nsplit,
                                  float scale, void* stream) {
  return ctx_launch(false, true, qkv, k_cache, v_cache, nullptr, nullptr, o, workspace, ws_elems, q_stride, o_stride,
                    past, lens, slot_ids, page_table, pages_per_seq, slots, B, S, Hq, Hkv, D, blocks, hm_rows, max_ctx,
                    nsplit, scale, stream);
}

// mls_flash_attention_ctx / _split on an e4m3 cache (kv_fp8.hip's layout): k_cache / v_cache uint8
// [blocks][Hkv][hm_rows][128], k_scale / v_scale fp32 [blocks][Hkv][hm_rows]; every other argument as
// the bf16 entry points take it, the split partials merged by the same combine kernel.
int mls_flash_attention_ctx_fp8(const void* qkv, const void* k_cache, const void* v_cache, const float* k_scale,
                                const float* v_scale, void* o, int q_stride, int o_stride, const int* past,
                                const int* lens, const int* slot_ids, const int* page_table, int pages_per_seq,
                                int slots, int B, int S, int Hq, int Hkv, int D, long blocks, int hm_rows, float scale,
                                void* stream) {
  return ctx_launch(true, false, qkv, k_cache, v_cache, k_scale, v_scale, o, nullptr, 0, q_stride, o_stride, past,
                    lens, slot_ids, page_table, pages_per_seq, slots, B, S, Hq, Hkv, D, blocks, hm_rows, 0, 0, scale,
                    stream);
}

int mls_flash_attention_ctx_fp8_split(const void* qkv, const void* k_cache, const void* v_cache, const float* k_scale,
                                      const float* v_scale, void* o, void* workspace, long ws_elems, int q_stride,
                                      int o_stride, const int* past, const int* lens, const int* slot_ids,
                                      const int* page_table, int pages_per_seq, int slots, int B, int S, int Hq,
                                      int Hkv, int D, long blocks, int hm_rows, int max_ctx, int nsplit, float scale,
                                      void* stream) {
  return ctx_launch(true, true, qkv, k_cache, v_cache, k_scale, v_scale, o, workspace, ws_elems, q_stride, o_stride,
                    past, lens, slot_ids, page_table, pages_per_seq, slots, B, S, Hq, Hkv, D, blocks, hm_rows, max_ctx,
                    nsplit, scale, stream);
}

}  // extern "C"

MLS_DEBUG_EXPORT(flash_ctx)
