// Per-request LoRA on the o, gate / up and down projections: y[m] += s * B[a] (A[a] . x[m]) for the adapter a
// of row m's sequence, on rows gathered by adapter.  lora.hip (q / k / v) ties a tile to <= 16 consecutive rows
// of one sequence, so 32 decode rows stream their adapters 32 times; here a tile table built once per forward
// names, per tile, an adapter and up to 16 rows that share it -- any rows -- and each adapter's A and B are
// streamed once per tile.  Four kernels, device arrays only (capturable), no atomics, deterministic:
//
//  mls_lora_tiles        one block.  S == 1: a counting sort of the B rows by adapter in LDS (adapters ascending,
//                        rows ascending within one, 16 per tile); S > 1: the runs of <= 16 consecutive rows of each
//                        sequence that has an adapter.  Table (int32): [0] ntiles, [16 ..] tile_adapter[max_tiles],
//                        tile_rows[max_tiles][16] (row or -1), row_flag[B * S] (1: the row is in a tile).  Base rows
//                        get no tile.  Every later grid is sized for the host worst case max_tiles; blocks with
//                        t >= ntiles leave before touching memory.
//  mls_lora_shrink_x     t[tile][16][0:R] = x[row] . A'[a]^T: lane fr of the MFMA A operand reads row
//                        tile_rows[t][fr] (-1: the buffer range check returns zeros).  Split-K over blockIdx.y,
//                        64 columns of t per blockIdx.z, the 4 waves take every 4th k-step and meet in LDS; fp32
//                        slabs [split][tile][16][acap + 1].  PLAIN: x is the bf16 activation; NORMED: x is the
//                        post-add residual, A' = bf16(A diag(gain)) and the row's square sum rides in column acap:
//                        it is the diagonal of one more MFMA per k-step, x against itself (no VALU work).
//                        A [adapter][acap][K]: the group's segments (o | gate, up | down) at the adapter's own
//                        padded rank, end to end.
//  mls_lora_expand_add   y[row][n] += s * rstd * (B[a] t[row])[n] in place.  A block sums the tile's slabs once, in
//                        split order, into LDS (with each row's rstd); each wave then packs its bf16 operand once
//                        and walks `ct` 64-column groups with it, 16 columns per wave and group.  B [adapter][N]
//                        [stride], stride the adapter's padded rank (from seg): N * rpad * 2 bytes per tile.
//  mls_lora_expand_silu  the gate / up form: pre [M][2I] interleaved by 8 (8 gate, 8 up columns per 16), out
//                        [M][I] = silu(g + dg) * (u + du).  Two MFMAs per rank step, one per module (its 8 lanes
//                        load B rows, the other 8 load nothing); gate and up lanes swap within the 16-lane row by
//                        DPP.  Blocks [0, max_tiles) take the tiles; blocks behind them take 16 consecutive rows
//                        each and serve those with row_flag 0, without a delta: mls_silu_mul_interleaved's
//                        arithmetic, bit for bit.
//
// MFMA operand maps as in lora.hip: lane (fr = lane & 15, fq = lane >> 4) holds X[row fr][k 8 fq ..] and
// W[col fr][k 8 fq ..]; acc[i] is D[row 4 fq + i][col fr].
#include "common.h"

namespace {

constexpr int LL_GRAN = 16;      // rank padding
constexpr int LL_MAX_RANK = 64;
constexpr int LL_BN = 64;        // columns per block (4 waves x 16)
constexpr int LL_KG = 128;       // K granule of a split
constexpr int LL_MAX_B = 1024;   // sequences the tile kernel sorts in LDS
constexpr int LL_HDR = 16;       // ints before tile_adapter
constexpr int LL_TCAP = 2 * LL_MAX_RANK;  // widest row of t: gate and up at the largest rank

struct LinArgs {
  const bf16* x;       // [rows][ldx]
  const bf16* A;       // [n_adapt][acap][K]
  const bf16* Bw;      // [n_adapt][N][bcap], rows at the adapter's own stride
  const int* seg;      // [n_adapt][4] padded ranks of o, gate, up, down
  const float* scale;  // [n_adapt][4]
  const int* tab;      // the tile table
  float* ws;           // [nsplit][max_tiles][16][acap + 1]
  bf16* y;             // add form: [rows][ldy] in place; silu form: out [rows][N / 2]
  const bf16* pre;     // silu form: [rows][N]
  int rows, K, ldx, ldy, N, acap, bcap, n_adapt, s0, nseg, max_tiles, nsplit, kchunk, normed, ct;
  float eps;
};

MLS_DEV int ll_ntiles(const LinArgs& g) {
  const int n = g.tab[0];
  MLS_CHECK(n >= 0 && n <= g.max_tiles, 511);
  return n < 0 ? 0 : min(n, g.max_tiles);
}

// tile t's adapter, -1 (serve as base) for anything out of range
MLS_DEV int ll_adapter(const LinArgs& g, int t) {
  const int a = g.tab[LL_HDR + t];
  MLS_CHECK(a >= 0 && a < g.n_adapt, 512);
  return (a < 0 || a >= g.n_adapt) ? -1 : a;
}

// row j of tile t, -1 for none
MLS_DEV int ll_row(const LinArgs& g, int t, int j) {
  const int r = g.tab[LL_HDR + g.max_tiles + t * 16 + j];
  MLS_CHECK(r >= -1 && r < g.rows, 513);
  return (r < 0 || r >= g.rows) ? -1 : r;
}

// the group's padded ranks; false (no delta) unless they fit the pack
MLS_DEV bool ll_ranks(const LinArgs& g, int a, int (&rk)[2]) {
  bool ok = true;
  rk[1] = 0;
  for (int p = 0; p < g.nseg; ++p) {
    rk[p] = g.seg[a * 4 + g.s0 + p];
    ok = ok && rk[p] >= 0 && rk[p] <= g.bcap && rk[p] % LL_GRAN == 0;
  }
  ok = ok && rk[0] + rk[1] <= g.acap;
  MLS_CHECK(ok, 514);
  return ok;
}

__global__ __launch_bounds__(1024) void lora_tiles_kernel(const int* lora_slot, const int* slot_ids, int* tab, int B,
                                                          int S, int n_adapt, int n_slots, int max_tiles) {
  __shared__ int ad[LL_MAX_B], pos[LL_MAX_B], cnt[LL_MAX_B], rstart[LL_MAX_B], tbase[LL_MAX_B + 1], ta[LL_MAX_B];
  const int tid = threadIdx.x;
  int* tile_adapter = tab + LL_HDR;
  int* tile_rows = tile_adapter + max_tiles;
  int* row_flag = tile_rows + (size_t)max_tiles * 16;
  int a = -1;
  if (tid < B) {
    const int slot = slot_ids ? slot_ids[tid] : tid;
    MLS_CHECK(slot >= 0 && slot < n_slots, 501);
    if (slot >= 0 && slot < n_slots) {
      a = lora_slot[slot];
      MLS_CHECK(a >= -1 && a < n_adapt, 502);
      if (a < 0 || a >= n_adapt) a = -1;
    }
    ad[tid] = a;
  }
  __syncthreads();
  if (S == 1) {
    // counting sort by adapter: counts, then each adapter's first tile and first sorted position
    if (tid < n_adapt) {
      int c = 0;
      for (int b = 0; b < B; ++b) c += ad[b] == tid;
      cnt[tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
      int tb = 0, rs = 0;
      for (int j = 0; j < n_adapt; ++j) {
        tbase[j] = tb, rstart[j] = rs;
        tb += (cnt[j] + 15) >> 4, rs += cnt[j];
      }
      tbase[n_adapt] = tb;
    }
    __syncthreads();
    const int ntiles = min(tbase[n_adapt], max_tiles);  // <= min(B, n_adapt + B / 16) by construction
    if (tid < B && a >= 0) {
      int rank = 0;
      for (int b = 0; b < tid; ++b) rank += ad[b] == a;
      pos[rstart[a] + rank] = tid;
    }
    if (tid < n_adapt)
      for (int t = tbase[tid]; t < tbase[tid + 1]; ++t) ta[t] = tid;
    __syncthreads();
    for (int q = tid; q < ntiles * 16; q += 1024) {
      const int t = q >> 4, aa = ta[t], idx = (t - tbase[aa]) * 16 + (q & 15);
      tile_rows[q] = idx < cnt[aa] ? pos[rstart[aa] + idx] : -1;
    }
    if (tid < ntiles) tile_adapter[tid] = ta[tid];
    if (tid < B) row_flag[tid] = a >= 0;
    if (tid == 0) tab[0] = ntiles;
    return;
  }
  // S > 1: the sequences that have an adapter, in order; ceil(S / 16) tiles of consecutive rows each
  const int tps = (S + 15) >> 4;
  int nseq = 0;
  for (int b = 0; b < B; ++b) nseq += ad[b] >= 0;
  if (tid < B && a >= 0) {
    int rank = 0;
    for (int b = 0; b < tid; ++b) rank += ad[b] >= 0;
    pos[rank] = tid;
  }
  __syncthreads();
  const int ntiles = min(nseq * tps, max_tiles);
  for (int q = tid; q < ntiles * 16; q += 1024) {
    const int t = q >> 4, b = pos[t / tps], r = (t % tps) * 16 + (q & 15);
    tile_rows[q] = r < S ? b * S + r : -1;
  }
  for (int t = tid; t < ntiles; t += 1024) tile_adapter[t] = ad[pos[t / tps]];
  for (int m = tid; m < B * S; m += 1024) row_flag[m] = ad[m / S] >= 0;
  if (tid == 0) tab[0] = ntiles;
}

template <bool NORMED>
__global__ __launch_bounds__(256) void lin_shrink_kernel(const LinArgs g) {
  __shared__ float red[4][16][LL_BN + 1];
  __shared__ float ssq_red[4][16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int t = blockIdx.x;
  if (t >= ll_ntiles(g)) return;
  const int a = ll_adapter(g, t);
  if (a < 0) return;
  int rk[2];
  if (!ll_ranks(g, a, rk)) return;
  const int rtot = rk[0] + rk[1];
  const int c0 = blockIdx.z * LL_BN;
  if (c0 >= rtot) return;
  const int split = blockIdx.y, kbeg = split * g.kchunk;
  const int row = ll_row(g, t, fr);

  const rsrc_t rr = make_rsrc(g.x, (uint32_t)(((size_t)(g.rows - 1) * g.ldx + g.K) * 2));
  const rsrc_t ar = make_rsrc(g.A + (size_t)a * g.acap * g.K, (uint32_t)((size_t)rtot * g.K * 2));
  const int x_off = row >= 0 ? (row * g.ldx + kbeg + fq * 8) * 2 : OOB;
  int w_off[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = c0 + j * 16 + fr;
    w_off[j] = col < rtot ? (col * g.K + kbeg + fq * 8) * 2 : OOB;
  }

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 sq = f32x4{0.f, 0.f, 0.f, 0.f};  // NORMED: x . x^T, whose diagonal is the rows' square sums
  const int nk = g.kchunk / 32;  // a multiple of 4: every wave runs nk / 4 steps
  for (int kt = wid; kt < nk; kt += 4) {
    const uint4 xv = bload16(rr, x_off == OOB ? OOB : x_off + kt * 64);
    uint4 wv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wv[j] = bload16(ar, w_off[j] == OOB ? OOB : w_off[j] + kt * 64);
    if constexpr (NORMED)
      sq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xv), __builtin_bit_cast(bf16x8, xv), sq, 0,
                                                   0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xv), __builtin_bit_cast(bf16x8, wv[j]),
                                                       acc[j], 0, 0, 0);
  }
  if constexpr (NORMED) {  // sq[i] is D[row 4 fq + i][col fr]: the diagonal element of row fr sits in lane group fr / 4
    if ((fr >> 2) == fq) ssq_red[wid][fr] = (fr & 2) ? ((fr & 1) ? sq[3] : sq[2]) : ((fr & 1) ? sq[1] : sq[0]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float e = acc[j][i];
      red[wid][fq * 4 + i][j * 16 + fr] = e;
    }
  __syncthreads();

  // all 16 rows of the tile (a row of -1 loaded nothing: zeros), so the expand never meets an unwritten word
  const size_t ldt = (size_t)g.acap + 1;
  float* slab = g.ws + ((size_t)split * g.max_tiles + t) * 16 * ldt;
  for (int q = tid; q < 16 * LL_BN; q += 256) {
    const int m = q / LL_BN, cc = q % LL_BN;
    if (c0 + cc >= rtot) continue;
    slab[m * ldt + c0 + cc] = red[0][m][cc] + red[1][m][cc] + red[2][m][cc] + red[3][m][cc];
  }
  if constexpr (NORMED)
    if (blockIdx.z == 0 && tid < 16)
      slab[tid * ldt + g.acap] = ssq_red[0][tid] + ssq_red[1][tid] + ssq_red[2][tid] + ssq_red[3][tid];
}

// Block prologue of both expands: tile t's rows of t summed over the split-K slabs, once and in split order
// (bit-identical repeats), into LDS, and per segment each row's factor s * rstd (rstd = 1 in the plain form).  The
// shrink wrote all 16 rows of every slab.  Ends with a barrier: every thread of the block must call it.
MLS_DEV void ll_stage(const LinArgs& g, int t, int a, int rtot, float (&ts)[16][LL_TCAP + 1], float (&rs)[2][16]) {
  const size_t ldt = (size_t)g.acap + 1, slab = (size_t)g.max_tiles * 16 * ldt;
  const float* base = g.ws + (size_t)t * 16 * ldt;
  for (int q = threadIdx.x; q < 16 * rtot; q += 256) {
    const int m = q / rtot, c = q - m * rtot;
    const float* src = base + m * ldt + c;
    float v = 0.f;
    for (int s = 0; s < g.nsplit; ++s, src += slab) v += *src;
    ts[m][c] = v;
  }
  if ((int)threadIdx.x < 16 * g.nseg) {
    const int p = threadIdx.x >> 4, m = threadIdx.x & 15;
    float r = 1.f;
    if (g.normed) {
      const float* src = base + m * ldt + g.acap;
      float ss = 0.f;
      for (int s = 0; s < g.nsplit; ++s, src += slab) ss += *src;
      r = rsqrtf(ss / (float)g.K + g.eps);
    }
    rs[p][m] = g.scale[a * 4 + g.s0 + p] * r;
  }
  __syncthreads();
}

// the lane's share of the MFMA A operand, t[row fr][off + 8 fq + 32 j ..] as bf16, for the <= 2 rank steps
MLS_DEV void ll_operand(const float (&ts)[16][LL_TCAP + 1], int fr, int fq, int off, int rp, uint4 (&op)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int kk = j * 32 + fq * 8;
    float tv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (kk < rp) {
#pragma unroll
      for (int e = 0; e < 8; ++e) tv[e] = ts[fr][off + kk + e];
    }
    op[j] = pack8(tv);
  }
}

// D[16 rows][16 columns] = t . B^T for the lane's B row at byte offset b_off (OOB: its column takes no part)
MLS_DEV f32x4 ll_mma(const uint4 (&op)[2], int fq, int rp, rsrc_t br, int b_off) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int kk = j * 32 + fq * 8;
    if (j * 32 >= rp) break;
    const uint4 bw = bload16(br, kk < rp && b_off != OOB ? b_off + kk * 2 : OOB);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, op[j]), __builtin_bit_cast(bf16x8, bw), acc,
                                                  0, 0, 0);
  }
  return acc;
}

__global__ __launch_bounds__(256) void lin_expand_add_kernel(const LinArgs g) {
  __shared__ float ts[16][LL_TCAP + 1];
  __shared__ float rs[2][16];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int t = blockIdx.x;
  if (t >= ll_ntiles(g)) return;  // every exit up to ll_stage is the whole block's
  const int a = ll_adapter(g, t);
  if (a < 0) return;
  int rk[2];
  if (!ll_ranks(g, a, rk)) return;
  const int rp = rk[0];
  if (rp == 0) return;
  ll_stage(g, t, a, rp, ts, rs);
  uint4 op[2];
  ll_operand(ts, fr, fq, 0, rp, op);
  int rows4[4];
  float sc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rows4[i] = ll_row(g, t, fq * 4 + i), sc[i] = rs[0][fq * 4 + i];
  const rsrc_t br = make_rsrc(g.Bw + (size_t)a * g.N * g.bcap, (uint32_t)((size_t)g.N * rp * 2));
  for (int c = 0; c < g.ct; ++c) {
    const int n0 = ((int)blockIdx.y * g.ct + c) * LL_BN + wid * 16;
    if (n0 >= g.N) break;
    const f32x4 acc = ll_mma(op, fq, rp, br, (n0 + fr) * rp * 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (rows4[i] < 0) continue;
      const float d = acc[i];
      bf16* o = g.y + (size_t)rows4[i] * g.ldy + n0 + fr;
      *o = (bf16)((float)*o + d * sc[i]);
    }
  }
}

__global__ __launch_bounds__(256) void lin_expand_silu_kernel(const LinArgs g) {
  __shared__ float ts[16][LL_TCAP + 1];
  __shared__ float rs[2][16];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const bool up = fr >= 8;  // interleaved columns: 8 gate, then 8 up of the same outputs
  int rows4[4], rk[2] = {0, 0}, a = -1;
  float sc[4] = {0.f, 0.f, 0.f, 0.f};
  uint4 opg[2], opu[2];
  bool delta = false;
  if ((int)blockIdx.x >= g.max_tiles) {
    // the rows no tile holds, 16 consecutive ones per block: no delta
    const int* row_flag = g.tab + LL_HDR + (size_t)g.max_tiles * 17;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = ((int)blockIdx.x - g.max_tiles) * 16 + fq * 4 + i;
      rows4[i] = m < g.rows && row_flag[m] == 0 ? m : -1;
    }
  } else {
    const int t = blockIdx.x;
    if (t >= ll_ntiles(g)) return;
    a = ll_adapter(g, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) rows4[i] = ll_row(g, t, fq * 4 + i);
    delta = a >= 0 && ll_ranks(g, a, rk) && (rk[0] | rk[1]);  // the whole block's: ll_stage holds a barrier
    if (!delta) rk[0] = rk[1] = 0;
    if (delta) {
      ll_stage(g, t, a, rk[0] + rk[1], ts, rs);
      ll_operand(ts, fr, fq, 0, rk[0], opg);
      ll_operand(ts, fr, fq, rk[0], rk[1], opu);
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[i] = rs[up ? 1 : 0][fq * 4 + i];
    }
  }
  const bool has = delta && (up ? rk[1] : rk[0]) > 0;
  const int stride = max(rk[0], rk[1]), I = g.N >> 1;
  const rsrc_t br = make_rsrc(g.Bw + (size_t)max(a, 0) * g.N * g.bcap, (uint32_t)((size_t)g.N * stride * 2));
  for (int c = 0; c < g.ct; ++c) {
    const int n0 = ((int)blockIdx.y * g.ct + c) * LL_BN + wid * 16;
    if (n0 >= g.N) break;
    f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
    if (delta) {
      // one MFMA chain per module: its 8 lanes bring B rows, the other 8 columns come out zero
      const int b_off = (n0 + fr) * stride * 2;
      const f32x4 dg = ll_mma(opg, fq, rk[0], br, up ? OOB : b_off);
      const f32x4 du = ll_mma(opu, fq, rk[1], br, up ? b_off : OOB);
      d = up ? du : dg;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rows4[i];
      const float p = row >= 0 ? (float)g.pre[(size_t)row * g.N + n0 + fr] : 0.f;
      const float dv = d[i];
      const float v = has ? p + dv * sc[i] : p;
      const float u = xor8_f(v);  // the up column of this gate lane
      if (row >= 0 && !up) g.y[(size_t)row * I + (n0 >> 4) * 8 + fr] = (bf16)(silu(v) * u);
    }
  }
}

// 64-column groups a block of the expands walks with one staged operand: 1 up to N = 4096 (o, down), 8 from N =
// 32768 (gate / up: the slabs are summed once per 512 columns) -- halved while the grid of `xblocks` row blocks
// would fall under 1024 blocks (4 per CU): with 8, a batch-1 decode step ran its one tile on 112 blocks and
// measured 0.27 ms per step slower than with 1 (docs/PERF_NOTES.md, "LoRA on every projection")
int ll_ct(int N, int ct, int xblocks) {
  if (ct > 0) return min(ct, 64);
  ct = N >= 32768 ? 8 : N >= 8192 ? N / 4096 : 1;
  while (ct > 1 && (long)xblocks * ((N + LL_BN * ct - 1) / (LL_BN * ct)) < 1024) ct >>= 1;
  return ct;
}

bool ll_geometry_ok(int rows, int K, int acap, int bcap, int nseg, int s0, int max_tiles, int nsplit) {
  return rows > 0 && rows < (1 << 24) && K > 0 && K % LL_KG == 0 && K <= (1 << 20) && bcap > 0 && bcap % LL_GRAN == 0 &&
         bcap <= LL_MAX_RANK && nseg >= 1 && nseg <= 2 && s0 >= 0 && s0 + nseg <= 4 && acap == nseg * bcap &&
         max_tiles > 0 && max_tiles < (1 << 20) && nsplit >= 1 && nsplit <= 64 && K % (nsplit * LL_KG) == 0;
}

size_t ll_ws_bytes(int max_tiles, int acap, int nsplit) { return (size_t)nsplit * max_tiles * 16 * (acap + 1) * 4; }

}  // namespace

MLS_DEBUG_EXPORT(lora_linear)

extern "C" {

// the tiles a table of B sequences of S rows over n_adapt adapters can hold (what every grid is sized for)
int mls_lora_max_tiles(int B, int S, int n_adapt) {
  if (B <= 0 || S <= 0 || n_adapt <= 0) return 0;
  if (S > 1) return B * ((S + 15) / 16);
  return B < n_adapt + B / 16 ? B : n_adapt + B / 16;
}

// int32 words of the table (0: B * S beyond what the kernels take)
int mls_lora_table_elems(int B, int S, int n_adapt) {
  if (B <= 0 || S <= 0 || (long)B * S >= (1l << 24)) return 0;
  return (int)(LL_HDR + (long)mls_lora_max_tiles(B, S, n_adapt) * 17 + (long)B * S);
}

// lora_slot [n_slots] int32; slot_ids [B] int32 or null; tab >= mls_lora_table_elems int32 words
int mls_lora_tiles(const int* lora_slot, const int* slot_ids, int* tab, size_t tab_bytes, int B, int S, int n_adapt,
                   int n_slots, void* stream) {
  if (!lora_slot || !tab || B <= 0 || S <= 0 || n_adapt <= 0 || n_slots <= 0) return MLS_BAD_ARG;
  if (!slot_ids && B > n_slots) return MLS_BAD_ARG;
  if (B > LL_MAX_B || n_adapt > LL_MAX_B || (long)B * S >= (1l << 24)) return MLS_UNSUPPORTED;
  if (tab_bytes < (size_t)mls_lora_table_elems(B, S, n_adapt) * 4) return MLS_BAD_ARG;
  if (mls_lora_max_tiles(B, S, n_adapt) >= (1 << 20)) return MLS_UNSUPPORTED;
  hipLaunchKernelGGL(lora_tiles_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, lora_slot, slot_ids, tab, B, S,
                     n_adapt, n_slots, mls_lora_max_tiles(B, S, n_adapt));
  return (int)hipGetLastError();
}

// x [rows][ldx] bf16; A [n_adapt][acap][K] bf16, acap = nseg * bcap; seg [n_adapt][4] int32, the group's segments
// s0 .. s0 + nseg - 1; tab: what mls_lora_tiles wrote for these rows (max_tiles as it sized it); ws >= nsplit *
// max_tiles * 16 * (acap + 1) floats.  normed: x is the residual, its square sum goes to column acap.
int mls_lora_shrink_x(const void* x, int ldx, const void* A, const int* seg, const int* tab, void* ws, size_t ws_bytes,
                      int rows, int K, int acap, int bcap, int s0, int nseg, int n_adapt, int max_tiles, int nsplit,
                      int normed, void* stream) {
  if (!x || !A || !seg || !tab || !ws || n_adapt <= 0 || ldx < K || ldx % 8 ||
      !ll_geometry_ok(rows, K, acap, bcap, nseg, s0, max_tiles, nsplit))
    return MLS_BAD_ARG;
  if (ws_bytes < ll_ws_bytes(max_tiles, acap, nsplit)) return MLS_BAD_ARG;
  if ((size_t)rows * ldx * 2 >= 0x80000000ull || (size_t)acap * K * 2 >= 0x80000000ull) return MLS_UNSUPPORTED;
  LinArgs g{};
  g.x = (const bf16*)x, g.A = (const bf16*)A, g.seg = seg, g.tab = tab, g.ws = (float*)ws;
  g.rows = rows, g.K = K, g.ldx = ldx, g.acap = acap, g.bcap = bcap, g.n_adapt = n_adapt, g.s0 = s0, g.nseg = nseg;
  g.max_tiles = max_tiles, g.nsplit = nsplit, g.kchunk = K / nsplit, g.normed = normed;
  const dim3 grid(max_tiles, nsplit, (acap + LL_BN - 1) / LL_BN);
  if (normed) hipLaunchKernelGGL(lin_shrink_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(lin_shrink_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

// y [rows][ldy] bf16 in place, N % 16 == 0; Bw [n_adapt][N][bcap] bf16 with the adapter's rows at stride seg[a][s0];
// one segment.  ws: what mls_lora_shrink_x wrote with the same table, acap, nsplit and normed.  ct: 64-column
// groups per block, 0: the rule ll_ct.
int mls_lora_expand_add(void* y, int ldy, const void* Bw, const int* seg, const float* scale, const int* tab,
                        const void* ws, size_t ws_bytes, int rows, int N, int K, float eps, int bcap, int s0, int n_adapt,
                        int max_tiles, int nsplit, int normed, int ct, void* stream) {
  if (!y || !Bw || !seg || !scale || !tab || !ws || n_adapt <= 0 || N <= 0 || N % 16 || ldy < N ||
      !ll_geometry_ok(rows, K, bcap, bcap, 1, s0, max_tiles, nsplit))
    return MLS_BAD_ARG;
  if (ws_bytes < ll_ws_bytes(max_tiles, bcap, nsplit)) return MLS_BAD_ARG;
  if ((size_t)N * bcap * 2 >= 0x80000000ull) return MLS_UNSUPPORTED;
  LinArgs g{};
  g.y = (bf16*)y, g.Bw = (const bf16*)Bw, g.seg = seg, g.scale = scale, g.tab = tab, g.ws = (float*)const_cast<void*>(ws);
  g.rows = rows, g.K = K, g.ldy = ldy, g.N = N, g.acap = bcap, g.bcap = bcap, g.n_adapt = n_adapt, g.s0 = s0, g.nseg = 1;
  g.max_tiles = max_tiles, g.nsplit = nsplit, g.kchunk = K / nsplit, g.normed = normed, g.eps = eps;
  g.ct = ll_ct(N, ct, max_tiles);
  hipLaunchKernelGGL(lin_expand_add_kernel, dim3(max_tiles, (N + LL_BN * g.ct - 1) / (LL_BN * g.ct)), dim3(256), 0,
                     (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

// pre [rows][N] bf16, gate / up interleaved by 8 (N = 2 I, I % 8 == 0); out [rows][I] bf16, every row written;
// Bw [n_adapt][N][bcap] interleaved likewise, rows at stride max(seg[a][s0], seg[a][s0 + 1]); two segments.
int mls_lora_expand_silu(const void* pre, void* out, const void* Bw, const int* seg, const float* scale, const int* tab,
                         const void* ws, size_t ws_bytes, int rows, int N, int K, float eps, int bcap, int s0,
                         int n_adapt, int max_tiles, int nsplit, int normed, int ct, void* stream) {
  if (!pre || !out || pre == out || !Bw || !seg || !scale || !tab || !ws || n_adapt <= 0 || N <= 0 || N % 16 ||
      !ll_geometry_ok(rows, K, 2 * bcap, bcap, 2, s0, max_tiles, nsplit))
    return MLS_BAD_ARG;
  if (ws_bytes < ll_ws_bytes(max_tiles, 2 * bcap, nsplit)) return MLS_BAD_ARG;
  if ((size_t)N * bcap * 2 >= 0x80000000ull) return MLS_UNSUPPORTED;
  LinArgs g{};
  g.pre = (const bf16*)pre, g.y = (bf16*)out, g.Bw = (const bf16*)Bw, g.seg = seg, g.scale = scale, g.tab = tab;
  g.ws = (float*)const_cast<void*>(ws);
  g.rows = rows, g.K = K, g.N = N, g.acap = 2 * bcap, g.bcap = bcap, g.n_adapt = n_adapt, g.s0 = s0, g.nseg = 2;
  g.max_tiles = max_tiles, g.nsplit = nsplit, g.kchunk = K / nsplit, g.normed = normed, g.eps = eps;
  g.ct = ll_ct(N, ct, max_tiles + (rows + 15) / 16);
  hipLaunchKernelGGL(lin_expand_silu_kernel,
                     dim3(max_tiles + (rows + 15) / 16, (N + LL_BN * g.ct - 1) / (LL_BN * g.ct)), dim3(256), 0,
                     (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

}  // extern "C"
