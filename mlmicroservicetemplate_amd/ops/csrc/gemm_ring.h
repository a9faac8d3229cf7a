// The persistent LDS-DMA tile GEMM that gemm_tile.hip (bf16) and gemm_w8a8.hip (e4m3 on the block-scaled
// MFMA) share:
//     out[M][N] = act(A[M][K] . W[N][K]^T (* xs[m] * ws[n]) + bias[N]) (+ residual[M][N])
// the ring primitives, the in-launch split-K combine, the tile epilogue and the host-side split-K / grid
// rules.  A 128-B LDS row is 64 bf16 or 128 e4m3 k values; an element type brings its argument struct,
// its fragment reads + MFMAs, and its own copy of the persistent ring loop (below).
//
// Design (cdna_hip_programming.md §5, "glds vs register staging" and "Pipelining across barriers"):
//  * both operands are K-contiguous (activations [M][K], weights [N][K]), so every MFMA fragment is
//    16-B ds_read_b128s from one LDS row (ROWB = 128 B, or 64 B for the BK = 32 bf16 tiles);
//  * operands reach LDS by LDS-DMA (buffer_load ... lds, 16 B per lane): no VGPR staging, no
//    ds_write pass; the LDS image is lane-linear, so the bank swizzle is applied on the SOURCE
//    address and the same involution on the read (rule 21): 16-B chunk c of row r lives at chunk
//    c ^ ((r >> 1) & 7), conflict-free for the gfx950 ds_read_b128 lane groups over the 16 rows of
//    a fragment read (checked against the 4 x 16-lane group table);
//  * a STAGES-deep ring (2 for the 256 x 256 tile = 128 KB, 3-4 for the smaller tiles): stage t + S - 1
//    is issued right after the barrier that retires stage t, one barrier per K-step, counted
//    `s_waitcnt vmcnt(N)` (never 0 in steady state) and a raw s_barrier, so the DMA of the next
//    stages stays in flight across the barrier while the MFMAs of this one run;
//  * swapped product: the MFMA computes D = W_tile . A_tile^T, so each lane's 4 accumulators are 4
//    consecutive OUTPUT COLUMNS of one row -> wide bias / residual loads and output stores per lane,
//    and the SiLU-mul pairing (gate / up interleaved in groups of 8 columns) is one lane^32 swap;
//  * XCD-aware bijective block remap, tiles ordered N-fastest inside an XCD so the blocks sharing
//    an A panel (and the whole, L2-sized weight matrix of a BERT projection) share one L2;
//  * rows past M and columns past N read as zero through the buffer range check (offset OOB) and are
//    never stored.  No data-dependent addressing: every offset is a function of the launch shape.
//
// The ring loop: work unit = (tile, K split), unit u -> tile u / S, split u % S (the S splits of a tile are
// adjacent units, so they land on one XCD and its reducer reads same-XCD slabs); persistent: block b takes
// units b', b' + G, ... where b' = XCD-contiguous remap of b, and the loader cursor runs ahead across unit
// boundaries, so a unit's epilogue overlaps the next unit's first DMAs.  Written in bytes (source row pitch,
// nk = pitch / ROWB / S) gemm_tile_kernel's and gemm_w8a8_kernel's loops are the same loop, but it STAYS IN
// EACH KERNEL: as a force-inlined function template taking the k-step, the unit epilogue and the stamp hook
// as callables it moved code in all 25 ring instantiations of gemm_tile.hip -- cfg 1: 333 opcode hunks,
// 11 -> 12 spilled SGPRs; the LayerNorm build of cfg 15: 245 -> 251 VGPRs -- whether it read a byte-typed
// argument struct or the kernel's own, derived nk from the pitch or took it, and with plain or always_inline
// closures (docs/PERF_NOTES.md, "csrc/gemm_ring.h").  A change to one loop must be made in the other.
//
// The epilogue is a template over the kernel's argument struct G: G::SCALED selects fma(acc, xs * ws, bias)
// over acc + bias.  The LayerNorm-folding forms (EPI 3 / 4, PART), which only gemm_tile.hip instantiates,
// sit in the same (row block, column pair) body because they share every load, swap and store of it --
// taken out they would be a second copy of that body.  With the pieces here every kernel of gemm_tile.hip
// compiles to the opcode sequence it had before, and the W8 kernels keep their k-loops and resources.
#pragma once
#include "common.h"

#define GLDS3 __attribute__((address_space(3)))
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

MLS_DEV void ring_glds16(rsrc_t r, char* lds, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (GLDS3 void*)lds, 16, voff, soff, 0, 0);
}

template <int N>
MLS_DEV void ring_wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

MLS_DEV void ring_barrier() {
  // LDS-only wait + raw barrier: __syncthreads() would also wait vmcnt(0) and drain the ring
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// 16-B chunk swizzle of an LDS row: 128-B rows (8 chunks): chunk ^ ((r >> 1) & 7); 64-B rows (4
// chunks, the BK = 32 bf16 tiles): chunk ^ ((r & 1) | ((r >> 1) & 2)).  Both make the 16-row fragment
// reads conflict-free for the four gfx950 ds_read_b128 lane groups.
template <int ROWB>
MLS_DEV int ring_swz(int row) {
  static_assert(ROWB == 128 || ROWB == 64, "LDS row");
  if constexpr (ROWB == 128) return (row >> 1) & 7;
  else return (row & 1) | ((row >> 1) & 2);
}

// Logical tile t -> (tm, tn) in GROUP_M-row bands walked column by column: t = band * (GM * tiles_n)
// + tn * gm + (tm - band * GM).  A persistent round hands each XCD 32 consecutive t = a 4 x 8 block
// of tiles (4 A panels + 8 W panels live in that XCD's L2 instead of 1 + 32 for a row-major walk:
// profiles/r3_gemm_tile_pmc.txt measured the row-major order at a 50 % L2 hit rate, 2.7x the HBM
// bytes of hipBLASLt on the same 256 x 256 tile).
constexpr int RING_GROUP_M = 4;
MLS_DEV void ring_tile(int t, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int per_band = RING_GROUP_M * tiles_n;
  const int band = t / per_band, first = band * RING_GROUP_M;
  const int gm = tiles_m - first < RING_GROUP_M ? tiles_m - first : RING_GROUP_M;
  const int r = t - band * per_band;
  tn = r / gm;
  tm = first + (r - tn * gm);
}

// wait until at most N of this wave's DMA groups are outstanding, N = LOADS * min(S - 2, left)
template <int STAGES, int LOADS>
MLS_DEV void ring_wait(int left) {
  if constexpr (STAGES == 2) {
    ring_wait_vmcnt<0>();
  } else if constexpr (STAGES == 3) {
    if (left >= 1) ring_wait_vmcnt<LOADS>();
    else ring_wait_vmcnt<0>();
  } else {
    static_assert(STAGES == 4, "ring depth");
    if (left >= 2) ring_wait_vmcnt<2 * LOADS>();
    else if (left == 1) ring_wait_vmcnt<LOADS>();
    else ring_wait_vmcnt<0>();
  }
}

// ------------------------------------------------------------------------------------ split-K
// In-launch split-K combine (cdna_hip_programming.md §5 "Projection GEMM", item 2): each K-split
// block writes its fp32 partial tile as a fragment-linear slab (lane-contiguous 16 B, 1 KB per wave
// instruction), retires it, and one lane releases at agent scope and draws a ticket from the tile's
// counter; the split that draws S - 1 is the reducer: acquire, add the other S - 1 slabs into its
// accumulators, reset the counter for the next launch, and run the normal epilogue.  Returns true
// for the reducer; the others return with zeroed accumulators.  Correct for any placement of a
// tile's splits (adjacent units -> same XCD in practice, the fast case).
//   ws  [tiles][S][TILE_ELEMS] fp32 partial tiles; cnt [tiles] arrival counters, zero before the launch
template <int TILE_ELEMS, int MT, int NTL>
MLS_DEV bool ring_splitk_arrive(f32x4 (&acc)[MT][NTL], float* ws, int* cnt, int S, int tile, int split, int* flag) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  f32x4* const tile_ws = reinterpret_cast<f32x4*>(ws + (size_t)tile * S * TILE_ELEMS);
  const int frag0 = wid * MT * NTL * 64 + lane;  // this lane's first f32x4 in a slab
  f32x4* mine = tile_ws + (size_t)split * (TILE_ELEMS / 4) + frag0;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int jn = 0; jn < NTL; ++jn) mine[(i * NTL + jn) * 64] = acc[i][jn];
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // every wave: its slab stores (and the ring's DMAs) retired
  ring_barrier();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    const int old = __hip_atomic_fetch_add(cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == S - 1;
    if (last) {
      __hip_atomic_store(cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __builtin_amdgcn_s_waitcnt(0x0F70);
    }
    *flag = last;
  }
  ring_barrier();
  const bool last = __builtin_amdgcn_readfirstlane(*flag) != 0;
  ring_barrier();  // flag read by every wave before it can be rewritten by this block's next unit
  if (!last) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    return false;
  }
  // sum ALL S slabs (its own re-read too) in split order: the result does not depend on which
  // split arrived last, so repeated launches are bit-identical
  for (int s2 = 0; s2 < S; ++s2) {
    const f32x4* slab = tile_ws + (size_t)s2 * (TILE_ELEMS / 4) + frag0;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      f32x4 t[NTL];
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn) t[jn] = slab[(i * NTL + jn) * 64];
#pragma unroll
      for (int jn = 0; jn < NTL; ++jn) acc[i][jn] = s2 == 0 ? t[jn] : acc[i][jn] + t[jn];
      __builtin_amdgcn_sched_barrier(0);  // NTL loads in flight at a time: the accumulators fill the file
    }
  }
  return true;
}

// ------------------------------------------------------------------------------------ epilogue
// Tile epilogue shared by every variant: lane (fr, fq) holds D[n = 4*fq + e][m = fr] of each 16 x 16
// MFMA tile = row m, 4 consecutive output columns.  Written so no memory op sits behind a per-element
// branch (cdna_hip_programming.md §5 item 4(c): hipcc would wait vmcnt(0) per element -- one
// dependent L2 round trip per (i, jn), ~32 per tile, measured as ~15 us of a 40 us BERT GEMM):
//  * bias / column scales: 16-B range-checked buffer loads (OOB -> 0) in the stores' layout;
//  * residual: range-checked buffer loads (OOB -> 0), two 16-row blocks ahead of their use;
//  * stores: range-checked buffer stores (rows >= M and columns >= N land on the OOB offset).
// EPI: 0 bias (+ act), 1 bias + residual (+ act), 2 SiLU-mul.  One specialisation per kind so the
// unrolled (i, pair) body is straight-line code: a runtime act / residual / SiLU branch inside it made
// hipcc re-home all 128 accumulator registers at every join (~500 instructions per store, measured
// by in-kernel stamps at 31-60k cycles per 256 x 256 tile epilogue).
// 16-B stores (T21, on the 16x16 fragment): v_permlane16_swap over the column tiles (2p, 2p + 1)
// gives each lane 8 consecutive columns of its row -- fq 0: tile 2p cols 0-7, fq 1: tile 2p+1 cols
// 0-7, fq 2: tile 2p cols 8-15, fq 3: tile 2p+1 cols 8-15 -- so a wave stores 16 rows x 64 B per
// instruction: half the store instructions of the bf16x4-per-lane layout (the tail is store-ISSUE
// bound: MI355X_MICROARCH.md, 'attention epilogue store tail').
// G (the kernel's argument struct) supplies bias, res, out, M, N, K, ldo, res_pitch(), flags and G::SCALED;
// SCALED: v = fma(acc, xs[m] * wsc[n], bias) with one fp32 scale per row (g.xs) and per column (g.wsc)
// in place of acc + bias.  EPI 3 / 4 and PART read the LayerNorm-folding fields of gemm_tile.hip.

// ablation flags (g.flags; tools/gemm_tile_probe.py --ablate; cfg bits 8+ of mls_gemm_tile): timing-only
// builds of the same instruction stream (cdna_hip_programming.md §7, "price ONE buffer's traffic")
constexpr int GT_ABL_NOLOAD = 1;   // zero-record A / W descriptors: every DMA dropped by the range check
constexpr int GT_ABL_NOSTORE = 2;  // epilogue stores land on a zero-record descriptor (dropped)
constexpr int GT_ABL_NOBIAS = 4;   // epilogue skips the bias loads

// Row statistics of this lane's MT epilogue rows from the [M][P][2] partials a PART epilogue wrote
// (P = width / 128 <= 8 partials per row, 128 columns each, P even): lane fq loads partials 2fq and 2fq + 1
// with one 16-B load (issued first, beside the bias loads), then two lane swaps finish the row in a
// fixed order -- deterministic.  ring_row_stats_finish returns rmu = -mu * rstd and rrs = rstd.
template <int MT>
MLS_DEV void ring_row_stats_issue(const float* part, int width, int m0, int rows, int wrow, uint4 (&t)[MT]) {
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int P = width >> 7;
  const rsrc_t rp = make_rsrc(part + (size_t)m0 * P * 2, (uint32_t)(rows * P * 8));
#pragma unroll
  for (int i = 0; i < MT; ++i) t[i] = bload16(rp, 2 * fq < P ? ((wrow + i * 16 + fr) * P + 2 * fq) * 8 : OOB);
}
template <int MT>
MLS_DEV void ring_row_stats_finish(const uint4 (&t)[MT], int width, float eps, float (&rmu)[MT], float (&rrs)[MT]) {
  const float invn = 1.f / (float)width;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    float s1 = __uint_as_float(t[i].x) + __uint_as_float(t[i].z);
    float s2 = __uint_as_float(t[i].y) + __uint_as_float(t[i].w);
    s1 += xor16_f(s1);
    s2 += xor16_f(s2);
    s1 += xor32_f(s1);
    s2 += xor32_f(s2);
    const float mu = s1 * invn;
    const float r = rsqrtf(fmaxf(s2 * invn - mu * mu, 0.f) + eps);
    rrs[i] = r;
    rmu[i] = -mu * r;
  }
}

// EPI 3: bias + LayerNorm(residual) (row statistics from g.ln_part, fp32 gamma per column; the LN's
// beta is folded into the bias by the caller);
// EPI 4: LN-folded A: rstd * (acc - mu * fold_c) + bias (+ act), A-row statistics from g.ln_part.
// PART: also accumulate each output row's sum / sum of squares over this wave's columns (of the bf16
// values stored); the two waves of each 128-column block combine theirs through LDS (pscr: [WN][BM]
// float2 past the ring, one block barrier) and one thread per (row, block) stores the pair to
// g.stats_part.  Every wave of the block runs the same epilogue, so the barrier is uniform.
template <int MT, int NTL, int EPI, int ACT, bool PART = false, int BM = 256, int WN = 4, class G>
MLS_DEV void ring_epilogue_t(f32x4 (&acc)[MT][NTL], const G& g, int m0, int n0, int wrow, int wcol,
                             float* pscr = nullptr) {
  static_assert(NTL % 2 == 0, "column tiles pair up");
  static_assert(!G::SCALED || (EPI <= 2 && !PART), "the scaled form has no LayerNorm folding");
  constexpr bool RES = EPI == 1 || EPI == 3;
  // the LayerNorm forms hold per-row values (stats, partial sums) across the column loop: the 256-row
  // tile (MT = 8) walks its rows in two halves, each re-reading the (L1-resident) column vectors, so
  // the per-row arrays stay at 4 entries (the whole tile at once spilled 8-19 VGPRs)
  constexpr int RH = (EPI >= 3 || PART) && MT >= 8 ? 2 : 1, MH = MT / RH;
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int ldr = g.res_pitch();  // residual row pitch in elements
  const int ldo2 = g.ldo * 2, ldr2 = ldr * 2;
  const int rows = g.M - m0 < 256 ? g.M - m0 : 256;  // valid rows of this tile (tiles are <= 256 tall)
  const bool nostore = g.flags & GT_ABL_NOSTORE;
  const rsrc_t ro = make_rsrc(g.out + (size_t)m0 * g.ldo, nostore ? 0u : (uint32_t)(rows * ldo2));
  const rsrc_t rr = make_rsrc(RES ? g.res + (size_t)m0 * ldr : g.out, RES ? (uint32_t)(rows * ldr2) : 0u);
  const bool use_bias = g.bias && !(g.flags & GT_ABL_NOBIAS);
  const rsrc_t rb = make_rsrc(use_bias ? (const void*)g.bias : (const void*)g.out, use_bias ? (uint32_t)g.N * 4u : 0u);
  rsrc_t rg = rb;  // EPI 3: the residual LN's gamma; EPI 4: fold_c; SCALED: the column scales
  if constexpr (EPI == 3) rg = make_rsrc(g.ln_g, (uint32_t)g.N * 4u);
  else if constexpr (EPI == 4) rg = make_rsrc(g.fold_c, (uint32_t)g.N * 4u);
  else if constexpr (G::SCALED) rg = make_rsrc(g.wsc, (uint32_t)g.N * 4u);
  rsrc_t rx = rb;  // SCALED: the row scales
  if constexpr (G::SCALED) rx = make_rsrc(g.xs + m0, (uint32_t)rows * 4u);
  const int sub = (fq & 1) * 16 + (fq >> 1) * 8;  // this lane's 8 columns within the 32-column pair
  float xs[G::SCALED ? MT : 1];
  if constexpr (G::SCALED) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
      xs[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, (wrow + i * 16 + fr) * 4, 0, 0));
  }
#pragma unroll
  for (int h = 0; h < RH; ++h) {
    const int hrow = wrow + h * MH * 16;  // first row of this half (within the tile)
    // per-row (-mu * rstd, rstd) of this lane's rows (EPI 3 / 4) and partial sums (PART)
    float rmu[MH], rrs[MH], ps1[MH], ps2[MH];
#pragma unroll
    for (int i = 0; i < MH; ++i) ps1[i] = ps2[i] = 0.f;
    constexpr bool STATS = EPI == 3 || EPI == 4;
    const int lnw = EPI == 3 ? g.N : g.K;  // the LN'd rows' width: the residual's (N) or A's (K)
    uint4 st[MH];
    if constexpr (STATS) ring_row_stats_issue<MH>(g.ln_part, lnw, m0, rows, hrow, st);
#pragma unroll
    for (int p = 0; p < NTL / 2; ++p) {
      const int c0 = n0 + wcol + p * 32, c = c0 + sub;
      const bool col_ok = c < g.N;  // N % 16 == 0: an 8-column run is wholly in or out
      const f32x4 b_lo = __builtin_bit_cast(f32x4, bload16(rb, col_ok ? c * 4 : OOB));
      const f32x4 b_hi = __builtin_bit_cast(f32x4, bload16(rb, col_ok ? c * 4 + 16 : OOB));
      f32x4 g_lo = {0.f, 0.f, 0.f, 0.f}, g_hi = g_lo;
      if constexpr (STATS || G::SCALED) {
        g_lo = __builtin_bit_cast(f32x4, bload16(rg, col_ok ? c * 4 : OOB));
        g_hi = __builtin_bit_cast(f32x4, bload16(rg, col_ok ? c * 4 + 16 : OOB));
      }
      if constexpr (STATS)
        if (p == 0) ring_row_stats_finish<MH>(st, lnw, g.eps, rmu, rrs);  // its loads flew beside the bias
      // residual rows two 16-row blocks ahead (a whole column of them live would cost 32 VGPRs and
      // spill the 256 x 256 tile).  The SCALED form loads each block where it uses it: two ahead, with the
      // row and column scales live as well, took its 256 x 256 kernel from 2 to 3 spilled SGPRs
      constexpr bool AHEAD = RES && !G::SCALED;
      const int roff = col_ok ? (hrow + fr) * ldr2 + c * 2 : OOB;
      uint4 rv0 = {0, 0, 0, 0}, rv1 = {0, 0, 0, 0};
      if constexpr (AHEAD) {
        rv0 = bload16(rr, roff);
        if (MH > 1) rv1 = bload16(rr, col_ok ? roff + 16 * ldr2 : OOB);
      }
#pragma unroll
      for (int i = 0; i < MH; ++i) {
        const int ia = h * MH + i;        // accumulator row block
        const int r = hrow + i * 16 + fr;  // row within the tile
        uint4 rcur = rv0;
        if constexpr (AHEAD) {
          rv0 = rv1;
          if (i + 2 < MH) rv1 = bload16(rr, col_ok ? roff + (i + 2) * 16 * ldr2 : OOB);
        } else if constexpr (RES) {
          rcur = bload16(rr, col_ok ? r * ldr2 + c * 2 : OOB);
        }
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // __float_as_uint, not __builtin_bit_cast: hipcc (ROCm 7.2) folds a bit_cast of an ext-vector
          // element feeding this builtin to element 0 -- one swap for all four (checked in the .s)
          const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[ia][2 * p][e]),
                                                           __float_as_uint(acc[ia][2 * p + 1][e]), false, false);
          if constexpr (EPI == 4) {  // rstd * (acc - mu * c) + b
            v[e] = fmaf(rrs[i], __uint_as_float(sw[0]), fmaf(rmu[i], g_lo[e], b_lo[e]));
            v[4 + e] = fmaf(rrs[i], __uint_as_float(sw[1]), fmaf(rmu[i], g_hi[e], b_hi[e]));
          } else if constexpr (G::SCALED) {
            v[e] = fmaf(__uint_as_float(sw[0]), xs[ia] * g_lo[e], b_lo[e]);
            v[4 + e] = fmaf(__uint_as_float(sw[1]), xs[ia] * g_hi[e], b_hi[e]);
          } else {
            v[e] = __uint_as_float(sw[0]) + b_lo[e];
            v[4 + e] = __uint_as_float(sw[1]) + b_hi[e];
          }
        }
        bf16x8 o;
        int off;
        if constexpr (EPI == 2) {
          // gate lanes fq 0/1 (tile 2p / 2p+1 cols 0-7) pair with their up columns on lanes fq 2/3
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (bf16)(silu_fast(v[e]) * xor32_f(v[e]));
          off = fq < 2 && col_ok ? r * ldo2 + ((c0 >> 1) + fq * 8) * 2 : OOB;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = v[e];
            v[e] = ACT == ACT_GELU ? gelu_fast(x) : ACT == ACT_RELU ? fmaxf(x, 0.f) : ACT == ACT_SILU ? silu_fast(x)
                   : ACT == ACT_TANH ? tanhf(x) : x;
          }
          if constexpr (EPI == 1) {
            const bf16x8 rb8 = __builtin_bit_cast(bf16x8, rcur);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += (float)rb8[e];
          } else if constexpr (EPI == 3) {
            const bf16x8 rb8 = __builtin_bit_cast(bf16x8, rcur);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float n = fmaf((float)rb8[e], rrs[i], rmu[i]);  // (r - mu) * rstd
              v[e] = fmaf(n, e < 4 ? g_lo[e] : g_hi[e - 4], v[e]);
            }
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (bf16)v[e];
          if constexpr (PART) {  // columns >= N read as zero (residual / accumulators) and add nothing
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float q = col_ok ? (float)o[e] : 0.f;
              ps1[i] += q;
              ps2[i] = fmaf(q, q, ps2[i]);
            }
          }
          off = col_ok ? r * ldo2 + c * 2 : OOB;
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ro, off, 0, 0);
        __builtin_amdgcn_sched_barrier(0);  // keep each row block's live range to itself
      }
    }
    if constexpr (PART) {
      // the 4 lanes fq of a row hold different columns: finish the wave's sums, lanes fq 0 park them
      static_assert(NTL * 16 == 64, "two 64-column waves per 128-column partial");
      const int wn = wcol / 64;
#pragma unroll
      for (int i = 0; i < MH; ++i) {
        float a = ps1[i], b = ps2[i];
        a += xor16_f(a);
        b += xor16_f(b);
        a += xor32_f(a);
        b += xor32_f(b);
        if (fq == 0) {
          float2 v;
          v.x = a;
          v.y = b;
          reinterpret_cast<float2*>(pscr)[wn * BM + hrow + i * 16 + fr] = v;
        }
      }
    }
  }
  if constexpr (PART) {
    // one thread per (row, 128-column block of this tile): add the block's two waves, store the pair
    constexpr int BN = WN * 64, QB = BN / 128;
    static_assert(QB >= 1, "tile covers whole 128-column blocks");
    const int P = g.N >> 7;
    ring_barrier();
    const rsrc_t rp = make_rsrc(g.stats_part + (size_t)m0 * P * 2, (uint32_t)(rows * P * 8));
    for (int t = threadIdx.x; t < BM * QB; t += blockDim.x) {
      const int r = t % BM, q = t / BM;
      const float2 a = reinterpret_cast<const float2*>(pscr)[(2 * q) * BM + r];
      const float2 b = reinterpret_cast<const float2*>(pscr)[(2 * q + 1) * BM + r];
      const u32x2 v = {__float_as_uint(a.x + b.x), __float_as_uint(a.y + b.y)};
      const int part = (n0 >> 7) + q;
      __builtin_amdgcn_raw_buffer_store_b64(v, rp, part < P ? (r * P + part) * 8 : OOB, 0, 0);
    }
  }
}

// after a unit's epilogue: zero the accumulators for the next unit in one straight run, then retire the
// epilogue's VMEM ops with the BUILTIN wait (hipcc's waitcnt pass sees it; an asm one it does not):
// otherwise the pass carries the bias / residual load registers as possibly pending around the k-loop
// back edge and emits vmcnt(0) before the first ds_read of EVERY k-step -- draining the DMA ring each
// step (+25-40 % k-step cycles, measured by stamps vs the x2 arm)
template <int MT, int NTL>
MLS_DEV void ring_epilogue_done(f32x4 (&acc)[MT][NTL]) {
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int jn = 0; jn < NTL; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) expcnt(7) lgkmcnt(15)
}

// ------------------------------------------------------------------------------------ host side
// split-K of a launch: whole k-steps per split, the slabs fit the workspace, the tiles fit the counters
static inline bool ring_splitk_ok(int splitk, int nk, long long tiles, long long tile_elems, const void* ws,
                                  long long ws_elems, const void* cnt, int cnt_elems) {
  return ws && cnt && nk % splitk == 0 && tiles <= cnt_elems && tiles * splitk * tile_elems <= ws_elems;
}

// persistent grid: one resident wave of blocks (cap), each walking its units with the LDS-DMA ring
// running ahead across unit boundaries
static inline dim3 ring_grid(long long units, int cap) { return dim3((unsigned)(units < cap ? units : cap)); }
