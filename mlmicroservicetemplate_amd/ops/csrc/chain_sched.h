// Tile schedule of the persistent conv_chain form (conv_chain.hip): which row tiles block `bid` of a
// `G`-block grid takes.  No block depends on another: the schedule is a pure function of (bid, G),
// so a grid larger than the tile count, or one whose blocks queue behind a CU mask, only leaves some
// blocks with fewer (or no) tiles.
//
// Block bid's logical index v is common.h's xcd_remap(bid, G) (hardware block ids b, b + 8, ... share
// an XCD; each XCD gets a contiguous range of logical indices); it takes tiles v, v + G, v + 2G, ...
// In every pass of G tiles an XCD therefore streams one contiguous range of rows.
//
// Plain C++ on purpose: tests/native/chain_sched_check.cpp compiles this header with the host
// compiler and checks that every tile is taken exactly once (tests/test_chain_sched.py).
#pragma once

#if defined(__HIP__)
#define MLS_SCHED_FN __host__ __device__ inline
#else
#define MLS_SCHED_FN inline
#endif

// the body of common.h xcd_remap: a bijection on [0, G) for every G >= 1
MLS_SCHED_FN int chain_logical_block(int bid, int G) {
  if (G <= 8) return bid;
  const int q = G >> 3, r = G & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// first tile of block bid (>= ntiles: the block has none) and the tile after `tile`
MLS_SCHED_FN int chain_first_tile(int bid, int G) { return chain_logical_block(bid, G); }
MLS_SCHED_FN int chain_next_tile(int tile, int G) { return tile + G; }
