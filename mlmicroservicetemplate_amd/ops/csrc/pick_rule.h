// The next-token rule of one candidate row, shared by decode_pick.hip (one token per sequence and
// step) and spec_step.hip (the K + 1 rows of a verify step): one copy, so the two cannot drift.
//
// cand_v / cand_i: [tp][B][k] (the one-shot all-gather of every rank's local top-k; rank-major, so
// candidate j = r * k + c of row b is the host's `permute(1, 0, 2).reshape(B, -1)` order).
//   greedy (top_k <= 1): the candidate at the FIRST maximum (torch.argmax order);
//   sampled: the top_k largest (ties -> lower j first, = a stable descending sort), p =
//   softmax(v / temperature), u = uniform(seed, step), the first i with cdf_i > u * cdf_last.
// uniform(seed, step) = (splitmix64(seed * 0x9E3779B97F4A7C15 + step) >> 40) * 2^-24: a counter-
// based draw the host reproduces bit-exactly (models/llama.py sample_uniform / pick_token).
#pragma once
#include "common.h"

constexpr int PICK_MAX_CAND = 512;  // tp * k
constexpr int PICK_MAX_TOPK = 64;

MLS_DEV unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct VI {
  float v;
  int j;
};
// larger value first; ties: lower candidate index first
MLS_DEV bool vi_better(VI a, VI b) { return a.v > b.v || (a.v == b.v && a.j < b.j); }

MLS_DEV VI wave_best(VI x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    VI y{__shfl_xor(x.v, o, 64), __shfl_xor(x.j, o, 64)};
    if (vi_better(y, x)) x = y;
  }
  return x;
}

// LDS of one pick (one 64-lane block per row)
struct PickLds {
  float sv[PICK_MAX_CAND];
  int sj[PICK_MAX_CAND];
  float tv[PICK_MAX_TOPK];
  int tj[PICK_MAX_TOPK];
};

// Token of candidate row b (of B) under (want = top_k, temperature t, seed, step).  Called by all 64
// lanes of a one-wave block with uniform arguments; every lane gets the token.  n = tp * k <=
// PICK_MAX_CAND (the launchers check).  `oob` is the MLS_CHECK code of a winner index outside [0, n)
// (all candidates NaN): the default build falls back to candidate 0.
MLS_DEV int pick_row(PickLds& L, const float* __restrict__ cv, const int* __restrict__ ci, int tp, int B, int k, int b,
                     int want, float t, unsigned long long seed, unsigned long long step, int oob) {
  const int lane = threadIdx.x;
  const int n = tp * k;
  __syncthreads();  // an earlier pick of this block is done with the LDS
  for (int j = lane; j < n; j += 64) {
    const int r = j / k, c = j - r * k;
    L.sv[j] = cv[((long)r * B + b) * k + c];
    L.sj[j] = ci[((long)r * B + b) * k + c];
  }
  __syncthreads();
  if (want <= 1) {
    VI best{-INFINITY, 0x7fffffff};
    for (int j = lane; j < n; j += 64) best = vi_better(VI{L.sv[j], j}, best) ? VI{L.sv[j], j} : best;
    best = wave_best(best);
    MLS_CHECK(best.j >= 0 && best.j < n, oob);
    return L.sj[best.j >= 0 && best.j < n ? best.j : 0];
  }
  const int kk = want < n ? (want < PICK_MAX_TOPK ? want : PICK_MAX_TOPK) : (n < PICK_MAX_TOPK ? n : PICK_MAX_TOPK);
  for (int s = 0; s < kk; ++s) {  // kk rounds of wave argmax, each removes its winner
    VI best{-INFINITY, 0x7fffffff};
    for (int j = lane; j < n; j += 64)
      if (L.sj[j] >= 0 || L.sv[j] > -INFINITY) best = vi_better(VI{L.sv[j], j}, best) ? VI{L.sv[j], j} : best;
    best = wave_best(best);
    if (lane == 0) {
      L.tv[s] = best.v;
      L.tj[s] = best.j;
      if (best.j >= 0 && best.j < n) L.sv[best.j] = -INFINITY, L.sj[best.j] = -1;
    }
    __syncthreads();
  }
  if (lane == 0) {
    const float tt = fmaxf(t, 1e-5f);
    const float mx = L.tv[0];
    float p[PICK_MAX_TOPK];
    float cdf = 0.f;
    for (int s = 0; s < kk; ++s) {
      p[s] = expf((L.tv[s] - mx) / tt);
      cdf += p[s];
      p[s] = cdf;  // running sum (same order as the host's cumsum)
    }
    const unsigned long long h = splitmix64(seed * 0x9E3779B97F4A7C15ull + step);
    const float u = (float)(h >> 40) * (1.f / 16777216.f);
    int pick = kk - 1;
    for (int s = 0; s < kk; ++s)
      if (p[s] > u * cdf) {
        pick = s;
        break;
      }
    int jj = L.tj[pick];
    MLS_CHECK(jj >= 0 && jj < n, oob);
    jj = jj >= 0 && jj < n ? jj : 0;
    // the winners' ids were cleared in sj: re-read the candidate id from global memory
    const int r = jj / k, c = jj - r * k;
    L.sj[0] = ci[((long)r * B + b) * k + c];
  }
  __syncthreads();
  return L.sj[0];
}
