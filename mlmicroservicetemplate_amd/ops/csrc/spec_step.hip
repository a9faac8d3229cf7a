// Speculative decoding's two ends on device, so a verify step is one graph replay and one read-back:
//
//   spec_draft_kernel   prompt lookup over each decoding slot's own tokens -> the verify forward's
//                       static inputs (ids / n / past / lens), the rule of models/speculative.py
//                       spec_feed(tokens, K, remaining, prompt_lookup_draft(max_ngram, min_ngram));
//   spec_accept_kernel  the pick of each fed row (pick_rule.h, the rule of decode_pick.hip) and the
//                       longest prefix of drafts that equals the picks (speculative.accept), the
//                       slot's state advanced in place.
//
// Both are latency-bound (a few dozen rows of a few hundred bytes): one 64-lane wave per verify row.
// A sequence's tokens live in two arrays, prompt[s][0 .. plen[s]) then hist[s][0 .. step[s]), so that
// decode_pick's hist[row][step] write is the append.  Every data-dependent index (slot, token position,
// history column, candidate index) is clamped or skipped in the default build and reported through
// MLS_CHECK in the MLS_DEBUG build (codes 411-416).
#include "pick_rule.h"

namespace {

MLS_DEV int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int y = __shfl_xor(v, o, 64);
    v = y > v ? y : v;
  }
  return v;
}

// token i of a sequence of pl prompt tokens followed by history; i in [0, pl + st), pl, st <= cols
struct SeqTokens {
  const int* p;
  const int* h;
  int pl;
  MLS_DEV int operator[](int i) const { return i < pl ? p[i] : h[i - pl]; }
};

__global__ __launch_bounds__(64) void spec_draft_kernel(const int* __restrict__ rows, int nslots,
                                                        const int* __restrict__ prompt,
                                                        const int* __restrict__ plen, const int* __restrict__ hist,
                                                        const int* __restrict__ step,
                                                        const int* __restrict__ max_new,
                                                        const int* __restrict__ pos, int cols, int K, int T,
                                                        int max_ngram, int min_ngram, int* __restrict__ ids,
                                                        int* __restrict__ n_out, int* __restrict__ past_out,
                                                        int* __restrict__ lens_out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  int* out = ids + (long)r * T;
  const int s = rows[r];
  const bool slot_ok = s >= 0 && s < nslots;
  MLS_CHECK(slot_ok, 411);
  int pl = 0, st = 0, remaining = 0, past = 0;
  if (slot_ok) {
    pl = plen[s], st = step[s], past = pos[s];
    remaining = max_new[s] - st;
    const bool ok = pl >= 0 && st >= 0 && pl <= cols && st <= cols && pl + st >= 1;
    MLS_CHECK(ok, 412);  // token counts outside the prompt / history arrays (or an empty sequence)
    if (!ok) remaining = 0;
  }
  int Kp = remaining - 1 < K ? remaining - 1 : K;
  Kp = Kp < 0 ? 0 : (Kp > T - 1 ? T - 1 : Kp);
  int n = remaining <= 0 ? 0 : 1 + Kp;
  const bool pos_ok = past >= 0 && past + n <= cols;
  MLS_CHECK(pos_ok, 413);  // the fed positions would leave the slot's rows
  if (!pos_ok) past = 0, n = 0;
  if (lane == 0) {
    n_out[r] = n;
    past_out[r] = past;
    lens_out[r] = past + n;
  }
  if (n == 0) {
    for (int t = lane; t < T; t += 64) out[t] = 0;
    return;
  }
  const SeqTokens tk{prompt + (long)s * cols, hist + (long)s * cols, pl};
  const int L = pl + st;
  const int last = tk[L - 1];
  // the longest n-gram first; lanes stride over the candidate starts i <= L - g - 1, the most recent wins
  int best = -1, g = max_ngram < L - 1 ? max_ngram : L - 1;
  const int gmin = min_ngram > 1 ? min_ngram : 1;
  for (; Kp > 0 && g >= gmin; --g) {
    int mine = -1;
    for (int i = lane; i <= L - g - 1; i += 64) {
      bool eq = tk[i + g - 1] == last;  // most candidates fail on their last token: one load each
      for (int j = 0; eq && j < g - 1; ++j) eq = tk[i + j] == tk[L - g + j];
      if (eq) mine = i;  // i ascends: the lane keeps its most recent match
    }
    best = wave_max_i(mine);
    if (best >= 0) break;
  }
  // drafts = tokens[best + g : best + g + Kp], padded with their last element (no match: the last token)
  const int from = best >= 0 ? best + g : L;
  const int have = best >= 0 ? (L - from < Kp ? L - from : Kp) : 0;
  const int pad = have > 0 ? tk[from + have - 1] : last;
  for (int t = lane; t < T; t += 64) out[t] = t == 0 ? last : (t - 1 < have ? tk[from + t - 1] : (t < n ? pad : 0));
}

__global__ __launch_bounds__(64) void spec_accept_kernel(const float* __restrict__ cv, const int* __restrict__ ci,
                                                         int tp, int Bv, int T, int k, const int* __restrict__ ids,
                                                         const int* __restrict__ n_in, const int* __restrict__ rows,
                                                         int nslots, const int* __restrict__ topk,
                                                         const float* __restrict__ temp,
                                                         const long long* __restrict__ seed, int* tok, int* pos,
                                                         int* lens, int* step, int* hist, int cols,
                                                         const int* __restrict__ eos, int n_eos, int* rb) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int s = rows[r];
  const bool slot_ok = s >= 0 && s < nslots;
  MLS_CHECK(slot_ok, 414);
  if (!slot_ok) return;
  int n = n_in[r];
  MLS_CHECK(n >= 0 && n <= T, 415);
  n = n < 0 ? 0 : (n > T ? T : n);
  int* blk = rb + (long)s * (T + 2);  // the slot's read-back block: n fed, got, the got tokens
  if (n == 0) {
    if (lane == 0) blk[0] = 0, blk[1] = 0;
    return;
  }
  __shared__ PickLds L;
  const int s0 = step[s];
  const int want = topk ? topk[s] : 1;
  const float t_ = temp ? temp[s] : 1.f;
  const unsigned long long sd = (unsigned long long)(seed ? seed[s] : 0);
  int got = 0, y = 0;
  // rows t >= n are padding: never read.  Every lane holds the same y, so the loop's exit is uniform.
  for (int t = 0; t < n; ++t) {
    y = pick_row(L, cv, ci, tp, Bv * T, k, r * T + t, want, t_, sd, (unsigned long long)(s0 + t), 416);
    got = t + 1;
    if (lane == 0) {
      blk[2 + t] = y;
      const bool col_ok = s0 + t >= 0 && s0 + t < cols;
      MLS_CHECK(col_ok, 412);
      if (col_ok) hist[(long)s * cols + s0 + t] = y;
    }
    bool stop = t + 1 >= n || ids[(long)r * T + t + 1] != y;
    for (int e = 0; e < n_eos; ++e) stop |= eos[e] == y;
    if (stop) break;
  }
  if (lane == 0) {
    blk[0] = n;
    blk[1] = got;
    step[s] = s0 + got;
    tok[s] = y;
    const int p = pos[s] + got;
    pos[s] = p;
    lens[s] = p + 1;
  }
}

}  // namespace

MLS_DEBUG_EXPORT(spec_step)

extern "C" {

// Per verify row r (slot s = rows[r] < nslots): ids [Bv][T] (the feed, zero-padded), n / past / lens [Bv].
// prompt / hist [nslots][cols] i32, plen / step / max_new / pos [nslots] i32.  A row whose slot may emit
// nothing more (max_new[s] - step[s] <= 0) feeds n = 0.
int mls_spec_draft(const int* rows, int Bv, int nslots, const int* prompt, const int* plen, const int* hist,
                   const int* step, const int* max_new, const int* pos, int cols, int K, int T, int max_ngram,
                   int min_ngram, int* ids, int* n, int* past, int* lens, void* stream) {
  if (Bv <= 0 || nslots <= 0 || cols <= 0 || K < 0 || T < K + 1 || max_ngram < 1 || !rows || !prompt || !plen ||
      !hist || !step || !max_new || !pos || !ids || !n || !past || !lens)
    return MLS_BAD_ARG;
  hipLaunchKernelGGL(spec_draft_kernel, dim3(Bv), dim3(64), 0, (hipStream_t)stream, rows, nslots, prompt, plen, hist,
                     step, max_new, pos, cols, K, T, max_ngram, min_ngram, ids, n, past, lens);
  return (int)hipGetLastError();
}

// cv / ci [tp][Bv * T][k] (decode_pick's layout), ids [Bv][T] / n [Bv] the feed, rows [Bv]; per-slot topk /
// temp / seed (nullptr: greedy, 1.0, 0); tok / pos / lens / step [nslots] and hist [nslots][cols] advanced in
// place; eos [n_eos] i32 (nullable with n_eos = 0); rb [nslots][T + 2] i32 the per-slot read-back block.
int mls_spec_accept(const float* cv, const int* ci, int tp, int Bv, int T, int k, const int* ids, const int* n,
                    const int* rows, int nslots, const int* topk, const float* temp, const long long* seed, int* tok,
                    int* pos, int* lens, int* step, int* hist, int cols, const int* eos, int n_eos, int* rb,
                    void* stream) {
  if (tp <= 0 || Bv <= 0 || T <= 0 || k <= 0 || tp * k > PICK_MAX_CAND || nslots <= 0 || cols <= 0 || n_eos < 0 ||
      (n_eos > 0 && !eos) || !cv || !ci || !ids || !n || !rows || !tok || !pos || !lens || !step || !hist || !rb)
    return MLS_BAD_ARG;
  hipLaunchKernelGGL(spec_accept_kernel, dim3(Bv), dim3(64), 0, (hipStream_t)stream, cv, ci, tp, Bv, T, k, ids, n, rows,
                     nslots, topk, temp, seed, tok, pos, lens, step, hist, cols, eos, n_eos, rb);
  return (int)hipGetLastError();
}

}  // extern "C"
