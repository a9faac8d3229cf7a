// X4 tail on device: merge the tensor-parallel ranks' top-k candidates and pick each sequence's
// next token inside the captured decode step, so a TP decode loop never waits on the host.
//
// cand_v / cand_i: [tp][B][k] (the one-shot all-gather of every rank's local top-k; rank-major, so
// candidate j = r * k + c of row b is the host's `permute(1, 0, 2).reshape(B, -1)` order).
// Per row (params per row: top_k, temperature, seed):
//   greedy (top_k <= 1): the candidate at the FIRST maximum (torch.argmax order);
//   sampled: the top_k largest (ties -> lower j first, = a stable descending sort), p =
//   softmax(v / temperature), u = uniform(seed, step), the first i with cdf_i > u * cdf_last.
// uniform(seed, step) = (splitmix64(seed * 0x9E3779B97F4A7C15 + step) >> 40) * 2^-24: a counter-
// based draw the host reproduces bit-exactly (models/llama.py sample_uniform), independent of the
// row's position in the batch -- so a sequence's tokens do not depend on what else is in flight.
// Then the step's static inputs advance in place: tok[b] = token, pos[b] += 1, lens[b] += 1,
// hist[b][step[b]] = token, step[b] += 1 -- the next graph replay decodes the next position.
#include "pick_rule.h"

namespace {

__global__ __launch_bounds__(64) void decode_pick_kernel(const float* __restrict__ cv, const int* __restrict__ ci,
                                                         int tp, int B, int k, const int* __restrict__ topk,
                                                         const float* __restrict__ temp,
                                                         const long long* __restrict__ seed, int* tok, int* pos,
                                                         int* lens, int* hist, int hist_cols, int* step,
                                                         const int* __restrict__ rows,
                                                         const int* __restrict__ active, int* emit) {
  const int b = blockIdx.x, lane = threadIdx.x;
  // per-sequence state row of candidate row b: rows[b] (a prefill of new sequences into their
  // serving slots) or b; inactive state rows (an idle serving slot) are left untouched
  const int sr = rows ? rows[b] : b;
  if (active && !active[sr]) return;
  __shared__ PickLds L;
  // the pick rule (greedy / top-k sampled, the splitmix64 draw) is pick_rule.h's, shared with spec_step.hip
  const int token = pick_row(L, cv, ci, tp, B, k, b, topk ? topk[sr] : 1, temp ? temp[sr] : 1.f,
                             (unsigned long long)(seed ? seed[sr] : 0), (unsigned long long)step[sr], 401);
  if (lane == 0) {
    const int s = step[sr];
    if (hist && s < hist_cols) hist[(long)sr * hist_cols + s] = token;
    step[sr] = s + 1;
    tok[sr] = token;
    pos[sr] += 1;
    lens[sr] += 1;
    if (emit) emit[sr] = token;
  }
}

}  // namespace

MLS_DEBUG_EXPORT(decode_pick)

extern "C" {

// cv [tp][B][k] f32, ci [tp][B][k] i32; per-row params topk / temp / seed (nullptr: greedy, 1.0, 0);
// tok / pos / lens [B] i32 advanced in place; hist [B][hist_cols] (nullable); step [B] i32.
// Serving extensions (all nullable): rows [B] i32 maps candidate row b to state row rows[b] (the
// state arrays then have the serving batch's size, indices < state_rows); active [state rows] i32
// skips idle state rows; emit [state rows] i32 receives each picked token (a per-iteration
// read-back buffer next to the decode graph's own tok).
int mls_decode_pick(const float* cv, const int* ci, int tp, int B, int k, const int* topk, const float* temp,
                    const long long* seed, int* tok, int* pos, int* lens, int* hist, int hist_cols, int* step,
                    const int* rows, const int* active, int* emit, void* stream) {
  if (tp <= 0 || B <= 0 || k <= 0 || tp * k > PICK_MAX_CAND || !tok || !pos || !lens || !step) return MLS_BAD_ARG;
  hipLaunchKernelGGL(decode_pick_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, cv, ci, tp, B, k, topk, temp, seed,
                     tok, pos, lens, hist, hist_cols, step, rows, active, emit);
  return (int)hipGetLastError();
}

}  // extern "C"
