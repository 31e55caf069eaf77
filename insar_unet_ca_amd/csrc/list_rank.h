// What outline.hip and contour.hip share: the ranking of a successor array by pointer doubling, one round per launch, on pairs
// packed as int2 so that the gather of a round is one 8-byte access. A round moves 24 bytes per element: 8 read in index order, 8
// gathered, 8 written. The kernels are templates on the work-group size: the header is included by more than one file of a
// library linked without relocatable device code.
// The pair buffers p[0] and p[1] ping-pong: a helper runs list_rounds(n) rounds, round r reads p[(from + r) & 1] and writes the
// other, so what it computes ends in p[(from + list_rounds(n)) & 1]. With a `cut` launch between them that reads the result of
// `lead` and writes the other buffer, lead from p[0] and rank from where `cut` wrote end in p[1] whatever n is, and p[0] is free.
#pragma once
#include "scene_common.h"

// pairs (jump, min): (j, m)[k] <- (j[j[k]], min(m[k], m[j[k]])). After list_rounds(n) rounds m[k] is the smallest m of k's ring;
// an element of a list that ends in a fixed point (jump == itself) has jumped there.
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
list_lead_round_kernel(const int2* __restrict__ in, int2* __restrict__ out, int n) {
  const int k = blockIdx.x * THREADS + threadIdx.x;
  if (k >= n) return;
  const int2 a = in[k];
  const int2 b = in[a.x];
  out[k] = make_int2(b.x, min(a.y, b.y));
}

// Wyllie list ranking on pairs (next, d), next < 0 at the end of a list: afterwards d[k] is the sum of d from k to the end.
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
list_rank_round_kernel(const int2* __restrict__ in, int2* __restrict__ out, int n) {
  const int k = blockIdx.x * THREADS + threadIdx.x;
  if (k >= n) return;
  int2 a = in[k];
  if (a.x >= 0) {
    const int2 b = in[a.x];
    a = make_int2(b.x, a.y + b.y);
  }
  out[k] = a;
}

static inline int list_rounds(int n) {                           // ceil(log2 n)
  int r = 0;
  while (((int64_t)1 << r) < n) ++r;
  return r;
}

typedef void (*ListRoundKernel)(const int2*, int2*, int);
static inline int list_run_rounds(ListRoundKernel round, int threads, int2* const p[2], int from, int n, hipStream_t s, const char* who) {
  const int rounds = list_rounds(n);
  for (int r = 0, cur = from & 1; r < rounds; ++r, cur ^= 1) {
    hipLaunchKernelGGL(round, dim3(scene_blocks(n, threads)), dim3(threads), 0, s, (const int2*)p[cur], p[cur ^ 1], n);
    INSAR_CHECK_LAUNCH(who);
  }
  return INSAR_OK;
}
template <int THREADS>
static inline int list_lead(int2* const p[2], int from, int n, hipStream_t s, const char* who) {
  return list_run_rounds(list_lead_round_kernel<THREADS>, THREADS, p, from, n, s, who);
}
template <int THREADS>
static inline int list_rank(int2* const p[2], int from, int n, hipStream_t s, const char* who) {
  return list_run_rounds(list_rank_round_kernel<THREADS>, THREADS, p, from, n, s, who);
}
