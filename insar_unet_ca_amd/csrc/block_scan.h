// What the two Douglas-Peucker files (simplify.hip, contour_simplify.hip) share: the scans of one value per thread over a
// work-group of BLOCK_SCAN_THREADS threads, by wave shuffles and one LDS slot per wave. Every thread of the work-group calls
// them (they synchronise); w is BLOCK_SCAN_WAVES ints of LDS, free again on return.
#pragma once
#include "scene_common.h"
#include <limits.h>

#define BLOCK_SCAN_THREADS 256
#define BLOCK_SCAN_WAVES (BLOCK_SCAN_THREADS / INSAR_WAVE)

// inclusive maximum over the threads 0 .. tid of the work-group, and the work-group's maximum
__device__ __forceinline__ int block_prefix_max(int v, int* w, int* total) {
  const int lane = threadIdx.x & (INSAR_WAVE - 1), wave = threadIdx.x / INSAR_WAVE;
#pragma unroll
  for (int d = 1; d < INSAR_WAVE; d <<= 1) {
    const int o = __shfl_up(v, d, INSAR_WAVE);
    if (lane >= d) v = o > v ? o : v;
  }
  if (lane == INSAR_WAVE - 1) w[wave] = v;
  __syncthreads();
  int tot = INT_MIN;
#pragma unroll
  for (int k = 0; k < BLOCK_SCAN_WAVES; ++k) {
    if (k < wave) v = w[k] > v ? w[k] : v;
    tot = w[k] > tot ? w[k] : tot;
  }
  *total = tot;
  __syncthreads();
  return v;
}
// inclusive minimum over the threads tid .. BLOCK_SCAN_THREADS - 1
__device__ __forceinline__ int block_suffix_min(int v, int* w, int* total) {
  const int lane = threadIdx.x & (INSAR_WAVE - 1), wave = threadIdx.x / INSAR_WAVE;
#pragma unroll
  for (int d = 1; d < INSAR_WAVE; d <<= 1) {
    const int o = __shfl_down(v, d, INSAR_WAVE);
    if (lane + d < INSAR_WAVE) v = o < v ? o : v;
  }
  if (lane == 0) w[wave] = v;
  __syncthreads();
  int tot = INT_MAX;
#pragma unroll
  for (int k = 0; k < BLOCK_SCAN_WAVES; ++k) {
    if (k > wave) v = w[k] < v ? w[k] : v;
    tot = w[k] < tot ? w[k] : tot;
  }
  *total = tot;
  __syncthreads();
  return v;
}
// exclusive prefix sum over the work-group's threads
__device__ __forceinline__ int block_prefix_sum(int v, int* w, int* total) {
  const int lane = threadIdx.x & (INSAR_WAVE - 1), wave = threadIdx.x / INSAR_WAVE;
  const int incl = wave_incl_scan(v, lane);
  if (lane == INSAR_WAVE - 1) w[wave] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < BLOCK_SCAN_WAVES; ++k) {
    if (k < wave) off += w[k];
    tot += w[k];
  }
  *total = tot;
  __syncthreads();
  return off + incl - v;
}

// One work-group: cmax[j] = max of bmax over the blocks before j, cmin[j] = min of bmin over the blocks after j (the last kept
// position before a block of positions and the first after it, -1 / INT_MAX where there is none).
__device__ __forceinline__ void block_carry(const int* bmax, const int* bmin, int* cmax, int* cmin, int nblk, int* w) {
  int carry = -1, total;
  for (int base = 0; base < nblk; base += BLOCK_SCAN_THREADS) {  // every thread keeps the same running maximum
    const int j = base + (int)threadIdx.x;
    const int v = (j >= 1 && j <= nblk) ? bmax[j - 1] : -1;
    const int m = block_prefix_max(v, w, &total);
    if (j < nblk) cmax[j] = m > carry ? m : carry;
    carry = total > carry ? total : carry;
  }
  carry = INT_MAX;
  for (int base = ((nblk - 1) / BLOCK_SCAN_THREADS) * BLOCK_SCAN_THREADS; base >= 0; base -= BLOCK_SCAN_THREADS) {
    const int j = base + (int)threadIdx.x;
    const int v = j + 1 < nblk ? bmin[j + 1] : INT_MAX;
    const int m = block_suffix_min(v, w, &total);
    if (j < nblk) cmin[j] = m < carry ? m : carry;
    carry = total < carry ? total : carry;
  }
}
