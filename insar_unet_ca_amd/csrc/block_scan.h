// The work-group scans of the scene tools (regions.hip, split.hip, raster.hip, outline.hip, contour.hip, hysteresis.hip, and
// dp_common.h for simplify.hip and contour_simplify.hip): one value per thread over a work-group of THREADS threads, by wave shuffles and one LDS
// slot per wave, and the one-work-group scan of a whole array built on the same steps. Every thread of the work-group calls them
// (they synchronise); w is THREADS / INSAR_WAVE ints of LDS, free again on return.
#pragma once
#include "scene_common.h"
#include <limits.h>

// inclusive maximum over the threads 0 .. tid of the work-group, and the work-group's maximum
template <int THREADS>
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
  for (int k = 0; k < THREADS / INSAR_WAVE; ++k) {
    if (k < wave) v = w[k] > v ? w[k] : v;
    tot = w[k] > tot ? w[k] : tot;
  }
  *total = tot;
  __syncthreads();
  return v;
}
// inclusive minimum over the threads tid .. THREADS - 1
template <int THREADS>
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
  for (int k = 0; k < THREADS / INSAR_WAVE; ++k) {
    if (k > wave) v = w[k] < v ? w[k] : v;
    tot = w[k] < tot ? w[k] : tot;
  }
  *total = tot;
  __syncthreads();
  return v;
}
// exclusive prefix sum over the work-group's threads; *total is the work-group's sum
template <int THREADS>
__device__ __forceinline__ int block_prefix_sum(int v, int* w, int* total) {
  const int lane = threadIdx.x & (INSAR_WAVE - 1), wave = threadIdx.x / INSAR_WAVE;
  const int incl = wave_incl_scan(v, lane);
  if (lane == INSAR_WAVE - 1) w[wave] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < THREADS / INSAR_WAVE; ++k) {
    if (k < wave) off += w[k];
    tot += w[k];
  }
  *total = tot;
  __syncthreads();
  return off + incl - v;
}

// One work-group: a[0 .. n) becomes its exclusive prefix sum in place, THREADS elements per pass; returns the total (< 2^31) to
// every thread. On return the new a[] is visible to the whole work-group. The caller writes its own header from the total.
template <int THREADS>
__device__ __forceinline__ int block_scan_array(int* a, int n, int* w) {
  const int lane = threadIdx.x & (INSAR_WAVE - 1), wave = threadIdx.x / INSAR_WAVE;
  int carry = 0;                                                 // every thread keeps the same running total
  for (int base = 0; base < n; base += THREADS) {
    const int i = base + (int)threadIdx.x;
    const int v = i < n ? a[i] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (lane == INSAR_WAVE - 1) w[wave] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < THREADS / INSAR_WAVE; ++k) {
      if (k < wave) off += w[k];
      tot += w[k];
    }
    if (i < n) a[i] = carry + off + incl - v;
    carry += tot;
    __syncthreads();
  }
  return carry;
}

// One work-group: cmax[j] = max of bmax over the blocks before j, cmin[j] = min of bmin over the blocks after j (the last kept
// position before a block of positions and the first after it, -1 / INT_MAX where there is none).
template <int THREADS>
__device__ __forceinline__ void block_carry(const int* bmax, const int* bmin, int* cmax, int* cmin, int nblk, int* w) {
  int carry = -1, total;
  for (int base = 0; base < nblk; base += THREADS) {             // every thread keeps the same running maximum
    const int j = base + (int)threadIdx.x;
    const int v = (j >= 1 && j <= nblk) ? bmax[j - 1] : -1;
    const int m = block_prefix_max<THREADS>(v, w, &total);
    if (j < nblk) cmax[j] = m > carry ? m : carry;
    carry = total > carry ? total : carry;
  }
  carry = INT_MAX;
  for (int base = ((nblk - 1) / THREADS) * THREADS; base >= 0; base -= THREADS) {
    const int j = base + (int)threadIdx.x;
    const int v = j + 1 < nblk ? bmin[j + 1] : INT_MAX;
    const int m = block_suffix_min<THREADS>(v, w, &total);
    if (j < nblk) cmin[j] = m < carry ? m : carry;
    carry = total < carry ? total : carry;
  }
}
