// Exact Euclidean distance transform of a class or label map [B][H][W] (uint8 or int32), with the nearest site, and the
// boundary-band counts built on it. Integers only: squared distances are exact in int32 (H, W <= 32767, so d2 <= 2 * 32766^2
// < 2^31 - 1 = INSAR_DIST_FAR), no float anywhere, no atomics in the transform. Two launches per transform:
//
//   columns  one thread per (column, band of 32 rows). The sites of the band go into a 32-bit mask (32 loads, coalesced over
//            the columns of a work-group); the nearest site above / below a row INSIDE the band is then a clz / ctz on the
//            mask, and the carry from outside the band is a look-back over the map itself: up from the band's first row (and
//            down from its last) until a site is met, the image ends, or max_distance rows have gone by. The look-back is
//            skipped when the band's first (last) row is itself a site. Output: int16 sy [B][H][W], the row of the nearest site
//            of the pixel's column (a tie goes to the upper one), -1 if the column has none in reach.
//   rows     one thread per pixel p = (y, x): d2 = min over x' of (y - sy[y][x'])^2 + (x - x')^2, scanned outwards k = 0, 1, 2,
//            ... over x - k and x + k, until k passes max_distance, both ends of the row are passed, or k^2 > best. The exit is
//            strict: a candidate at k^2 == best (its column holds a site in the pixel's own row) ties and may carry the smaller
//            index. For a fixed k the lanes of a wave read consecutive int16 of sy: 128 contiguous bytes, served by L1 / L2;
//            neighbouring pixels have distances within 1 of each other, so a wave leaves the loop together. FAR is never added
//            to: a column without a site is skipped by a compare.
//
// Tie rule: of several nearest sites the one with the smallest linear index y * W + x wins. In one column the candidates at
// the least distance are the nearest above and the nearest below; the upper one has the smaller index, so `columns` keeps it;
// `rows` compares indices whenever two columns give the same d2.
//
// Boundary counts (a clear and one more launch): per class c the pixels of P_c & G_c, P_c, G_c outside the void map, where
// P_c = {pred == c, d2_pred <= r2} and G_c = {gt == c, d2_gt <= r2}. Per thread 3 K int32 counters in registers, summed over
// the wave with shuffles, over the work-group in LDS, then 3 K agent-scope int64 atomic adds per work-group (the pattern of
// overlap.hip): integer sums, independent of the launch geometry.
#include "scene_common.h"
#include <limits.h>

#define DT_THREADS 256
#define DT_BAND 32
#define DT_MAX_DIM 32767
#define DT_MAX_K 8
// R >= 46340 caps nothing: the largest d2 of the contract is 2 * 32766^2 = 2147221512 <= 46340^2; below that R^2 fits int32
#define DT_MAX_R 46339

static_assert(INSAR_DIST_FAR == INT_MAX, "FAR is the largest int32");
static_assert(2ll * (DT_MAX_DIM - 1) * (DT_MAX_DIM - 1) < (long long)INSAR_DIST_FAR, "every d2 of the contract is below FAR");

// ---- site predicates ------------------------------------------------------------------------------------------------------
// img: element (0, 0) of one image. EDGE: v is the ignored value (< 0: none); a pixel is a site if it is not ignored and one
// of its 4-neighbours inside the image is neither ignored nor of its value.
template <typename T, int MODE>
__device__ __forceinline__ bool dt_site(const T* __restrict__ img, int H, int W, int y, int x, int v) {
  const int64_t p = (int64_t)y * W + x;
  const int c = (int)img[p];
  if (MODE == INSAR_DIST_EQ) return c == v;
  if (MODE == INSAR_DIST_NE) return c != v;
  const bool ign = v >= 0;
  if (ign && c == v) return false;
  bool e = false;
  if (y > 0) { const int q = (int)img[p - W]; e |= q != c && !(ign && q == v); }
  if (y + 1 < H) { const int q = (int)img[p + W]; e |= q != c && !(ign && q == v); }
  if (x > 0) { const int q = (int)img[p - 1]; e |= q != c && !(ign && q == v); }
  if (x + 1 < W) { const int q = (int)img[p + 1]; e |= q != c && !(ign && q == v); }
  return e;
}

// ---- columns ----------------------------------------------------------------------------------------------------------------
// items = B * nbands * wblocks work items of 256 columns x 32 rows; R = 0: unbounded
template <typename T, int MODE>
__global__ void __launch_bounds__(DT_THREADS)
dist_columns_kernel(const T* __restrict__ m, int H, int W, int v, int R, int16_t* __restrict__ sy, int64_t items, int nbands,
                    int wblocks) {
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int wb = (int)(item % wblocks);
    const int64_t t = item / wblocks;
    const int band = (int)(t % nbands);
    const int64_t b = t / nbands;
    const int x = wb * DT_THREADS + (int)threadIdx.x;
    if (x >= W) continue;                                            // no barrier in this kernel
    const T* img = m + b * (int64_t)H * W;
    int16_t* out = sy + b * (int64_t)H * W;
    const int y0 = band * DT_BAND, y1 = min(H, y0 + DT_BAND), n = y1 - y0;
    uint32_t mask = 0u;
    for (int r = 0; r < n; ++r)
      if (dt_site<T, MODE>(img, H, W, y0 + r, x, v)) mask |= 1u << r;
    int up = -1, dn = -1;                                            // the nearest site above the band / below it
    if (!(mask & 1u)) {
      const int lo = R > 0 ? max(0, y0 - R) : 0;
      for (int y = y0 - 1; y >= lo; --y)
        if (dt_site<T, MODE>(img, H, W, y, x, v)) { up = y; break; }
    }
    if (!((mask >> (n - 1)) & 1u)) {
      const int hi = R > 0 ? min(H, y1 + R) : H;
      for (int y = y1; y < hi; ++y)
        if (dt_site<T, MODE>(img, H, W, y, x, v)) { dn = y; break; }
    }
    for (int r = 0; r < n; ++r) {
      const int y = y0 + r;
      const uint32_t at_or_above = mask & (0xffffffffu >> (31 - r));          // bits 0..r
      const uint32_t at_or_below = mask & (0xffffffffu << r);                 // bits r..31
      const int u = at_or_above ? y0 + 31 - __clz((int)at_or_above) : up;
      const int d = at_or_below ? y0 + __ffs((int)at_or_below) - 1 : dn;
      int s;
      if (u < 0) s = d;
      else if (d < 0) s = u;
      else s = (y - u <= d - y) ? u : d;                                      // a tie goes to the upper site
      out[(int64_t)y * W + x] = (int16_t)s;
    }
  }
}

// ---- rows -------------------------------------------------------------------------------------------------------------------
template <bool NEAR>
__global__ void __launch_bounds__(DT_THREADS)
dist_rows_kernel(const int16_t* __restrict__ sy, int H, int W, int R, int64_t npix, int32_t* __restrict__ d2,
                 int32_t* __restrict__ nearest) {
  const int r2 = R > 0 ? R * R : INSAR_DIST_FAR;
  for (int64_t p = blockIdx.x * (int64_t)DT_THREADS + threadIdx.x; p < npix; p += (int64_t)gridDim.x * DT_THREADS) {
    const int x = (int)(p % W);
    const int y = (int)((p / W) % H);
    const int16_t* row = sy + (p - x);
    int best = INSAR_DIST_FAR, bidx = -1;
    {
      const int s = row[x];
      if (s >= 0) { best = (y - s) * (y - s); bidx = s * W + x; }
    }
    int kmax = max(x, W - 1 - x);
    if (R > 0) kmax = min(kmax, R);
    for (int k = 1; k <= kmax; ++k) {
      const int kk = k * k;
      if (kk > best) break;                                          // strict: k^2 == best may still tie with a smaller index
      if (k <= x) {
        const int s = row[x - k];
        if (s >= 0) {
          const int d = (y - s) * (y - s) + kk, idx = s * W + x - k;
          if (d < best || (NEAR && d == best && idx < bidx)) { best = d; bidx = idx; }
        }
      }
      if (x + k < W) {
        const int s = row[x + k];
        if (s >= 0) {
          const int d = (y - s) * (y - s) + kk, idx = s * W + x + k;
          if (d < best || (NEAR && d == best && idx < bidx)) { best = d; bidx = idx; }
        }
      }
    }
    if (best > r2) { best = INSAR_DIST_FAR; bidx = -1; }
    d2[p] = best;
    if (NEAR) nearest[p] = bidx;
  }
}

// ---- boundary-band counts -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT_THREADS)
dist_counts_clear_kernel(long long* __restrict__ counts, int n) {
  if ((int)threadIdx.x < n) counts[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(DT_THREADS)
dist_counts_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, const int* __restrict__ d2p,
                   const int* __restrict__ d2g, int64_t npix, int vec, int r2, int K, int void_value, long long* counts) {
  __shared__ int part[DT_THREADS / INSAR_WAVE][3 * DT_MAX_K];
  int cnt[3 * DT_MAX_K];
#pragma unroll
  for (int i = 0; i < 3 * DT_MAX_K; ++i) cnt[i] = 0;
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q = blockIdx.x * (int64_t)DT_THREADS + threadIdx.x; q < nquads; q += (int64_t)gridDim.x * DT_THREADS) {
    int p[4], g[4], dp[4], dg[4];
    quad_load_u8(pred, q << 2, npix, vec, 0, p);
    quad_load_u8(gt, q << 2, npix, vec, void_value, g);              // past the end: void, dropped
    quad_load(d2p, q << 2, npix, vec, INSAR_DIST_FAR, dp);
    quad_load(d2g, q << 2, npix, vec, INSAR_DIST_FAR, dg);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (g[j] == void_value) continue;
      const bool inP = dp[j] <= r2, inG = dg[j] <= r2;
#pragma unroll
      for (int c = 0; c < DT_MAX_K; ++c) {                           // classes >= K are in no set
        const bool pc = inP && p[j] == c && c < K, gc = inG && g[j] == c && c < K;
        cnt[3 * c + 0] += pc && gc;
        cnt[3 * c + 1] += pc;
        cnt[3 * c + 2] += gc;
      }
    }
  }
  const int lane = (int)__lane_id(), wave = threadIdx.x / INSAR_WAVE;
#pragma unroll
  for (int i = 0; i < 3 * DT_MAX_K; ++i) {
    int v = cnt[i];          // written out: through a shared wave_sum(int) the compiler allocates 60 VGPRs here instead of 52
#pragma unroll
    for (int o = INSAR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, INSAR_WAVE);
    if (lane == 0) part[wave][i] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < 3 * K) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < DT_THREADS / INSAR_WAVE; ++w) s += part[w][threadIdx.x];
    if (s) __hip_atomic_fetch_add(&counts[threadIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int dist_check_shape(const char* who, int32_t B, int32_t H, int32_t W, int64_t* npix) {
  if (B < 1 || H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty map %d x %d x %d", who, B, H, W);
  if (H > DT_MAX_DIM || W > DT_MAX_DIM) INSAR_FAIL(INSAR_E_SHAPE, "%s: map %d x %d: H and W at most %d", who, H, W, DT_MAX_DIM);
  const int64_t n = (int64_t)B * H * W;
  if (n >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: map %d x %d x %d has 2^31 pixels or more", who, B, H, W);
  *npix = n;
  return INSAR_OK;
}

extern "C" int insar_dist_scratch_bytes(int32_t B, int32_t H, int32_t W, int64_t* scratch_bytes) {
  const char* who = "insar_dist_scratch_bytes";
  if (!scratch_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  int64_t npix;
  if (int rc = dist_check_shape(who, B, H, W, &npix)) return rc;
  *scratch_bytes = (npix * (int64_t)sizeof(int16_t) + 15) & ~(int64_t)15;
  return INSAR_OK;
}

template <typename T>
static void dist_launch_columns(int mode, const void* m, int H, int W, int v, int R, int16_t* sy, int64_t items, int nbands,
                                int wblocks, hipStream_t stream) {
  const dim3 grid(insar_grid_cap(items)), block(DT_THREADS);
  if (mode == INSAR_DIST_EQ)
    hipLaunchKernelGGL((dist_columns_kernel<T, INSAR_DIST_EQ>), grid, block, 0, stream, (const T*)m, H, W, v, R, sy, items, nbands, wblocks);
  else if (mode == INSAR_DIST_NE)
    hipLaunchKernelGGL((dist_columns_kernel<T, INSAR_DIST_NE>), grid, block, 0, stream, (const T*)m, H, W, v, R, sy, items, nbands, wblocks);
  else
    hipLaunchKernelGGL((dist_columns_kernel<T, INSAR_DIST_EDGE>), grid, block, 0, stream, (const T*)m, H, W, v, R, sy, items, nbands, wblocks);
}

extern "C" int insar_dist_transform(const void* m, int32_t elem_type, int32_t B, int32_t H, int32_t W, int32_t site_mode,
                                    int32_t value, int32_t max_distance, void* scratch, int32_t* d2, int32_t* nearest,
                                    void* stream) {
  const char* who = "insar_dist_transform";
  if (!m || !scratch || !d2) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !m ? "m" : !scratch ? "scratch" : "d2");
  if (elem_type != INSAR_DIST_U8 && elem_type != INSAR_DIST_I32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: element type %d: INSAR_DIST_U8 or INSAR_DIST_I32", who, elem_type);
  if (site_mode != INSAR_DIST_EQ && site_mode != INSAR_DIST_NE && site_mode != INSAR_DIST_EDGE)
    INSAR_FAIL(INSAR_E_ARG, "%s: site mode %d: INSAR_DIST_EQ, _NE or _EDGE", who, site_mode);
  int64_t npix;
  if (int rc = dist_check_shape(who, B, H, W, &npix)) return rc;
  if (elem_type == INSAR_DIST_I32 && (((uintptr_t)m) & 3u)) INSAR_FAIL(INSAR_E_ALIGN, "%s: int32 map not 4-byte aligned", who);
  if ((((uintptr_t)d2) | ((uintptr_t)nearest)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: d2 / nearest not 4-byte aligned", who);
  if (((uintptr_t)scratch) & 1u) INSAR_FAIL(INSAR_E_ALIGN, "%s: scratch not 2-byte aligned", who);
  const int R = max_distance <= 0 || max_distance > DT_MAX_R ? 0 : max_distance;
  const int nbands = (H + DT_BAND - 1) / DT_BAND, wblocks = (W + DT_THREADS - 1) / DT_THREADS;
  const int64_t items = (int64_t)B * nbands * wblocks;
  int16_t* sy = (int16_t*)scratch;
  if (elem_type == INSAR_DIST_U8)
    dist_launch_columns<uint8_t>(site_mode, m, H, W, value, R, sy, items, nbands, wblocks, (hipStream_t)stream);
  else
    dist_launch_columns<int32_t>(site_mode, m, H, W, value, R, sy, items, nbands, wblocks, (hipStream_t)stream);
  INSAR_CHECK_LAUNCH(who);
  const dim3 grid(insar_grid_cap((npix + DT_THREADS - 1) / DT_THREADS, 1 << 16)), block(DT_THREADS);
  if (nearest)
    hipLaunchKernelGGL(dist_rows_kernel<true>, grid, block, 0, (hipStream_t)stream, (const int16_t*)sy, H, W, R, npix, d2, nearest);
  else
    hipLaunchKernelGGL(dist_rows_kernel<false>, grid, block, 0, (hipStream_t)stream, (const int16_t*)sy, H, W, R, npix, d2, nearest);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_dist_boundary_counts(const uint8_t* pred, const uint8_t* gt, const int32_t* d2_pred, const int32_t* d2_gt,
                                          int32_t H, int32_t W, int64_t r2, int32_t K, int32_t void_value, int64_t* counts,
                                          void* stream) {
  const char* who = "insar_dist_boundary_counts";
  if (!pred || !gt || !d2_pred || !d2_gt || !counts) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  int64_t npix;
  if (int rc = dist_check_shape(who, 1, H, W, &npix)) return rc;
  if (K < 2 || K > DT_MAX_K) INSAR_FAIL(INSAR_E_SHAPE, "%s: %d classes outside 2..%d", who, K, DT_MAX_K);
  if (r2 < 0) INSAR_FAIL(INSAR_E_ARG, "%s: r2 %lld is negative", who, (long long)r2);
  if (void_value < -1 || void_value > 255) INSAR_FAIL(INSAR_E_ARG, "%s: void_value %d outside -1..255 (-1: none)", who, void_value);
  if ((((uintptr_t)d2_pred) | ((uintptr_t)d2_gt)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: d2 map not 4-byte aligned", who);
  if (((uintptr_t)counts) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: counts not 8-byte aligned", who);
  const int r2c = r2 >= (int64_t)INSAR_DIST_FAR ? INSAR_DIST_FAR - 1 : (int)r2;          // FAR is in no band
  const int vec = (npix % 4 == 0) && insar_aligned16(d2_pred) && insar_aligned16(d2_gt) &&
                  (((((uintptr_t)pred) | ((uintptr_t)gt)) & 3u) == 0);
  hipLaunchKernelGGL(dist_counts_clear_kernel, dim3(1), dim3(DT_THREADS), 0, (hipStream_t)stream, (long long*)counts, 3 * K);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(dist_counts_kernel, dim3(insar_grid_cap((npix / 4 + DT_THREADS) / DT_THREADS / 4, 1024)), dim3(DT_THREADS), 0,
                     (hipStream_t)stream, pred, gt, (const int*)d2_pred, (const int*)d2_gt, npix, vec, r2c, (int)K, (int)void_value,
                     (long long*)counts);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
