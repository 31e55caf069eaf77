// Whole-scene inference: cut a scene into tiles (gather), blend the tiles' class probabilities back into scene-sized
// accumulators (blend), and turn the accumulators into a probability map, a class map and a confidence map (finalize).
// All three are HBM-bound streaming kernels: one thread owns four horizontally adjacent pixels (one 16-byte access per
// plane) where the addresses allow it, one pixel otherwise; grid-stride over the work; vector stores only.
//
// Determinism: the blend is in GATHER form. A thread owns scene pixels, looks up the tiles of the batch that cover them in
// the origin table and adds their contributions in ascending tile index, so that a pixel's sum is one fixed chain of
// fp32 operations (acc = fma(w, p, acc); wsum = wsum + w) whatever the batch size: the chain is merely cut at batch
// boundaries, where acc / wsum pass through memory unchanged. No atomics, no dependence on scheduling.
#include "scene_common.h"

// every multiply-add below is written out (fmaf) or meant to stay two roundings: the bitwise contract of the blend must not
// hang on where the compiler chooses to fuse
#pragma clang fp contract(off)

#define SC_THREADS 256
#define SC_MAX_K 8

// r(i) = min(i + 1, T - i, o + 1) / (o + 1): the 1-D trapezoid window (infer.window_1d computes the same fp32 quotient)
__device__ __forceinline__ float scene_ramp(int i, int T, int o) {
  int m = i + 1;
  if (T - i < m) m = T - i;
  if (o + 1 < m) m = o + 1;
  return (float)m / (float)(o + 1);
}

// ---------------------------------------------------------------------------------------------
// gather: out[t][0][ty][tx] = norm(scene[y0_t + ty][x0_t + tx]); uint8 scenes get the reference's ToTensor + Normalize
// (x = v / 255; (x - 0.5) / 0.5, data.reference_transforms), float32 scenes are copied (image_quad). One thread per four output
// pixels (T % 4 == 0: a quad never leaves its tile row). A tile whose origin lies outside the scene is zero-filled.
// ---------------------------------------------------------------------------------------------
template <typename S>
__global__ void __launch_bounds__(SC_THREADS)
scene_gather_kernel(const S* __restrict__ scene, int H, int W, const int32_t* __restrict__ origins, int n, int T,
                    float* __restrict__ out) {
  const int qrow = T >> 2;                                   // quads per tile row
  const int64_t nquads = (int64_t)n * T * qrow;
  for (int64_t q = blockIdx.x * (int64_t)SC_THREADS + threadIdx.x; q < nquads; q += (int64_t)gridDim.x * SC_THREADS) {
    const int tx = (int)(q % qrow) << 2;
    const int64_t r = q / qrow;
    const int ty = (int)(r % T);
    const int t = (int)(r / T);
    const int y0 = origins[2 * t], x0 = origins[2 * t + 1];
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (y0 >= 0 && x0 >= 0 && y0 + T <= H && x0 + T <= W)
      image_quad<S>(scene + (int64_t)(y0 + ty) * W + x0 + tx, f);
    *reinterpret_cast<float4*>(out + (q << 2)) = make_float4(f[0], f[1], f[2], f[3]);
  }
}

extern "C" int insar_scene_gather(const void* scene, int32_t dtype, int32_t H, int32_t W, const int32_t* origins,
                                  int32_t n, int32_t T, float* out, void* stream) {
  if (!scene || !origins || !out) INSAR_FAIL(INSAR_E_ARG, "insar_scene_gather: null pointer");
  if (dtype != INSAR_SCENE_U8 && dtype != INSAR_SCENE_F32) INSAR_FAIL(INSAR_E_DTYPE, "insar_scene_gather: scene dtype %d (uint8 or float32)", dtype);
  if (T < 16 || T % 16) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_gather: tile %d is not a positive multiple of 16", T);
  if (H < T || W < T) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_gather: scene %d x %d smaller than the tile %d", H, W, T);
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_gather: no tiles");
  if (!insar_aligned16(out)) INSAR_FAIL(INSAR_E_ALIGN, "insar_scene_gather: out not 16-byte aligned");
  if (dtype == INSAR_SCENE_F32 && (((uintptr_t)scene) & 3u)) INSAR_FAIL(INSAR_E_ALIGN, "insar_scene_gather: float32 scene not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nquads = (int64_t)n * T * (T / 4);
  const int nb = insar_grid_cap((nquads + SC_THREADS - 1) / SC_THREADS);
  if (dtype == INSAR_SCENE_U8)
    hipLaunchKernelGGL(scene_gather_kernel<uint8_t>, dim3(nb), dim3(SC_THREADS), 0, s, (const uint8_t*)scene, H, W, origins, n, T, out);
  else
    hipLaunchKernelGGL(scene_gather_kernel<float>, dim3(nb), dim3(SC_THREADS), 0, s, (const float*)scene, H, W, origins, n, T, out);
  INSAR_CHECK_LAUNCH("insar_scene_gather");
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// blend: a thread owns V (4, or 1 where W % 4 != 0 or a buffer is not 16-byte aligned) adjacent pixels of the batch's
// bounding box [y_lo, y_hi) x [x_lo, x_hi) and walks the batch's origin table in index order. The table entries are
// wave-uniform (scalar loads); the logits of a covering tile come in as one 16-byte load per class where the quad lies
// whole in the tile on a 16-byte boundary of its row, element by element otherwise; the arithmetic below the loads is
// the same code either way. acc / wsum are read on the first covering tile and written once; pixels that no tile of the
// batch covers cost no memory traffic.
// ---------------------------------------------------------------------------------------------
template <int K, int V>
__global__ void __launch_bounds__(SC_THREADS)
scene_blend_kernel(const float* __restrict__ logits, const int32_t* __restrict__ origins, int n, int T, int o,
                   float* __restrict__ acc, float* __restrict__ wsum, int H, int W, int y_lo, int y_hi, int x_lo, int x_hi) {
  const int gw = (x_hi - x_lo + V - 1) / V;                  // thread columns of the box (x_lo is a multiple of V)
  const int64_t nwork = (int64_t)(y_hi - y_lo) * gw;
  const int64_t plane = (int64_t)H * W;
  const int64_t tplane = (int64_t)T * T;
  for (int64_t g = blockIdx.x * (int64_t)SC_THREADS + threadIdx.x; g < nwork; g += (int64_t)gridDim.x * SC_THREADS) {
    const int y = y_lo + (int)(g / gw);
    const int x = x_lo + (int)(g % gw) * V;
    const int64_t pix = (int64_t)y * W + x;
    float a[K][V], ws[V];
    bool loaded = false;
    for (int t = 0; t < n; ++t) {
      const int y0 = origins[2 * t], x0 = origins[2 * t + 1];
      if (y0 < 0 || x0 < 0 || y0 + T > H || x0 + T > W) continue;          // not a tile of this scene: ignored
      const int yi = y - y0, xi = x - x0;
      if (yi < 0 || yi >= T || xi + V <= 0 || xi >= T) continue;
      if (!loaded) {
        loaded = true;
        if constexpr (V == 4) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(acc + k * plane + pix);
            a[k][0] = v.x; a[k][1] = v.y; a[k][2] = v.z; a[k][3] = v.w;
          }
          const float4 v = *reinterpret_cast<const float4*>(wsum + pix);
          ws[0] = v.x; ws[1] = v.y; ws[2] = v.z; ws[3] = v.w;
        } else {
#pragma unroll
          for (int k = 0; k < K; ++k) a[k][0] = acc[k * plane + pix];
          ws[0] = wsum[pix];
        }
      }
      const float* lp = logits + (int64_t)t * K * tplane + (int64_t)yi * T + xi;
      float lg[K][V];
      bool in[V];
#pragma unroll
      for (int j = 0; j < V; ++j) in[j] = (xi + j >= 0) && (xi + j < T);
      bool vec = false;
      if constexpr (V == 4) {
        vec = xi >= 0 && xi + 4 <= T && (xi & 3) == 0;
        if (vec) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(lp + k * tplane);
            lg[k][0] = v.x; lg[k][1] = v.y; lg[k][2] = v.z; lg[k][3] = v.w;
          }
        }
      }
      if (!vec) {
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int j = 0; j < V; ++j) lg[k][j] = in[j] ? lp[k * tplane + j] : 0.f;
      }
      const float ry = scene_ramp(yi, T, o);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (!in[j]) continue;
        const float w = ry * scene_ramp(xi + j, T, o);
        float mx = lg[0][j];
#pragma unroll
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, lg[k][j]);
        float e[K], sum = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) { e[k] = expf(lg[k][j] - mx); sum += e[k]; }
#pragma unroll
        for (int k = 0; k < K; ++k) a[k][j] = fmaf(w, e[k] / sum, a[k][j]);
        ws[j] += w;
      }
    }
    if (!loaded) continue;
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        *reinterpret_cast<float4*>(acc + k * plane + pix) = make_float4(a[k][0], a[k][1], a[k][2], a[k][3]);
      *reinterpret_cast<float4*>(wsum + pix) = make_float4(ws[0], ws[1], ws[2], ws[3]);
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k * plane + pix] = a[k][0];
      wsum[pix] = ws[0];
    }
  }
}

static int scene_check_geometry(const char* who, int32_t K, int32_t T, int32_t overlap, int32_t H, int32_t W) {
  if (K < 2 || K > SC_MAX_K) INSAR_FAIL(INSAR_E_SHAPE, "%s: num_classes %d outside 2..%d", who, K, SC_MAX_K);
  if (T < 16 || T % 16) INSAR_FAIL(INSAR_E_SHAPE, "%s: tile %d is not a positive multiple of 16", who, T);
  if (overlap < 0 || overlap > T / 2) INSAR_FAIL(INSAR_E_SHAPE, "%s: overlap %d outside 0..tile/2 = %d", who, overlap, T / 2);
  if (H < T || W < T) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d smaller than the tile %d", who, H, W, T);
  return INSAR_OK;
}

template <int V>
static void scene_blend_launch(int K, int nb, hipStream_t s, const float* logits, const int32_t* origins, int n, int T, int o,
                               float* acc, float* wsum, int H, int W, int y_lo, int y_hi, int x_lo, int x_hi) {
#define SC_BLEND(KK)                                                                                                      \
  case KK:                                                                                                                \
    hipLaunchKernelGGL((scene_blend_kernel<KK, V>), dim3(nb), dim3(SC_THREADS), 0, s, logits, origins, n, T, o, acc, wsum, \
                       H, W, y_lo, y_hi, x_lo, x_hi);                                                                     \
    break;
  switch (K) { SC_BLEND(2) SC_BLEND(3) SC_BLEND(4) SC_BLEND(5) SC_BLEND(6) SC_BLEND(7) SC_BLEND(8) }
#undef SC_BLEND
}

extern "C" int insar_scene_blend(const float* logits, const int32_t* origins, int32_t n, int32_t K, int32_t T, int32_t overlap,
                                 float* acc, float* wsum, int32_t H, int32_t W, int32_t y_lo, int32_t y_hi, int32_t x_lo,
                                 int32_t x_hi, void* stream) {
  if (!logits || !origins || !acc || !wsum) INSAR_FAIL(INSAR_E_ARG, "insar_scene_blend: null pointer");
  if (int rc = scene_check_geometry("insar_scene_blend", K, T, overlap, H, W)) return rc;
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_blend: no tiles");
  if (y_lo < 0 || x_lo < 0 || y_hi > H || x_hi > W || y_lo >= y_hi || x_lo >= x_hi)
    INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_blend: box [%d, %d) x [%d, %d) is empty or leaves the %d x %d scene", y_lo, y_hi, x_lo, x_hi, H, W);
  if ((((uintptr_t)logits) | ((uintptr_t)acc) | ((uintptr_t)wsum)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "insar_scene_blend: buffer not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const bool v4 = (W % 4 == 0) && insar_aligned16(logits) && insar_aligned16(acc) && insar_aligned16(wsum);
  if (v4) {
    x_lo &= ~3;                                              // whole quads; x_hi <= W and W % 4 == 0 keep the last one inside
    const int64_t nwork = (int64_t)(y_hi - y_lo) * ((x_hi - x_lo + 3) / 4);
    scene_blend_launch<4>(K, insar_grid_cap((nwork + SC_THREADS - 1) / SC_THREADS), s, logits, origins, n, T, overlap, acc, wsum,
                          H, W, y_lo, y_hi, x_lo, x_hi);
  } else {
    const int64_t nwork = (int64_t)(y_hi - y_lo) * (x_hi - x_lo);
    scene_blend_launch<1>(K, insar_grid_cap((nwork + SC_THREADS - 1) / SC_THREADS), s, logits, origins, n, T, overlap, acc, wsum,
                          H, W, y_lo, y_hi, x_lo, x_hi);
  }
  INSAR_CHECK_LAUNCH("insar_scene_blend");
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// finalize: per pixel prob[k] = acc[k] / wsum, mask = argmax_k (ties to the lower class, the rule of insar_confusion),
// conf = prob[mask]. Nothing here is two-dimensional: the H x W planes are walked as flat arrays of npix pixels, four per
// thread where npix % 4 == 0. A pixel that no tile covered (wsum == 0) gets prob = 0, mask = 0, conf = 0.
// ---------------------------------------------------------------------------------------------
template <int K, int V>
__global__ void __launch_bounds__(SC_THREADS)
scene_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ wsum, int64_t npix, float* __restrict__ prob,
                      uint8_t* __restrict__ mask, float* __restrict__ conf) {
  const int64_t nwork = npix / V;
  for (int64_t g = blockIdx.x * (int64_t)SC_THREADS + threadIdx.x; g < nwork; g += (int64_t)gridDim.x * SC_THREADS) {
    const int64_t pix = g * V;
    float a[K][V], ws[V];
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(acc + k * npix + pix);
        a[k][0] = v.x; a[k][1] = v.y; a[k][2] = v.z; a[k][3] = v.w;
      }
      const float4 v = *reinterpret_cast<const float4*>(wsum + pix);
      ws[0] = v.x; ws[1] = v.y; ws[2] = v.z; ws[3] = v.w;
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) a[k][0] = acc[k * npix + pix];
      ws[0] = wsum[pix];
    }
    float best[V];
    uint32_t arg[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool covered = ws[j] > 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) a[k][j] = covered ? a[k][j] / ws[j] : 0.f;
      best[j] = a[0][j]; arg[j] = 0;
#pragma unroll
      for (int k = 1; k < K; ++k)
        if (a[k][j] > best[j]) { best[j] = a[k][j]; arg[j] = k; }
    }
    if constexpr (V == 4) {
      if (prob) {
#pragma unroll
        for (int k = 0; k < K; ++k)
          *reinterpret_cast<float4*>(prob + k * npix + pix) = make_float4(a[k][0], a[k][1], a[k][2], a[k][3]);
      }
      *reinterpret_cast<uint32_t*>(mask + pix) = arg[0] | (arg[1] << 8) | (arg[2] << 16) | (arg[3] << 24);
      *reinterpret_cast<float4*>(conf + pix) = make_float4(best[0], best[1], best[2], best[3]);
    } else {
      if (prob) {
#pragma unroll
        for (int k = 0; k < K; ++k) prob[k * npix + pix] = a[k][0];
      }
      mask[pix] = (uint8_t)arg[0];
      conf[pix] = best[0];
    }
  }
}

extern "C" int insar_scene_finalize(const float* acc, const float* wsum, int32_t K, int32_t H, int32_t W, float* prob,
                                    uint8_t* mask, float* conf, void* stream) {
  if (!acc || !wsum || !mask || !conf) INSAR_FAIL(INSAR_E_ARG, "insar_scene_finalize: null pointer");
  if (K < 2 || K > SC_MAX_K) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_finalize: num_classes %d outside 2..%d", K, SC_MAX_K);
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_finalize: empty scene %d x %d", H, W);
  if ((((uintptr_t)acc) | ((uintptr_t)wsum) | ((uintptr_t)prob) | ((uintptr_t)conf)) & 3u)
    INSAR_FAIL(INSAR_E_ALIGN, "insar_scene_finalize: buffer not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)H * W;
  const bool v4 = (npix % 4 == 0) && insar_aligned16(acc) && insar_aligned16(wsum) && insar_aligned16(prob) &&
                  insar_aligned16(conf) && ((((uintptr_t)mask) & 3u) == 0);
  const int nb = insar_grid_cap((npix / (v4 ? 4 : 1) + SC_THREADS - 1) / SC_THREADS);
#define SC_FIN(KK)                                                                                                             \
  case KK:                                                                                                                     \
    if (v4) hipLaunchKernelGGL((scene_finalize_kernel<KK, 4>), dim3(nb), dim3(SC_THREADS), 0, s, acc, wsum, npix, prob, mask, conf); \
    else hipLaunchKernelGGL((scene_finalize_kernel<KK, 1>), dim3(nb), dim3(SC_THREADS), 0, s, acc, wsum, npix, prob, mask, conf);    \
    break;
  switch (K) { SC_FIN(2) SC_FIN(3) SC_FIN(4) SC_FIN(5) SC_FIN(6) SC_FIN(7) SC_FIN(8) }
#undef SC_FIN
  INSAR_CHECK_LAUNCH("insar_scene_finalize");
  return INSAR_OK;
}
