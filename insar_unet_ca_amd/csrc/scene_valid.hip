// Scenes with no-data: the three kernels that scene.hip's pipeline needs when not every pixel of the scene means something.
// census counts the valid pixels of each tile (the host then runs only the tiles that hold any), gather_valid is
// scene_gather_kernel with invalid pixels replaced by a fill value (and an affine normalisation of float32 scenes), and
// finalize_valid is scene_finalize_kernel with the invalid and the uncovered pixels forced to zero and a validity plane
// written next to the class map. Same conventions as scene.hip: HBM-bound streaming kernels, four adjacent pixels per
// thread where the addresses allow it, grid-stride, vector stores only, no atomics.
//
// A pixel is valid iff its byte of the validity plane is non-zero (no plane: every byte counts as 1), its value is not the
// no-data value (an exact compare) and, in a float32 scene, it is finite. The rule is scene_pixel_valid below and nowhere else.
#include "scene_common.h"

// (v - offset) * scale of gather_valid is two roundings, and finalize_valid repeats scene_finalize_kernel's arithmetic bit for bit
#pragma clang fp contract(off)

#define SC_THREADS 256
#define SC_MAX_K 8

template <typename S>
__device__ __forceinline__ bool scene_pixel_valid(S v, uint32_t vbyte, bool has_nodata, S nodata);
template <>
__device__ __forceinline__ bool scene_pixel_valid<uint8_t>(uint8_t v, uint32_t vbyte, bool has_nodata, uint8_t nodata) {
  return vbyte != 0u && !(has_nodata && v == nodata);
}
// a NaN no-data value compares unequal to everything: "non-finite only"
template <>
__device__ __forceinline__ bool scene_pixel_valid<float>(float v, uint32_t vbyte, bool has_nodata, float nodata) {
  const bool finite = (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
  return vbyte != 0u && finite && !(has_nodata && v == nodata);
}

// four adjacent scene pixels as they are stored, at any address
template <typename S>
__device__ __forceinline__ void scene_quad_raw(const S* p, S* v);
template <>
__device__ __forceinline__ void scene_quad_raw<uint8_t>(const uint8_t* p, uint8_t* v) {
  const uint32_t u = load4_u8_any(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (uint8_t)((u >> (8 * j)) & 0xffu);
}
template <>
__device__ __forceinline__ void scene_quad_raw<float>(const float* p, float* v) { image_quad<float>(p, v); }

// their four bytes of the validity plane; without a plane every pixel counts as observed
__device__ __forceinline__ uint32_t valid_quad(const uint8_t* valid, int64_t i) {
  return valid ? load4_u8_any(valid + i) : 0x01010101u;
}

__device__ __forceinline__ bool origin_inside(int y0, int x0, int T, int H, int W) {
  return y0 >= 0 && x0 >= 0 && y0 + T <= H && x0 + T <= W;
}

// ---------------------------------------------------------------------------------------------
// census: counts[t] = number of valid pixels of tile t. One work-group per tile (grid-stride over the table where it is
// longer than the grid), its threads stride over the tile's quads; the threads' counts reduce over the wave by shuffles,
// the waves' through LDS, and thread 0 writes the tile's count with one plain store. A tile whose origin lies outside the
// scene counts 0.
// ---------------------------------------------------------------------------------------------
template <typename S>
__global__ void __launch_bounds__(SC_THREADS)
scene_census_kernel(const S* __restrict__ scene, int H, int W, const uint8_t* __restrict__ valid, int has_nodata, S nodata,
                    const int32_t* __restrict__ origins, int n, int T, int32_t* __restrict__ counts) {
  __shared__ int part[SC_THREADS / INSAR_WAVE];
  const int qrow = T >> 2;                                   // quads per tile row
  const int nquads = T * qrow;                               // T <= 32768: fits
  for (int t = blockIdx.x; t < n; t += gridDim.x) {
    const int y0 = origins[2 * t], x0 = origins[2 * t + 1];
    int c = 0;
    if (origin_inside(y0, x0, T, H, W)) {
      for (int q = threadIdx.x; q < nquads; q += SC_THREADS) {
        const int64_t i = (int64_t)(y0 + q / qrow) * W + x0 + ((q % qrow) << 2);
        S v[4];
        scene_quad_raw<S>(scene + i, v);
        const uint32_t vb = valid_quad(valid, i);
#pragma unroll
        for (int j = 0; j < 4; ++j) c += scene_pixel_valid<S>(v[j], (vb >> (8 * j)) & 0xffu, has_nodata != 0, nodata) ? 1 : 0;
      }
    }
#pragma unroll
    for (int d = INSAR_WAVE / 2; d > 0; d >>= 1) c += __shfl_xor(c, d, INSAR_WAVE);
    if ((threadIdx.x & (INSAR_WAVE - 1)) == 0) part[threadIdx.x / INSAR_WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < SC_THREADS / INSAR_WAVE; ++w) s += part[w];
      counts[t] = s;
    }
    __syncthreads();                                         // part is written again for the block's next tile
  }
}

static int scene_valid_check_scene(const char* who, const void* scene, int32_t dtype, int32_t H, int32_t W, int32_t T,
                                   int32_t has_nodata, float nodata) {
  if (!scene) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (dtype != INSAR_SCENE_U8 && dtype != INSAR_SCENE_F32) INSAR_FAIL(INSAR_E_DTYPE, "%s: scene dtype %d (uint8 or float32)", who, dtype);
  if (T < 16 || T % 16 || T > 32768) INSAR_FAIL(INSAR_E_SHAPE, "%s: tile %d is not a multiple of 16 in 16..32768", who, T);
  if (H < T || W < T) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d smaller than the tile %d", who, H, W, T);
  if (dtype == INSAR_SCENE_F32 && (((uintptr_t)scene) & 3u)) INSAR_FAIL(INSAR_E_ALIGN, "%s: float32 scene not 4-byte aligned", who);
  if (has_nodata && dtype == INSAR_SCENE_U8 && !(nodata >= 0.f && nodata <= 255.f && nodata == (float)(int)nodata))
    INSAR_FAIL(INSAR_E_ARG, "%s: nodata %g of a uint8 scene is not an integer in 0..255", who, (double)nodata);
  return INSAR_OK;
}

extern "C" int insar_scene_census(const void* scene, int32_t dtype, int32_t H, int32_t W, const uint8_t* valid, int32_t has_nodata,
                                  float nodata, const int32_t* origins, int32_t n, int32_t T, int32_t* counts, void* stream) {
  if (!origins || !counts) INSAR_FAIL(INSAR_E_ARG, "insar_scene_census: null pointer");
  if (int rc = scene_valid_check_scene("insar_scene_census", scene, dtype, H, W, T, has_nodata, nodata)) return rc;
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_census: no tiles");
  hipStream_t s = (hipStream_t)stream;
  const int nb = insar_grid_cap(n);
  if (dtype == INSAR_SCENE_U8)
    hipLaunchKernelGGL(scene_census_kernel<uint8_t>, dim3(nb), dim3(SC_THREADS), 0, s, (const uint8_t*)scene, H, W, valid,
                       has_nodata, (uint8_t)(has_nodata ? (int)nodata : 0), origins, n, T, counts);
  else
    hipLaunchKernelGGL(scene_census_kernel<float>, dim3(nb), dim3(SC_THREADS), 0, s, (const float*)scene, H, W, valid, has_nodata,
                       nodata, origins, n, T, counts);
  INSAR_CHECK_LAUNCH("insar_scene_census");
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// gather_valid: scene_gather_kernel, one thread per four output pixels, one float4 store. A valid pixel of a uint8 scene
// gets the reference's ToTensor + Normalize (image_quad), one of a float32 scene x = (v - offset) * scale (has_norm) or v.
// An invalid pixel becomes `fill`; its value is replaced before the arithmetic, so that none is done on a NaN or an inf.
// ---------------------------------------------------------------------------------------------
template <typename S>
__global__ void __launch_bounds__(SC_THREADS)
scene_gather_valid_kernel(const S* __restrict__ scene, int H, int W, const uint8_t* __restrict__ valid, int has_nodata, S nodata,
                          float fill, int has_norm, float offset, float scale, const int32_t* __restrict__ origins, int n, int T,
                          float* __restrict__ out) {
  const int qrow = T >> 2;
  const int64_t nquads = (int64_t)n * T * qrow;
  for (int64_t q = blockIdx.x * (int64_t)SC_THREADS + threadIdx.x; q < nquads; q += (int64_t)gridDim.x * SC_THREADS) {
    const int tx = (int)(q % qrow) << 2;
    const int64_t r = q / qrow;
    const int ty = (int)(r % T);
    const int t = (int)(r / T);
    const int y0 = origins[2 * t], x0 = origins[2 * t + 1];
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (origin_inside(y0, x0, T, H, W)) {
      const int64_t i = (int64_t)(y0 + ty) * W + x0 + tx;
      S v[4];
      scene_quad_raw<S>(scene + i, v);
      const uint32_t vb = valid_quad(valid, i);
      bool ok[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) ok[j] = scene_pixel_valid<S>(v[j], (vb >> (8 * j)) & 0xffu, has_nodata != 0, nodata);
      if constexpr (sizeof(S) == 1) {
        image_quad<S>(scene + i, f);                         // the same dword as v: one load
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x = ok[j] ? v[j] : offset;
          f[j] = has_norm ? (x - offset) * scale : x;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = ok[j] ? f[j] : fill;
    }
    *reinterpret_cast<float4*>(out + (q << 2)) = make_float4(f[0], f[1], f[2], f[3]);
  }
}

extern "C" int insar_scene_gather_valid(const void* scene, int32_t dtype, int32_t H, int32_t W, const uint8_t* valid,
                                        int32_t has_nodata, float nodata, float fill, int32_t has_norm, float offset, float scale,
                                        const int32_t* origins, int32_t n, int32_t T, float* out, void* stream) {
  if (!origins || !out) INSAR_FAIL(INSAR_E_ARG, "insar_scene_gather_valid: null pointer");
  if (int rc = scene_valid_check_scene("insar_scene_gather_valid", scene, dtype, H, W, T, has_nodata, nodata)) return rc;
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_gather_valid: no tiles");
  if (!insar_aligned16(out)) INSAR_FAIL(INSAR_E_ALIGN, "insar_scene_gather_valid: out not 16-byte aligned");
  if (!std::isfinite(fill)) INSAR_FAIL(INSAR_E_ARG, "insar_scene_gather_valid: fill is not finite");
  if (has_norm && dtype != INSAR_SCENE_F32) INSAR_FAIL(INSAR_E_DTYPE, "insar_scene_gather_valid: norm is for float32 scenes (a uint8 scene has the reference's transform)");
  if (has_norm && (!std::isfinite(offset) || !std::isfinite(scale) || scale == 0.f))
    INSAR_FAIL(INSAR_E_ARG, "insar_scene_gather_valid: norm needs a finite offset and a finite non-zero scale");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nquads = (int64_t)n * T * (T / 4);
  const int nb = insar_grid_cap((nquads + SC_THREADS - 1) / SC_THREADS);
  if (dtype == INSAR_SCENE_U8)
    hipLaunchKernelGGL(scene_gather_valid_kernel<uint8_t>, dim3(nb), dim3(SC_THREADS), 0, s, (const uint8_t*)scene, H, W, valid,
                       has_nodata, (uint8_t)(has_nodata ? (int)nodata : 0), fill, 0, 0.f, 1.f, origins, n, T, out);
  else
    hipLaunchKernelGGL(scene_gather_valid_kernel<float>, dim3(nb), dim3(SC_THREADS), 0, s, (const float*)scene, H, W, valid,
                       has_nodata, nodata, fill, has_norm, offset, scale, origins, n, T, out);
  INSAR_CHECK_LAUNCH("insar_scene_gather_valid");
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// finalize_valid: scene_finalize_kernel's arithmetic (prob = acc / wsum, argmax with ties to the lower class, conf =
// prob[mask]) at the pixels that are valid and covered (wsum > 0); everywhere else prob = mask = conf = 0, by a select: a
// NaN in acc does not get through, and nothing is divided by a wsum of 0. The validity rule is evaluated again from the
// scene and the plane (5 bytes a pixel at most; no scene-sized plane is kept between census and finalize), and
// valid_out = 1 where the pixel is valid and covered. The planes are walked as flat arrays, four pixels per thread where
// npix % 4 == 0 and the buffers are aligned for it (then valid_out and mask move as one dword each).
// ---------------------------------------------------------------------------------------------
template <typename S, int K, int V>
__global__ void __launch_bounds__(SC_THREADS)
scene_finalize_valid_kernel(const float* __restrict__ acc, const float* __restrict__ wsum, int64_t npix,
                            const S* __restrict__ scene, const uint8_t* __restrict__ valid, int has_nodata, S nodata,
                            float* __restrict__ prob, uint8_t* __restrict__ mask, float* __restrict__ conf,
                            uint8_t* __restrict__ valid_out) {
  const int64_t nwork = npix / V;
  for (int64_t g = blockIdx.x * (int64_t)SC_THREADS + threadIdx.x; g < nwork; g += (int64_t)gridDim.x * SC_THREADS) {
    const int64_t pix = g * V;
    float a[K][V], ws[V];
    S sv[V];
    uint32_t vb;
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(acc + k * npix + pix);
        a[k][0] = v.x; a[k][1] = v.y; a[k][2] = v.z; a[k][3] = v.w;
      }
      const float4 v = *reinterpret_cast<const float4*>(wsum + pix);
      ws[0] = v.x; ws[1] = v.y; ws[2] = v.z; ws[3] = v.w;
      scene_quad_raw<S>(scene + pix, sv);
      vb = valid_quad(valid, pix);
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) a[k][0] = acc[k * npix + pix];
      ws[0] = wsum[pix];
      sv[0] = scene[pix];
      vb = valid ? (uint32_t)valid[pix] : 1u;
    }
    float best[V];
    uint32_t arg[V], keep[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool ok = ws[j] > 0.f && scene_pixel_valid<S>(sv[j], (vb >> (8 * j)) & 0xffu, has_nodata != 0, nodata);
      const float den = ok ? ws[j] : 1.f;
      keep[j] = ok ? 1u : 0u;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float p = a[k][j] / den;
        a[k][j] = ok ? p : 0.f;
      }
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
      *reinterpret_cast<uint32_t*>(valid_out + pix) = keep[0] | (keep[1] << 8) | (keep[2] << 16) | (keep[3] << 24);
    } else {
      if (prob) {
#pragma unroll
        for (int k = 0; k < K; ++k) prob[k * npix + pix] = a[k][0];
      }
      mask[pix] = (uint8_t)arg[0];
      conf[pix] = best[0];
      valid_out[pix] = (uint8_t)keep[0];
    }
  }
}

template <typename S>
static void scene_finalize_valid_launch(int K, bool v4, int nb, hipStream_t s, const float* acc, const float* wsum, int64_t npix,
                                        const S* scene, const uint8_t* valid, int has_nodata, S nodata, float* prob, uint8_t* mask,
                                        float* conf, uint8_t* valid_out) {
#define SC_FINV(KK)                                                                                                          \
  case KK:                                                                                                                   \
    if (v4) hipLaunchKernelGGL((scene_finalize_valid_kernel<S, KK, 4>), dim3(nb), dim3(SC_THREADS), 0, s, acc, wsum, npix,   \
                               scene, valid, has_nodata, nodata, prob, mask, conf, valid_out);                               \
    else hipLaunchKernelGGL((scene_finalize_valid_kernel<S, KK, 1>), dim3(nb), dim3(SC_THREADS), 0, s, acc, wsum, npix,      \
                            scene, valid, has_nodata, nodata, prob, mask, conf, valid_out);                                  \
    break;
  switch (K) { SC_FINV(2) SC_FINV(3) SC_FINV(4) SC_FINV(5) SC_FINV(6) SC_FINV(7) SC_FINV(8) }
#undef SC_FINV
}

extern "C" int insar_scene_finalize_valid(const float* acc, const float* wsum, int32_t K, int32_t H, int32_t W, const void* scene,
                                          int32_t dtype, const uint8_t* valid, int32_t has_nodata, float nodata, float* prob,
                                          uint8_t* mask, float* conf, uint8_t* valid_out, void* stream) {
  if (!acc || !wsum || !scene || !mask || !conf || !valid_out) INSAR_FAIL(INSAR_E_ARG, "insar_scene_finalize_valid: null pointer");
  if (K < 2 || K > SC_MAX_K) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_finalize_valid: num_classes %d outside 2..%d", K, SC_MAX_K);
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_scene_finalize_valid: empty scene %d x %d", H, W);
  if (dtype != INSAR_SCENE_U8 && dtype != INSAR_SCENE_F32) INSAR_FAIL(INSAR_E_DTYPE, "insar_scene_finalize_valid: scene dtype %d (uint8 or float32)", dtype);
  if (has_nodata && dtype == INSAR_SCENE_U8 && !(nodata >= 0.f && nodata <= 255.f && nodata == (float)(int)nodata))
    INSAR_FAIL(INSAR_E_ARG, "insar_scene_finalize_valid: nodata %g of a uint8 scene is not an integer in 0..255", (double)nodata);
  if ((((uintptr_t)acc) | ((uintptr_t)wsum) | ((uintptr_t)prob) | ((uintptr_t)conf)) & 3u)
    INSAR_FAIL(INSAR_E_ALIGN, "insar_scene_finalize_valid: buffer not 4-byte aligned");
  if (dtype == INSAR_SCENE_F32 && (((uintptr_t)scene) & 3u)) INSAR_FAIL(INSAR_E_ALIGN, "insar_scene_finalize_valid: float32 scene not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)H * W;
  // the scene and the plane are read at any address (scene_quad_raw, valid_quad); what is stored four at a time must be aligned
  const bool v4 = (npix % 4 == 0) && insar_aligned16(acc) && insar_aligned16(wsum) && insar_aligned16(prob) && insar_aligned16(conf) &&
                  ((((uintptr_t)mask) | ((uintptr_t)valid_out)) & 3u) == 0;
  const int nb = insar_grid_cap((npix / (v4 ? 4 : 1) + SC_THREADS - 1) / SC_THREADS);
  if (dtype == INSAR_SCENE_U8)
    scene_finalize_valid_launch<uint8_t>(K, v4, nb, s, acc, wsum, npix, (const uint8_t*)scene, valid, has_nodata,
                                         (uint8_t)(has_nodata ? (int)nodata : 0), prob, mask, conf, valid_out);
  else
    scene_finalize_valid_launch<float>(K, v4, nb, s, acc, wsum, npix, (const float*)scene, valid, has_nodata, nodata, prob, mask,
                                       conf, valid_out);
  INSAR_CHECK_LAUNCH("insar_scene_finalize_valid");
  return INSAR_OK;
}
