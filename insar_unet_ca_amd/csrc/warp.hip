// Resampling rasters: a fixed-point affine warp (insar_warp_raster for whole rasters and label maps, insar_warp_gather for
// training crops, insar_warp_draw for the matrices of a batch) and the exact box mean (insar_multilook). A warp is six
// int64 in Q32 that take destination pixel indices to source pixel indices; positions are cut to 1/256 pixel, the
// rasteriser's unit, and everything that decides anything is integer. The float32 interpolation is four products and three
// sums in one stated order, each rounded on its own. Nothing is read back, there are no atomics and no work-group waits on
// another: every output is bitwise defined (include/insar_hip.h states the arithmetic, tests/warp_ref.py restates it).
//
// Launch shape of the two warp kernels: a work-group of 256 threads covers a 64 x 16 block of destination pixels, one thread
// four adjacent pixels of a row, so that the source footprint of a work-group stays a compact parallelogram under rotation
// and its taps are served from L2; work-groups that share an XCD get consecutive blocks (xcd_tile). The taps are scalar
// gathers, the stores 16 bytes (4 for uint8) per thread where the width allows, guarded scalars otherwise.
#include <type_traits>

#include "scene_common.h"

// the contract is bitwise: no product below may fuse with a sum
#pragma clang fp contract(off)

#define WP_THREADS 256
#define WP_BX 64
#define WP_BY 16
#define WP_MAX_C 4
#define WP_MAX_DIM 32768
#define WP_ANGLES 1024
#define WP_MAX_ZOOM 4096
#define WP_STREAM 0x9FB21C651E98DF25ull          // separates the warp draws from the crop draws of the same batch key

// ---------------------------------------------------------------------------------------------
// coordinates
// ---------------------------------------------------------------------------------------------
struct WarpMat { int64_t a, b, c, d, e, f; };

__device__ __forceinline__ WarpMat warp_mat(const int64_t* __restrict__ m) {
  WarpMat r;
  r.a = m[0]; r.b = m[1]; r.c = m[2]; r.d = m[3]; r.e = m[4]; r.f = m[5];
  return r;
}
// (a x + b y + c + 2^23) >> 24 in int64 with wrap-around (the sums go through uint64: no table content is undefined)
__device__ __forceinline__ int64_t warp_pos(int64_t a, int64_t b, int64_t c, int x, int y) {
  const uint64_t q = (uint64_t)a * (uint64_t)(int64_t)x + (uint64_t)b * (uint64_t)(int64_t)y + (uint64_t)c + (1ull << 23);
  return (int64_t)q >> 24;
}
__device__ __forceinline__ bool warp_inside(int64_t sx, int64_t sy, int H, int W) {
  return sx >= -128 && sx < 256 * (int64_t)W - 128 && sy >= -128 && sy < 256 * (int64_t)H - 128;
}
// inside only: sx + 128 in [0, 256 W), the index in [0, W); H W < 2^31 keeps the offset an int
__device__ __forceinline__ int warp_nearest_at(int64_t sx, int64_t sy, int W) {
  return (int)((sy + 128) >> 8) * W + (int)((sx + 128) >> 8);
}
// inside only: sx >> 8 in [-1, W - 1], the two taps clamped to [0, W - 1]
struct WarpTaps { int o00, o01, o10, o11, fx, fy; };
__device__ __forceinline__ WarpTaps warp_taps(int64_t sx, int64_t sy, int H, int W) {
  const int ix = (int)(sx >> 8), iy = (int)(sy >> 8);
  const int x0 = ix < 0 ? 0 : ix, x1 = ix + 1 > W - 1 ? W - 1 : ix + 1;
  const int y0 = iy < 0 ? 0 : iy, y1 = iy + 1 > H - 1 ? H - 1 : iy + 1;
  WarpTaps t;
  t.o00 = y0 * W + x0; t.o01 = y0 * W + x1; t.o10 = y1 * W + x0; t.o11 = y1 * W + x1;
  t.fx = (int)(sx & 255); t.fy = (int)(sy & 255);
  return t;
}
__device__ __forceinline__ int warp_bilinear(const uint8_t* __restrict__ p, const WarpTaps& t) {
  const int wx0 = 256 - t.fx, wy0 = 256 - t.fy;
  const int s = wx0 * wy0 * (int)p[t.o00] + t.fx * wy0 * (int)p[t.o01] + wx0 * t.fy * (int)p[t.o10] + t.fx * t.fy * (int)p[t.o11];
  return (s + 32768) >> 16;                                          // the weights sum to 65536: 0..255
}
// a computed NaN leaves as the one quiet NaN 0x7fc00000: which payload and sign an operation hands on is not part of the contract
__device__ __forceinline__ float warp_quiet(float v) { return v == v ? v : __int_as_float(0x7fc00000); }
__device__ __forceinline__ float warp_bilinear(const float* __restrict__ p, const WarpTaps& t) {
  const float wx0 = (float)(256 - t.fx), wx1 = (float)t.fx, wy0 = (float)(256 - t.fy), wy1 = (float)t.fy;
  const float top = p[t.o00] * wx0 + p[t.o01] * wx1;
  const float bot = p[t.o10] * wx0 + p[t.o11] * wx1;
  return warp_quiet((top * wy0 + bot * wy1) * 0x1p-16f);
}

// four adjacent elements of a destination row of width w that start at column x: p is the row
__device__ __forceinline__ void warp_store(int32_t* p, int x, int w, bool vec, const int32_t* v) { quad_store(p, x, w, vec, v); }
__device__ __forceinline__ void warp_store(float* p, int x, int w, bool vec, const float* v) {
  const int u[4] = {__float_as_int(v[0]), __float_as_int(v[1]), __float_as_int(v[2]), __float_as_int(v[3])};
  quad_store(reinterpret_cast<int*>(p), x, w, vec, u);
}
__device__ __forceinline__ void warp_store(uint8_t* p, int x, int w, bool vec, const uint8_t* v) {
  if (vec) {
    *reinterpret_cast<uint32_t*>(p + x) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < w) p[x + j] = v[j];
  }
}

// the 64 x 16 block of this work-group and the quad of this thread in it; false where the quad lies outside the h x w plane
struct WarpQuad { int s, x, y; };
__device__ __forceinline__ bool warp_quad(int h, int w, WarpQuad& q) {
  const int bxn = (w + WP_BX - 1) / WP_BX, byn = (h + WP_BY - 1) / WP_BY;
  const int b = xcd_tile((int)blockIdx.x, (int)gridDim.x);
  q.x = (b % bxn) * WP_BX + ((int)threadIdx.x & 15) * 4;
  const int r = b / bxn;
  q.y = (r % byn) * WP_BY + ((int)threadIdx.x >> 4);
  q.s = r / byn;
  return q.x < w && q.y < h;
}

// ---------------------------------------------------------------------------------------------
// insar_warp_raster
// ---------------------------------------------------------------------------------------------
template <typename S, int MODE>
__global__ void __launch_bounds__(WP_THREADS)
warp_raster_kernel(const S* __restrict__ src, int C, int H, int W, const int64_t* __restrict__ mats, int h, int w, S fill,
                   S* __restrict__ dst, uint8_t* __restrict__ valid, bool vec, bool vec_valid) {
  WarpQuad q;
  if (!warp_quad(h, w, q)) return;
  const WarpMat m = warp_mat(mats + 6 * (int64_t)q.s);
  bool in[4];
  int at[4];
  WarpTaps tp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t sx = warp_pos(m.a, m.b, m.c, q.x + j, q.y), sy = warp_pos(m.d, m.e, m.f, q.x + j, q.y);
    in[j] = q.x + j < w && warp_inside(sx, sy, H, W);
    if constexpr (MODE == INSAR_WARP_BILINEAR) {
      if (in[j]) tp[j] = warp_taps(sx, sy, H, W);
    } else {
      at[j] = in[j] ? warp_nearest_at(sx, sy, W) : 0;
    }
  }
  const int64_t plane = (int64_t)H * W;
  for (int c = 0; c < C; ++c) {
    const S* p = src + c * plane;
    S v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = fill;
      if (in[j]) {
        if constexpr (MODE == INSAR_WARP_BILINEAR) v[j] = (S)warp_bilinear(p, tp[j]);
        else v[j] = p[at[j]];
      }
    }
    warp_store(dst + (((int64_t)q.s * C + c) * h + q.y) * w, q.x, w, vec, v);
  }
  if (valid) {
    const uint8_t v[4] = {(uint8_t)in[0], (uint8_t)in[1], (uint8_t)in[2], (uint8_t)in[3]};
    warp_store(valid + ((int64_t)q.s * h + q.y) * w, q.x, w, vec_valid, v);
  }
}

static int warp_check_source(const char* who, int32_t C, int32_t H, int32_t W) {
  if (C < 1 || C > WP_MAX_C) INSAR_FAIL(INSAR_E_SHAPE, "%s: %d channels outside 1..%d", who, C, WP_MAX_C);
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty source %d x %d", who, H, W);
  if ((int64_t)H * W >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: source %d x %d has 2^31 pixels or more", who, H, W);
  return INSAR_OK;
}

static int warp_blocks(const char* who, int32_t n, int32_t h, int32_t w, int64_t* blocks) {
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: n = %d matrices", who, n);
  if (h < 1 || w < 1 || h > WP_MAX_DIM || w > WP_MAX_DIM) INSAR_FAIL(INSAR_E_SHAPE, "%s: output %d x %d outside 1..%d", who, h, w, WP_MAX_DIM);
  *blocks = (int64_t)n * ((h + WP_BY - 1) / WP_BY) * ((w + WP_BX - 1) / WP_BX);
  if (*blocks >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: %d outputs of %d x %d need 2^31 work-groups or more", who, n, h, w);
  return INSAR_OK;
}

template <typename S>
static void warp_raster_launch(int mode, dim3 grid, hipStream_t s, const void* src, int C, int H, int W, const int64_t* mats, int h, int w,
                               uint32_t fill_bits, void* dst, uint8_t* valid, bool vec, bool vec_valid) {
  S fill;
  if constexpr (sizeof(S) == 1) fill = (S)(fill_bits & 0xffu);
  else __builtin_memcpy(&fill, &fill_bits, 4);
  const dim3 block(WP_THREADS);
  if constexpr (std::is_same<S, int32_t>::value) {                  // int32: nearest only
    hipLaunchKernelGGL((warp_raster_kernel<S, INSAR_WARP_NEAREST>), grid, block, 0, s, (const S*)src, C, H, W, mats, h, w, fill, (S*)dst, valid, vec, vec_valid);
  } else {
    if (mode == INSAR_WARP_BILINEAR)
      hipLaunchKernelGGL((warp_raster_kernel<S, INSAR_WARP_BILINEAR>), grid, block, 0, s, (const S*)src, C, H, W, mats, h, w, fill, (S*)dst, valid, vec, vec_valid);
    else
      hipLaunchKernelGGL((warp_raster_kernel<S, INSAR_WARP_NEAREST>), grid, block, 0, s, (const S*)src, C, H, W, mats, h, w, fill, (S*)dst, valid, vec, vec_valid);
  }
}

extern "C" int insar_warp_raster(const void* src, int32_t dtype, int32_t C, int32_t H, int32_t W, const int64_t* matrices, int32_t n,
                                 int32_t h, int32_t w, int32_t mode, uint32_t fill_bits, void* dst, uint8_t* valid, void* stream) {
  const char* who = "insar_warp_raster";
  if (!src || !matrices || !dst) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !src ? "src" : !matrices ? "matrices" : "dst");
  if (dtype != INSAR_WARP_U8 && dtype != INSAR_WARP_I32 && dtype != INSAR_WARP_F32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: dtype %d (uint8, int32 or float32)", who, dtype);
  if (mode != INSAR_WARP_NEAREST && mode != INSAR_WARP_BILINEAR) INSAR_FAIL(INSAR_E_ARG, "%s: mode %d (nearest or bilinear)", who, mode);
  if (mode == INSAR_WARP_BILINEAR && dtype == INSAR_WARP_I32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: bilinear on int32 (label maps take nearest)", who);
  if (int rc = warp_check_source(who, C, H, W)) return rc;
  int64_t blocks;
  if (int rc = warp_blocks(who, n, h, w, &blocks)) return rc;
  const uintptr_t esz = dtype == INSAR_WARP_U8 ? 1 : 4;
  if ((((uintptr_t)src) | ((uintptr_t)dst)) & (esz - 1)) INSAR_FAIL(INSAR_E_ALIGN, "%s: src or dst not aligned to its element", who);
  if (((uintptr_t)matrices) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: matrices not 8-byte aligned", who);
  const bool vec = w % 4 == 0 && (((uintptr_t)dst) & (4 * esz - 1)) == 0;
  const bool vec_valid = w % 4 == 0 && (((uintptr_t)valid) & 3u) == 0;
  const dim3 grid((unsigned)blocks);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == INSAR_WARP_U8) warp_raster_launch<uint8_t>(mode, grid, s, src, C, H, W, matrices, h, w, fill_bits, dst, valid, vec, vec_valid);
  else if (dtype == INSAR_WARP_I32) warp_raster_launch<int32_t>(mode, grid, s, src, C, H, W, matrices, h, w, fill_bits, dst, valid, vec, vec_valid);
  else warp_raster_launch<float>(mode, grid, s, src, C, H, W, matrices, h, w, fill_bits, dst, valid, vec, vec_valid);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// insar_warp_gather: the warped counterpart of insar_crops_gather. One thread makes the image quad (bilinear, then the
// normalisation of image_quad of scene_common.h for a uint8 scene) and the label quad (nearest) of its four pixels from
// one set of positions. T % 4 == 0 and aligned outputs: every store is whole.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float warp_image(const uint8_t* __restrict__ p, const WarpTaps& t) {
  const float x = (float)warp_bilinear(p, t) / 255.0f;              // image_quad<uint8_t>: ToTensor + Normalize(0.5, 0.5)
  return (x - 0.5f) / 0.5f;
}
__device__ __forceinline__ float warp_image(const float* __restrict__ p, const WarpTaps& t) { return warp_bilinear(p, t); }

template <typename S, int MD>
__global__ void __launch_bounds__(WP_THREADS)
warp_gather_kernel(const S* __restrict__ scene, const uint8_t* __restrict__ labels, int H, int W, const int64_t* __restrict__ mats, int T,
                   float fill, float* __restrict__ images, void* __restrict__ masks) {
  WarpQuad q;
  if (!warp_quad(T, T, q)) return;
  const WarpMat m = warp_mat(mats + 6 * (int64_t)q.s);
  float f[4];
  uint32_t lab = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t sx = warp_pos(m.a, m.b, m.c, q.x + j, q.y), sy = warp_pos(m.d, m.e, m.f, q.x + j, q.y);
    const bool in = warp_inside(sx, sy, H, W);
    f[j] = fill;
    uint32_t l = 255u;
    if (in) {
      if (images) f[j] = warp_image(scene, warp_taps(sx, sy, H, W));
      if constexpr (MD != INSAR_AUG_MASK_NONE) l = labels[warp_nearest_at(sx, sy, W)];
    }
    lab |= l << (8 * j);
  }
  const int64_t o = ((int64_t)q.s * T + q.y) * T + q.x;
  if (images) *reinterpret_cast<float4*>(images + o) = make_float4(f[0], f[1], f[2], f[3]);
  if constexpr (MD == INSAR_AUG_MASK_U8) *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(masks) + o) = lab;
  else if constexpr (MD == INSAR_AUG_MASK_I64) labels4_store_i64(reinterpret_cast<int64_t*>(masks) + o, lab);
}

template <typename S>
static void warp_gather_launch(int md, dim3 grid, hipStream_t s, const void* scene, const uint8_t* labels, int H, int W, const int64_t* mats,
                               int T, float fill, float* images, void* masks) {
  const dim3 block(WP_THREADS);
  const S* sc = (const S*)scene;
  if (md == INSAR_AUG_MASK_U8)
    hipLaunchKernelGGL((warp_gather_kernel<S, INSAR_AUG_MASK_U8>), grid, block, 0, s, sc, labels, H, W, mats, T, fill, images, masks);
  else if (md == INSAR_AUG_MASK_I64)
    hipLaunchKernelGGL((warp_gather_kernel<S, INSAR_AUG_MASK_I64>), grid, block, 0, s, sc, labels, H, W, mats, T, fill, images, masks);
  else
    hipLaunchKernelGGL((warp_gather_kernel<S, INSAR_AUG_MASK_NONE>), grid, block, 0, s, sc, labels, H, W, mats, T, fill, images, masks);
}

extern "C" int insar_warp_gather(const void* scene, int32_t scene_dtype, const uint8_t* labels, int32_t H, int32_t W, const int64_t* matrices,
                                 int32_t n, int32_t T, float fill, float* images, void* masks, int32_t mask_dtype, void* stream) {
  const char* who = "insar_warp_gather";
  if (!matrices) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (matrices)", who);
  if (!images && !masks) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (neither images nor masks)", who);
  if (images && !scene) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (scene, with images asked for)", who);
  if (masks && !labels) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (labels, with masks asked for)", who);
  if (images && scene_dtype != INSAR_SCENE_U8 && scene_dtype != INSAR_SCENE_F32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: scene dtype %d (uint8 or float32)", who, scene_dtype);
  if (masks && mask_dtype != INSAR_AUG_MASK_U8 && mask_dtype != INSAR_AUG_MASK_I64)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: mask dtype %d (uint8 or int64)", who, mask_dtype);
  if (int rc = warp_check_source(who, 1, H, W)) return rc;
  if (T < 4 || T % 4) INSAR_FAIL(INSAR_E_SHAPE, "%s: tile %d is not a positive multiple of 4", who, T);
  int64_t blocks;
  if (int rc = warp_blocks(who, n, T, T, &blocks)) return rc;
  if (((uintptr_t)matrices) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: matrices not 8-byte aligned", who);
  if (images && !insar_aligned16(images)) INSAR_FAIL(INSAR_E_ALIGN, "%s: images not 16-byte aligned", who);
  if (images && scene_dtype == INSAR_SCENE_F32 && (((uintptr_t)scene) & 3u)) INSAR_FAIL(INSAR_E_ALIGN, "%s: float32 scene not 4-byte aligned", who);
  if (masks && (mask_dtype == INSAR_AUG_MASK_I64 ? !insar_aligned16(masks) : (((uintptr_t)masks) & 3u) != 0))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: masks not aligned (int64: 16 bytes, uint8: 4 bytes)", who);
  const int md = masks ? mask_dtype : INSAR_AUG_MASK_NONE;
  const dim3 grid((unsigned)blocks);
  hipStream_t s = (hipStream_t)stream;
  if (images && scene_dtype == INSAR_SCENE_F32) warp_gather_launch<float>(md, grid, s, scene, labels, H, W, matrices, T, fill, images, masks);
  else warp_gather_launch<uint8_t>(md, grid, s, scene, labels, H, W, matrices, T, fill, images, masks);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// insar_warp_draw: one thread per sample; the rule is stated in include/insar_hip.h
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t warp_q38(int64_t p) { return (p + 32) >> 6; }          // Q38 -> Q32, round half up
// the offset that keeps the tile centre (origin + (T - 1) / 2 in pixel indices) fixed: wrap-around like warp_pos
__device__ __forceinline__ int64_t warp_offset(int o, int T, int64_t p, int64_t q) {
  const int64_t half = (int64_t)((uint64_t)(p + q) * (uint64_t)(int64_t)(T - 1)) >> 1;
  return (int64_t)(((uint64_t)(2 * (int64_t)o + T - 1) << 31) - (uint64_t)half);
}

__global__ void __launch_bounds__(WP_THREADS)
warp_draw_kernel(uint64_t key, const int32_t* __restrict__ origins, int n, int T, int amax, int zoom_lo, int zoom_hi,
                 const int32_t* __restrict__ angles, int64_t* __restrict__ mats) {
  const int i = blockIdx.x * WP_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint64_t r = insar_hash64(key ^ WP_STREAM, (uint64_t)i);
  const int k = (int)(((r >> 32) * (uint64_t)(2 * amax + 1)) >> 32) - amax;
  const int64_t z = zoom_lo + (int64_t)(((r & 0xffffffffull) * (uint64_t)(zoom_hi - zoom_lo + 1)) >> 32);
  const int64_t cs = angles[2 * (k & (WP_ANGLES - 1))], sn = angles[2 * (k & (WP_ANGLES - 1)) + 1];
  const int64_t a = warp_q38(z * cs), b = warp_q38(-(z * sn)), d = warp_q38(z * sn);
  int64_t* m = mats + 6 * (int64_t)i;
  m[0] = a; m[1] = b; m[2] = warp_offset(origins[2 * i + 1], T, a, b);
  m[3] = d; m[4] = a; m[5] = warp_offset(origins[2 * i], T, d, a);
}

extern "C" int insar_warp_draw(uint64_t key, const int32_t* origins, int32_t n, int32_t T, int32_t amax, int32_t zoom_lo, int32_t zoom_hi,
                               const int32_t* angles, int64_t* matrices, void* stream) {
  const char* who = "insar_warp_draw";
  if (!origins || !angles || !matrices)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !origins ? "origins" : !angles ? "angles" : "matrices");
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: n = %d samples", who, n);
  if (T < 1 || T > WP_MAX_DIM) INSAR_FAIL(INSAR_E_SHAPE, "%s: tile %d outside 1..%d", who, T, WP_MAX_DIM);
  if (amax < 0 || amax > WP_ANGLES / 2) INSAR_FAIL(INSAR_E_ARG, "%s: amax %d outside 0..%d", who, amax, WP_ANGLES / 2);
  if (zoom_lo < 1 || zoom_hi < zoom_lo || zoom_hi > WP_MAX_ZOOM)
    INSAR_FAIL(INSAR_E_ARG, "%s: zoom %d..%d outside 1 <= lo <= hi <= %d (Q8)", who, zoom_lo, zoom_hi, WP_MAX_ZOOM);
  if ((((uintptr_t)origins) | ((uintptr_t)angles)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: origins or angles not 4-byte aligned", who);
  if (((uintptr_t)matrices) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: matrices not 8-byte aligned", who);
  hipLaunchKernelGGL(warp_draw_kernel, dim3((n + WP_THREADS - 1) / WP_THREADS), dim3(WP_THREADS), 0, (hipStream_t)stream, key, origins, n, T,
                     amax, zoom_lo, zoom_hi, angles, matrices);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// insar_multilook: one thread per four adjacent outputs of a row. Where the source rows allow (W % 4 == 0, an aligned source,
// a whole quad and fx in {1, 2, 4, 8}) the 4 fx source elements of a box row come as fx 16-byte (uint8: 4-byte) loads; the
// order of the float32 sum is the same on both paths: box rows top to bottom, each left to right, from +0.
// ---------------------------------------------------------------------------------------------
struct LookU8 {
  int sum;
  __device__ __forceinline__ void clear() { sum = 0; }
  __device__ __forceinline__ void add(int v) { sum += v; }
};
struct LookF32 {
  float sum;
  int cnt;
  __device__ __forceinline__ void clear() { sum = 0.f; cnt = 0; }
  __device__ __forceinline__ void add(float v) {
    if (v == v) { sum = sum + v; ++cnt; }
  }
};
__device__ __forceinline__ void look_load(const uint8_t* p, int64_t i, int* v) { quad_load_u8(p, i, 0, true, 0, v); }
__device__ __forceinline__ void look_load(const float* p, int64_t i, float* v) { quad_load(p, i, 0, true, 0.f, v); }

template <typename S, typename A, typename V, int FX>
__device__ __forceinline__ void look_rows_vec(const S* __restrict__ p, int64_t W, int fy, A* acc) {
  for (int r = 0; r < fy; ++r, p += W) {
#pragma unroll
    for (int g = 0; g < FX; ++g) {
      V t[4];
      look_load(p, 4 * g, t);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[(4 * g + k) / FX].add(t[k]);
    }
  }
}

template <typename S>
__global__ void __launch_bounds__(WP_THREADS)
multilook_kernel(const S* __restrict__ src, int C, int H, int W, int fy, int fx, int h, int w, int min_valid, S* __restrict__ dst,
                 int32_t* __restrict__ count, bool vec_src, bool vec_dst, bool vec_count) {
  constexpr bool F = sizeof(S) == 4;
  using A = typename std::conditional<F, LookF32, LookU8>::type;
  using V = typename std::conditional<F, float, int>::type;
  const int qrow = (w + 3) >> 2;
  const int64_t nwork = (int64_t)C * h * qrow;
  for (int64_t t = blockIdx.x * (int64_t)WP_THREADS + threadIdx.x; t < nwork; t += (int64_t)gridDim.x * WP_THREADS) {
    const int x = (int)(t % qrow) << 2;
    const int64_t r = t / qrow;
    const int y = (int)(r % h), c = (int)(r / h);
    const S* p = src + ((int64_t)c * H + (int64_t)y * fy) * W + (int64_t)x * fx;
    A acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j].clear();
    const bool whole = vec_src && x + 4 <= w;
    if (whole && fx == 1) look_rows_vec<S, A, V, 1>(p, W, fy, acc);
    else if (whole && fx == 2) look_rows_vec<S, A, V, 2>(p, W, fy, acc);
    else if (whole && fx == 4) look_rows_vec<S, A, V, 4>(p, W, fy, acc);
    else if (whole && fx == 8) look_rows_vec<S, A, V, 8>(p, W, fy, acc);
    else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x + j >= w) continue;                                    // (x + j + 1) fx <= w fx <= W: the box stays in its row
        for (int a = 0; a < fy; ++a)
          for (int b = 0; b < fx; ++b) acc[j].add((V)p[(int64_t)a * W + j * fx + b]);
      }
    }
    S v[4];
    int32_t cn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (F) {
        cn[j] = acc[j].cnt;
        const float mean = acc[j].sum / (float)acc[j].cnt;          // 0 / 0 = NaN where nothing is valid
        v[j] = acc[j].cnt >= min_valid ? warp_quiet(mean) : __int_as_float(0x7fc00000);
      } else {
        const int nb = fy * fx;
        cn[j] = nb;
        v[j] = (S)((acc[j].sum + nb / 2) / nb);
      }
    }
    const int64_t row = ((int64_t)c * h + y) * w;
    warp_store(dst + row, x, w, vec_dst, v);
    if (count) quad_store(count + row, x, w, vec_count, cn);
  }
}

extern "C" int insar_multilook(const void* src, int32_t dtype, int32_t C, int32_t H, int32_t W, int32_t fy, int32_t fx, int32_t min_valid,
                               void* dst, int32_t* count, void* stream) {
  const char* who = "insar_multilook";
  if (!src || !dst) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !src ? "src" : "dst");
  if (dtype != INSAR_WARP_U8 && dtype != INSAR_WARP_F32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: dtype %d (uint8 or float32; label maps take the nearest warp)", who, dtype);
  if (int rc = warp_check_source(who, C, H, W)) return rc;
  if (fy < 1 || fy > 16 || fx < 1 || fx > 16) INSAR_FAIL(INSAR_E_ARG, "%s: factors %d x %d outside 1..16", who, fy, fx);
  if (fy > H || fx > W) INSAR_FAIL(INSAR_E_SHAPE, "%s: factors %d x %d above the source %d x %d", who, fy, fx, H, W);
  if (min_valid < 1 || min_valid > fy * fx) INSAR_FAIL(INSAR_E_ARG, "%s: min_valid %d outside 1..%d", who, min_valid, fy * fx);
  const uintptr_t esz = dtype == INSAR_WARP_U8 ? 1 : 4;
  if ((((uintptr_t)src) | ((uintptr_t)dst)) & (esz - 1)) INSAR_FAIL(INSAR_E_ALIGN, "%s: src or dst not aligned to its element", who);
  if (((uintptr_t)count) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: count not 4-byte aligned", who);
  const int h = H / fy, w = W / fx;
  const bool vec_src = W % 4 == 0 && (((uintptr_t)src) & (4 * esz - 1)) == 0;
  const bool vec_dst = w % 4 == 0 && (((uintptr_t)dst) & (4 * esz - 1)) == 0;
  const bool vec_count = w % 4 == 0 && insar_aligned16(count);
  const int64_t nwork = (int64_t)C * h * ((w + 3) / 4);
  const dim3 grid(insar_grid_cap((nwork + WP_THREADS - 1) / WP_THREADS, 1 << 16)), block(WP_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == INSAR_WARP_U8)
    hipLaunchKernelGGL(multilook_kernel<uint8_t>, grid, block, 0, s, (const uint8_t*)src, C, H, W, fy, fx, h, w, min_valid, (uint8_t*)dst, count,
                       vec_src, vec_dst, vec_count);
  else
    hipLaunchKernelGGL(multilook_kernel<float>, grid, block, 0, s, (const float*)src, C, H, W, fy, fx, h, w, min_valid, (float*)dst, count,
                       vec_src, vec_dst, vec_count);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
