// Focal (neighbourhood) operations on a raster [planes][H][W] with the no-data rules of the scene tools: a NaN-aware separable
// smoothing in exact integers, min / max / lower-median rank filters and a slope (gradient) stencil. One launch per call, no
// atomics, no work-group waits on another, nothing read back; taps and scalars are kernel arguments.
//
// Validity (all three): a pixel is valid iff it lies inside the raster, its byte of `valid` (uint8 [H][W], shared by the planes,
// nullable) is non-zero, it does not equal `nodata` in the raster's own type and, in a float32 raster, it is finite.
//
//   smooth / min / max   focal_sep_kernel: one work-group of 256 threads per FC_TH x FC_TW output tile of one plane (planes on
//                        grid z). The tile and its R halo are staged ONCE in LDS as an int32 word (the quantised pixel with
//                        invalid pixels as 0; for min / max the order key with invalid pixels as the neutral key) and a
//                        validity byte; the row pass writes (A, Wr) for the FC_TH + 2R staged rows into LDS; the column pass
//                        reads them. Lanes run along x in every pass: the int32 reads of a 32-lane half are one contiguous
//                        128 bytes and the int64 reads of the column walk one contiguous 256 bytes (64 banks, each once), so
//                        neither pass has a bank conflict, whatever R makes of the row pitch.
//   median               focal_median_kernel<T, R>, R = 1..3: the same staging (static, at most 38 x 38); a thread takes the
//                        (2R + 1)^2 keys of its window into registers and finds element (n - 1) / 2 by bisection over the 32
//                        key bits (the largest probe with fewer than (n - 1) / 2 + 1 keys below it). Invalid pixels hold the
//                        key 0xffffffff, which is never below a probe.
//   gradient             focal_gradient_kernel: one thread per pixel, five loads; float32 operations in a fixed order, no
//                        contraction.
//
// Smoothing arithmetic (tests/focal_ref.py restates it): q by the rule of insar_zonal_accumulate; A = sum_i k[i] m q, Wr = sum_i
// k[i] m along the row; N = sum_j k[j] A, D = sum_j k[j] Wr down the column. |A| < 2^43, |N| < 2^55, D <= 2^24 since the taps sum to
// at most 4096. q_out = floor((2 N + D) / (2 D)): a FLOOR division, ties towards +infinity for both signs.
#include "scene_common.h"

#define FC_THREADS 256
#define FC_TH 32
#define FC_TW 32
#define FC_MAX_R 15
#define FC_MAX_SUM 4096
#define FC_MAX_MEDIAN_R 3
#define FC_MAX_PLANES 65535
#define FC_LIMIT 2147483647.0
#define FC_QNAN 0x7fc00000u

static_assert(FC_TW == 32 && FC_THREADS % FC_TW == 0, "a 32-lane half of a wave is one tile row");
static_assert(FC_TH * FC_TW % FC_THREADS == 0, "whole outputs per thread");

enum { FC_SMOOTH = 0, FC_MIN = 1, FC_MAX = 2 };

struct FocalTaps { int k[2 * FC_MAX_R + 1]; };

struct FocalArgs {
  const void* raster;
  const uint8_t* valid;
  void* out;
  uint8_t* out_valid;
  int H, W, R;
  int has_nodata, keep_invalid, fill;
  double scale, nodata;
  long long threshold;               // smooth: T on D; rank filters: min_count on n
};

// ---- per element type: validity of a value, the quantised pixel, the order key and its inverse, the stores -----------------
template <typename T> struct FcElem;
template <> struct FcElem<float> {
  __device__ __forceinline__ static bool ok(float v, bool has_nodata, double nodata) {
    return fabsf(v) <= 3.402823466e38f && !(has_nodata && v == (float)nodata);
  }
  __device__ __forceinline__ static int quantise(float v, double scale) {
    double d = (double)v * scale;
    d = d > FC_LIMIT ? FC_LIMIT : d < -FC_LIMIT ? -FC_LIMIT : d;
    return (int)rint(d);                                         // nearest even; |d| <= 2^31 - 1 fits
  }
  __device__ __forceinline__ static uint32_t key(float v) {      // hysteresis.ordered_u32
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
  }
  __device__ __forceinline__ static float from_key(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
  __device__ __forceinline__ static float from_q(long long q, double scale) { return (float)((double)q / scale); }
  __device__ __forceinline__ static float invalid(int) { return __uint_as_float(FC_QNAN); }
};
template <> struct FcElem<int> {
  __device__ __forceinline__ static bool ok(int v, bool has_nodata, double nodata) { return !(has_nodata && v == (int)nodata); }
  __device__ __forceinline__ static int quantise(int v, double) { return v; }
  __device__ __forceinline__ static uint32_t key(int v) { return (uint32_t)v ^ 0x80000000u; }
  __device__ __forceinline__ static int from_key(uint32_t k) { return (int)(k ^ 0x80000000u); }
  __device__ __forceinline__ static int from_q(long long q, double) { return (int)q; }
  __device__ __forceinline__ static int invalid(int fill) { return fill; }
};
template <> struct FcElem<uint8_t> {
  __device__ __forceinline__ static bool ok(uint8_t v, bool has_nodata, double nodata) { return !(has_nodata && (int)v == (int)nodata); }
  __device__ __forceinline__ static int quantise(uint8_t v, double) { return (int)v; }
  __device__ __forceinline__ static uint32_t key(uint8_t v) { return (uint32_t)v; }
  __device__ __forceinline__ static uint8_t from_key(uint32_t k) { return (uint8_t)k; }
  __device__ __forceinline__ static uint8_t from_q(long long q, double) { return (uint8_t)q; }
  __device__ __forceinline__ static uint8_t invalid(int fill) { return (uint8_t)fill; }
};

// floor(num / den) for |num| < 2^57, 1 <= den <= 2^25 and a quotient inside int32: the double quotient is off by at most one
// (a relative 2^-52 of at most 2^32), the products decide. C's `/` truncates, which is wrong below zero.
__device__ __forceinline__ long long fc_floor_div(long long num, long long den) {
  long long b = (long long)floor((double)num / (double)den);
  if (b * den > num) --b;
  else if ((b + 1) * den <= num) ++b;
  return b;
}

// the staged word and validity byte of pixel (gy, gx) of the plane at `src`; outside the raster is invalid
template <typename T, int OP>
__device__ __forceinline__ void fc_stage(const T* __restrict__ src, const FocalArgs& a, int gy, int gx, int* word, uint8_t* ok) {
  bool m = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
  T v = T();
  if (m) {
    const int64_t p = (int64_t)gy * a.W + gx;
    v = src[p];
    m = (!a.valid || a.valid[p] != 0) && FcElem<T>::ok(v, a.has_nodata != 0, a.nodata);
  }
  *ok = m ? 1 : 0;
  if (OP == FC_SMOOTH) *word = m ? FcElem<T>::quantise(v, a.scale) : 0;
  else if (OP == FC_MIN) *word = (int)(m ? FcElem<T>::key(v) : 0xffffffffu);
  else *word = (int)(m ? FcElem<T>::key(v) : 0u);
}

extern __shared__ __align__(16) unsigned char fc_lds[];

// bytes of fc_lds for radius R: rowv int64 [SH][TW], roww int32 [SH][TW], word int32 [SH][SW], taps int32 [32], ok uint8 [SH][SW]
static inline size_t fc_lds_bytes(int R) {
  const size_t SH = FC_TH + 2 * R, SW = FC_TW + 2 * R;
  return SH * FC_TW * 12 + SH * SW * 4 + 128 + ((SH * SW + 15) & ~(size_t)15);
}

template <typename T, int OP>
__global__ void __launch_bounds__(FC_THREADS)
focal_sep_kernel(FocalArgs a, FocalTaps taps, int tiles_x) {
  const int R = a.R, SH = FC_TH + 2 * R, SW = FC_TW + 2 * R, n_taps = 2 * R + 1;
  long long* rowv = reinterpret_cast<long long*>(fc_lds);
  int* roww = reinterpret_cast<int*>(rowv + SH * FC_TW);
  int* word = roww + SH * FC_TW;
  int* sk = word + SH * SW;
  uint8_t* ok = reinterpret_cast<uint8_t*>(sk + 32);
  const int tid = threadIdx.x;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int y0 = ty * FC_TH, x0 = tx * FC_TW;
  const int64_t plane = (int64_t)blockIdx.z * a.H * a.W;
  const T* src = reinterpret_cast<const T*>(a.raster) + plane;

  // constant indices into the by-value taps: scalar loads of the kernel arguments, no private copy
#pragma unroll
  for (int i = 0; i < 2 * FC_MAX_R + 1; ++i)
    if (tid == i) sk[i] = taps.k[i];
  for (int idx = tid; idx < SH * SW; idx += FC_THREADS) {
    const int sy = idx / SW, sx = idx - sy * SW;
    fc_stage<T, OP>(src, a, y0 - R + sy, x0 - R + sx, &word[idx], &ok[idx]);
  }
  __syncthreads();

  // ---- row pass: every staged row, the FC_TW output columns ----
  for (int idx = tid; idx < SH * FC_TW; idx += FC_THREADS) {
    const int r = idx / FC_TW, x = idx - r * FC_TW;
    const int* w = word + r * SW + x;
    const uint8_t* m = ok + r * SW + x;
    if (OP == FC_SMOOTH) {
      long long A = 0;
      int Wr = 0;
      for (int i = 0; i < n_taps; ++i) {
        const int k = sk[i];
        A += (long long)k * (long long)w[i];                     // invalid pixels were staged as 0
        Wr += k * (int)m[i];
      }
      rowv[idx] = A;
      roww[idx] = Wr;
    } else {
      uint32_t best = OP == FC_MIN ? 0xffffffffu : 0u;
      int n = 0;
      for (int i = 0; i < n_taps; ++i) {
        const uint32_t k = (uint32_t)w[i];
        best = OP == FC_MIN ? (k < best ? k : best) : (k > best ? k : best);
        n += (int)m[i];
      }
      rowv[idx] = (long long)best;
      roww[idx] = n;
    }
  }
  __syncthreads();

  // ---- column pass: FC_TH x FC_TW outputs, lanes along x ----
  T* out = reinterpret_cast<T*>(a.out) + plane;
  uint8_t* out_valid = a.out_valid ? a.out_valid + plane : nullptr;
  for (int o = tid; o < FC_TH * FC_TW; o += FC_THREADS) {
    const int y = o / FC_TW, x = o - y * FC_TW;
    const int gy = y0 + y, gx = x0 + x;
    if (gy >= a.H || gx >= a.W) continue;
    const long long* cv = rowv + y * FC_TW + x;
    const int* cw = roww + y * FC_TW + x;
    const bool centre = ok[(y + R) * SW + x + R] != 0;
    bool good;
    T res;
    if (OP == FC_SMOOTH) {
      long long N = 0, D = 0;
      for (int j = 0; j < n_taps; ++j) {
        const long long k = sk[j];
        N += k * cv[j * FC_TW];
        D += k * (long long)cw[j * FC_TW];
      }
      good = D >= a.threshold && (centre || !a.keep_invalid);      // threshold >= 1: D > 0 below
      res = good ? FcElem<T>::from_q(fc_floor_div(2 * N + D, 2 * D), a.scale) : FcElem<T>::invalid(a.fill);
    } else {
      uint32_t best = OP == FC_MIN ? 0xffffffffu : 0u;
      long long n = 0;
      for (int j = 0; j < n_taps; ++j) {
        const uint32_t k = (uint32_t)cv[j * FC_TW];
        best = OP == FC_MIN ? (k < best ? k : best) : (k > best ? k : best);
        n += cw[j * FC_TW];
      }
      good = n >= a.threshold && (centre || !a.keep_invalid);      // threshold >= 1: a valid key was seen
      res = good ? FcElem<T>::from_key(best) : FcElem<T>::invalid(a.fill);
    }
    const int64_t p = (int64_t)gy * a.W + gx;
    out[p] = res;
    if (out_valid) out_valid[p] = good ? 1 : 0;
  }
}

template <typename T, int R>
__global__ void __launch_bounds__(FC_THREADS)
focal_median_kernel(FocalArgs a, int tiles_x) {
  constexpr int SH = FC_TH + 2 * R, SW = FC_TW + 2 * R, NW = (2 * R + 1) * (2 * R + 1);
  __shared__ int word[SH * SW];
  __shared__ uint8_t ok[SH * SW];
  const int tid = threadIdx.x;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int y0 = ty * FC_TH, x0 = tx * FC_TW;
  const int64_t plane = (int64_t)blockIdx.z * a.H * a.W;
  const T* src = reinterpret_cast<const T*>(a.raster) + plane;
  for (int idx = tid; idx < SH * SW; idx += FC_THREADS) {
    const int sy = idx / SW, sx = idx - sy * SW;
    fc_stage<T, FC_MIN>(src, a, y0 - R + sy, x0 - R + sx, &word[idx], &ok[idx]);       // invalid: key 0xffffffff
  }
  __syncthreads();
  T* out = reinterpret_cast<T*>(a.out) + plane;
  uint8_t* out_valid = a.out_valid ? a.out_valid + plane : nullptr;
  for (int o = tid; o < FC_TH * FC_TW; o += FC_THREADS) {
    const int y = o / FC_TW, x = o - y * FC_TW;
    const int gy = y0 + y, gx = x0 + x;
    if (gy >= a.H || gx >= a.W) continue;
    uint32_t keys[NW];
    int n = 0;
#pragma unroll
    for (int j = 0; j < 2 * R + 1; ++j)
#pragma unroll
      for (int i = 0; i < 2 * R + 1; ++i) {
        keys[j * (2 * R + 1) + i] = (uint32_t)word[(y + j) * SW + x + i];
        n += (int)ok[(y + j) * SW + x + i];
      }
    const bool good = n >= a.threshold && (ok[(y + R) * SW + x + R] != 0 || !a.keep_invalid);
    T res = FcElem<T>::invalid(a.fill);
    if (good) {                                                  // threshold >= 1: n >= 1
      const int rank = (n - 1) >> 1;                             // the LOWER median
      uint32_t ans = 0u;
      for (int bit = 31; bit >= 0; --bit) {
        const uint32_t probe = ans | (1u << bit);
        int below = 0;
#pragma unroll
        for (int t = 0; t < NW; ++t) below += keys[t] < probe;
        if (below <= rank) ans = probe;                          // the largest probe with at most `rank` keys below it
      }
      res = FcElem<T>::from_key(ans);
    }
    const int64_t p = (int64_t)gy * a.W + gx;
    out[p] = res;
    if (out_valid) out_valid[p] = good ? 1 : 0;
  }
}

struct FocalGradArgs {
  const float* raster;
  const uint8_t* valid;
  float* out;
  uint8_t* out_valid;
  int H, W;
  int has_nodata, keep_invalid;
  double nodata;
  float hy1, hy2, hx1, hx2;
};

// one component: vm, v0, vp are the pixels at -1, 0, +1 along the axis
__device__ __forceinline__ float fc_slope(bool mm, bool m0, bool mp, float vm, float v0, float vp, float h1, float h2, bool keep_invalid,
                                          bool* good) {
#pragma clang fp contract(off)
  *good = true;
  if (!(keep_invalid && !m0)) {
    if (mm && mp) return (vp - vm) * h2;
    if (m0 && mp) return (vp - v0) * h1;
    if (m0 && mm) return (v0 - vm) * h1;
  }
  *good = false;
  return __uint_as_float(FC_QNAN);
}

__global__ void __launch_bounds__(FC_THREADS)
focal_gradient_kernel(FocalGradArgs a) {
  const int64_t npix = (int64_t)a.H * a.W;
  const int64_t p = (int64_t)blockIdx.x * FC_THREADS + threadIdx.x;
  if (p >= npix) return;
  const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
  const float* src = a.raster + (int64_t)blockIdx.z * npix;
  const bool nd = a.has_nodata != 0;
  auto look = [&](int yy, int xx, float* v) -> bool {
    if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) { *v = 0.0f; return false; }
    const int64_t q = (int64_t)yy * a.W + xx;
    *v = src[q];
    return (!a.valid || a.valid[q] != 0) && FcElem<float>::ok(*v, nd, a.nodata);
  };
  float v0, vu, vd, vl, vr;
  const bool m0 = look(y, x, &v0), mu = look(y - 1, x, &vu), md = look(y + 1, x, &vd), ml = look(y, x - 1, &vl), mr = look(y, x + 1, &vr);
  bool gy_ok, gx_ok;
  const float gy = fc_slope(mu, m0, md, vu, v0, vd, a.hy1, a.hy2, a.keep_invalid != 0, &gy_ok);
  const float gx = fc_slope(ml, m0, mr, vl, v0, vr, a.hx1, a.hx2, a.keep_invalid != 0, &gx_ok);
  float* out = a.out + (int64_t)blockIdx.z * 2 * npix;
  out[p] = gy;
  out[npix + p] = gx;
  if (a.out_valid) a.out_valid[(int64_t)blockIdx.z * npix + p] = (gy_ok && gx_ok) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int focal_check_map(const char* who, const void* raster, int32_t elem_type, int32_t planes, int32_t H, int32_t W, int32_t has_nodata,
                           double nodata, const void* out) {
  if (!raster || !out) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !raster ? "raster" : "out");
  if (raster == out) INSAR_FAIL(INSAR_E_ARG, "%s: out is the raster itself (a neighbourhood is read after its centre is written)", who);
  if (elem_type != INSAR_ZONAL_F32 && elem_type != INSAR_ZONAL_U8 && elem_type != INSAR_ZONAL_I32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: element type %d", who, elem_type);
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty raster %d x %d", who, H, W);
  if ((int64_t)H * W >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: raster %d x %d has 2^31 pixels or more", who, H, W);
  if (planes < 1 || planes > FC_MAX_PLANES) INSAR_FAIL(INSAR_E_SHAPE, "%s: planes %d outside 1..%d", who, planes, FC_MAX_PLANES);
  if (elem_type != INSAR_ZONAL_U8 && ((((uintptr_t)raster) & 3u) || (((uintptr_t)out) & 3u)))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: raster / out not 4-byte aligned", who);
  if (has_nodata && nodata != nodata) INSAR_FAIL(INSAR_E_ARG, "%s: nodata is NaN", who);
  if (has_nodata && elem_type != INSAR_ZONAL_F32 && (nodata != (double)(int64_t)nodata || nodata < -2147483648.0 || nodata > 2147483647.0))
    INSAR_FAIL(INSAR_E_ARG, "%s: nodata %g is no value of an integer raster", who, nodata);
  return INSAR_OK;
}
static int focal_check_fill(const char* who, int32_t elem_type, int32_t fill) {
  if (elem_type == INSAR_ZONAL_U8 && (fill < 0 || fill > 255)) INSAR_FAIL(INSAR_E_ARG, "%s: fill %d is no uint8 value", who, fill);
  return INSAR_OK;
}
static inline int64_t focal_tiles(int32_t H, int32_t W, int* tiles_x) {
  *tiles_x = (W + FC_TW - 1) / FC_TW;
  return (int64_t)*tiles_x * ((H + FC_TH - 1) / FC_TH);       // < 2^31: H * W < 2^31 and a tile has 1024 pixels
}

extern "C" int insar_focal_tile(int32_t radius, int32_t* rows, int32_t* cols) {
  const char* who = "insar_focal_tile";
  if (!rows || !cols) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (radius < 0 || radius > FC_MAX_R) INSAR_FAIL(INSAR_E_SHAPE, "%s: radius %d outside 0..%d", who, radius, FC_MAX_R);
  *rows = FC_TH;
  *cols = FC_TW;
  return INSAR_OK;
}

template <int OP>
static void focal_launch_sep(int32_t elem_type, const FocalArgs& a, const FocalTaps& t, int32_t planes, hipStream_t stream) {
  int tiles_x;
  const dim3 grid((unsigned)focal_tiles(a.H, a.W, &tiles_x), 1, (unsigned)planes), block(FC_THREADS);
  const size_t lds = fc_lds_bytes(a.R);                          // at most 43168 bytes: below the 64 KiB that need no attribute
  if (elem_type == INSAR_ZONAL_F32) hipLaunchKernelGGL((focal_sep_kernel<float, OP>), grid, block, lds, stream, a, t, tiles_x);
  else if (elem_type == INSAR_ZONAL_U8) hipLaunchKernelGGL((focal_sep_kernel<uint8_t, OP>), grid, block, lds, stream, a, t, tiles_x);
  else hipLaunchKernelGGL((focal_sep_kernel<int, OP>), grid, block, lds, stream, a, t, tiles_x);
}

extern "C" int insar_focal_smooth(const void* raster, int32_t elem_type, int32_t planes, int32_t H, int32_t W, const int32_t* taps,
                                  int32_t radius, double scale, int32_t has_nodata, double nodata, const uint8_t* valid,
                                  int64_t threshold, int32_t keep_invalid, int32_t fill, void* out, uint8_t* out_valid, void* stream) {
  const char* who = "insar_focal_smooth";
  if (int rc = focal_check_map(who, raster, elem_type, planes, H, W, has_nodata, nodata, out)) return rc;
  if (int rc = focal_check_fill(who, elem_type, fill)) return rc;
  if (!taps) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (taps)", who);
  if (radius < 0 || radius > FC_MAX_R) INSAR_FAIL(INSAR_E_SHAPE, "%s: radius %d outside 0..%d", who, radius, FC_MAX_R);
  FocalTaps t;
  int64_t sum = 0;
  for (int i = 0; i < 2 * FC_MAX_R + 1; ++i) {
    t.k[i] = i <= 2 * radius ? taps[i] : 0;
    if (t.k[i] < 0) INSAR_FAIL(INSAR_E_ARG, "%s: tap %d is negative (%d)", who, i, t.k[i]);
    sum += t.k[i];
  }
  if (sum < 1 || sum > FC_MAX_SUM) INSAR_FAIL(INSAR_E_ARG, "%s: the taps sum to %lld, outside 1..%d", who, (long long)sum, FC_MAX_SUM);
  if (threshold < 1 || threshold > sum * sum)
    INSAR_FAIL(INSAR_E_ARG, "%s: threshold %lld outside 1..%lld", who, (long long)threshold, (long long)(sum * sum));
  if (!(scale > 0.0) || !(scale <= 1.7976931348623157e308)) INSAR_FAIL(INSAR_E_ARG, "%s: scale %g: positive and finite", who, scale);
  FocalArgs a;
  a.raster = raster; a.valid = valid; a.out = out; a.out_valid = out_valid;
  a.H = H; a.W = W; a.R = radius;
  a.has_nodata = has_nodata; a.keep_invalid = keep_invalid != 0; a.fill = fill;
  a.scale = scale; a.nodata = nodata; a.threshold = threshold;
  focal_launch_sep<FC_SMOOTH>(elem_type, a, t, planes, (hipStream_t)stream);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

template <int R>
static void focal_launch_median(int32_t elem_type, const FocalArgs& a, int32_t planes, hipStream_t stream) {
  int tiles_x;
  const dim3 grid((unsigned)focal_tiles(a.H, a.W, &tiles_x), 1, (unsigned)planes), block(FC_THREADS);
  if (elem_type == INSAR_ZONAL_F32) hipLaunchKernelGGL((focal_median_kernel<float, R>), grid, block, 0, stream, a, tiles_x);
  else if (elem_type == INSAR_ZONAL_U8) hipLaunchKernelGGL((focal_median_kernel<uint8_t, R>), grid, block, 0, stream, a, tiles_x);
  else hipLaunchKernelGGL((focal_median_kernel<int, R>), grid, block, 0, stream, a, tiles_x);
}

extern "C" int insar_focal_rank(const void* raster, int32_t elem_type, int32_t planes, int32_t H, int32_t W, int32_t op, int32_t radius,
                                int32_t has_nodata, double nodata, const uint8_t* valid, int32_t min_count, int32_t keep_invalid,
                                int32_t fill, void* out, uint8_t* out_valid, void* stream) {
  const char* who = "insar_focal_rank";
  if (int rc = focal_check_map(who, raster, elem_type, planes, H, W, has_nodata, nodata, out)) return rc;
  if (int rc = focal_check_fill(who, elem_type, fill)) return rc;
  if (op != INSAR_FOCAL_MIN && op != INSAR_FOCAL_MAX && op != INSAR_FOCAL_MEDIAN) INSAR_FAIL(INSAR_E_ARG, "%s: op %d", who, op);
  const int rmax = op == INSAR_FOCAL_MEDIAN ? FC_MAX_MEDIAN_R : FC_MAX_R;
  if (radius < 1 || radius > rmax) INSAR_FAIL(INSAR_E_SHAPE, "%s: radius %d outside 1..%d", who, radius, rmax);
  const int window = (2 * radius + 1) * (2 * radius + 1);
  if (min_count < 1 || min_count > window) INSAR_FAIL(INSAR_E_ARG, "%s: min_count %d outside 1..%d", who, min_count, window);
  FocalArgs a;
  a.raster = raster; a.valid = valid; a.out = out; a.out_valid = out_valid;
  a.H = H; a.W = W; a.R = radius;
  a.has_nodata = has_nodata; a.keep_invalid = keep_invalid != 0; a.fill = fill;
  a.scale = 1.0; a.nodata = nodata; a.threshold = min_count;
  FocalTaps t = {};
  if (op == INSAR_FOCAL_MIN) focal_launch_sep<FC_MIN>(elem_type, a, t, planes, (hipStream_t)stream);
  else if (op == INSAR_FOCAL_MAX) focal_launch_sep<FC_MAX>(elem_type, a, t, planes, (hipStream_t)stream);
  else if (radius == 1) focal_launch_median<1>(elem_type, a, planes, (hipStream_t)stream);
  else if (radius == 2) focal_launch_median<2>(elem_type, a, planes, (hipStream_t)stream);
  else focal_launch_median<3>(elem_type, a, planes, (hipStream_t)stream);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_focal_gradient(const float* raster, int32_t planes, int32_t H, int32_t W, float hy1, float hy2, float hx1, float hx2,
                                    int32_t has_nodata, double nodata, const uint8_t* valid, int32_t keep_invalid, float* out,
                                    uint8_t* out_valid, void* stream) {
  const char* who = "insar_focal_gradient";
  if (int rc = focal_check_map(who, raster, INSAR_ZONAL_F32, planes, H, W, has_nodata, nodata, out)) return rc;
  const float h[4] = {hy1, hy2, hx1, hx2};
  for (int i = 0; i < 4; ++i)
    if (!(h[i] > 0.0f) || !(h[i] <= 3.402823466e38f)) INSAR_FAIL(INSAR_E_ARG, "%s: reciprocal spacing %g: positive and finite", who, (double)h[i]);
  FocalGradArgs a;
  a.raster = raster; a.valid = valid; a.out = out; a.out_valid = out_valid;
  a.H = H; a.W = W;
  a.has_nodata = has_nodata; a.keep_invalid = keep_invalid != 0;
  a.nodata = nodata;
  a.hy1 = hy1; a.hy2 = hy2; a.hx1 = hx1; a.hx2 = hx2;
  const int64_t blocks = ((int64_t)H * W + FC_THREADS - 1) / FC_THREADS;      // < 2^23
  hipLaunchKernelGGL(focal_gradient_kernel, dim3((unsigned)blocks, 1, (unsigned)planes), dim3(FC_THREADS), 0, (hipStream_t)stream, a);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
