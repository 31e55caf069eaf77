// Training-time augmentation and test-time augmentation (TTA): the eight flips / rotations of the square (the dihedral
// group D4) applied to images and their masks together, a per-sample gain / bias and additive noise on the images.
// insar_aug_draw fills a per-sample parameter table on the device from a counter-based hash (insar_hash64 of scene_common.h,
// the aug_hash64 of include/insar_hip.h); insar_aug_apply carries it out. Both are pure functions of their arguments: no
// state, no atomics, bitwise reproducible.
//
// apply is an HBM-bound permutation. A work-group owns one 64 x 64 tile of one OUTPUT plane (an image channel or a mask)
// of one sample, so the op is uniform per work-group and no branch on it diverges.
//   non-transposing ops (0..3): no LDS. Where W % 4 == 0 and the pointers allow it a thread moves four adjacent pixels
//     with 16-byte accesses; a reversed row is reversed inside the quad and the quad order is reversed with it, so a wave
//     still reads and writes whole 256-byte runs of a row. Otherwise one pixel per lane, lanes along the row.
//   transposing ops (4..7): the source tile is read along ITS rows (lanes along the source row) into an LDS tile
//     [64][65] dwords and written along the OUTPUT rows from the transposed position. Row padding 65: the write
//     tile[r][lane] puts 64 consecutive dwords on banks (r + lane) % 32, the read tile[lane][r] puts stride-65 dwords on
//     banks (lane + r) % 32; in both, lanes l and l + 32 share a bank but sit in different 32-lane groups of
//     ds_write_b32 / ds_read_b32, which do not conflict. int64 masks use two such planes (low and high dword), so the
//     bank picture is the same for every element type.
#include <math.h>
#include "scene_common.h"

// the contract of this file is bitwise (tests/augment_ref.py restates it rounding for rounding)
#pragma clang fp contract(off)

#define AUG_THREADS 256
#define AUG_TILE 64
#define AUG_LDS_STRIDE 65
#define AUG_PLANE (AUG_TILE * AUG_LDS_STRIDE)
#define AUG_MAX_SIDE 32768
#define AUG_ZS 0x1.bb67aep-16f          // float32(1 / sqrt((65536^2 - 1) / 3)): the sum of four uniform 16-bit fields has this deviation

// ---------------------------------------------------------------------------------------------
// draw: one thread per sample, row s of the table = {op, gain, bias, sigma}
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float aug_uniform(uint32_t h) { return (float)(h >> 8) * 0x1p-24f; }

__global__ void __launch_bounds__(AUG_THREADS)
aug_draw_kernel(uint64_t key, int n, int ops_mask, float gain_lo, float gain_d, float bias_lo, float bias_d, float sigma_lo,
                float sigma_d, int32_t* __restrict__ table) {
  const int s = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (s >= n) return;
  uint32_t h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] = (uint32_t)(insar_hash64(key, 4ull * (uint64_t)s + j) >> 32);
  int k = (int)(h[0] % (uint32_t)__popc((unsigned)ops_mask));
  int op = 0;
  for (int b = 0; b < 8; ++b) {
    if ((ops_mask >> b) & 1) {
      if (k == 0) { op = b; break; }
      --k;
    }
  }
  float g = gain_d * aug_uniform(h[1]);
  g = gain_lo + g;
  float b = bias_d * aug_uniform(h[2]);
  b = bias_lo + b;
  float sg = sigma_d * aug_uniform(h[3]);
  sg = sigma_lo + sg;
  *reinterpret_cast<int4*>(table + 4 * s) = make_int4(op, __float_as_int(g), __float_as_int(b), __float_as_int(sg));
}

static bool aug_range_ok(float lo, float hi) { return isfinite(lo) && isfinite(hi) && lo <= hi; }

extern "C" int insar_aug_draw(uint64_t seed, uint64_t step, int32_t n, int32_t ops_mask, float gain_lo, float gain_hi,
                              float bias_lo, float bias_hi, float sigma_lo, float sigma_hi, int32_t* table, void* stream) {
  if (!table) INSAR_FAIL(INSAR_E_ARG, "insar_aug_draw: null table");
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_aug_draw: n = %d samples", n);
  if (ops_mask < 1 || ops_mask > 255) INSAR_FAIL(INSAR_E_ARG, "insar_aug_draw: ops_mask %d outside 1..255", ops_mask);
  if (!aug_range_ok(gain_lo, gain_hi)) INSAR_FAIL(INSAR_E_ARG, "insar_aug_draw: gain range [%g, %g] is empty or not finite", gain_lo, gain_hi);
  if (!aug_range_ok(bias_lo, bias_hi)) INSAR_FAIL(INSAR_E_ARG, "insar_aug_draw: bias range [%g, %g] is empty or not finite", bias_lo, bias_hi);
  if (!aug_range_ok(sigma_lo, sigma_hi)) INSAR_FAIL(INSAR_E_ARG, "insar_aug_draw: sigma range [%g, %g] is empty or not finite", sigma_lo, sigma_hi);
  if (sigma_lo < 0.f) INSAR_FAIL(INSAR_E_ARG, "insar_aug_draw: sigma_lo %g is negative", sigma_lo);
  if (!insar_aligned16(table)) INSAR_FAIL(INSAR_E_ALIGN, "insar_aug_draw: table not 16-byte aligned");
  const uint64_t key = seed ^ (step * 0xD1B54A32D192ED03ull);
  hipLaunchKernelGGL(aug_draw_kernel, dim3((n + AUG_THREADS - 1) / AUG_THREADS), dim3(AUG_THREADS), 0, (hipStream_t)stream, key,
                     n, ops_mask, gain_lo, gain_hi - gain_lo, bias_lo, bias_hi - bias_lo, sigma_lo, sigma_hi - sigma_lo, table);
  INSAR_CHECK_LAUNCH("insar_aug_draw");
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------------------------
struct AugArgs {
  const float* x;
  float* xo;
  const void* m;
  int64_t* mo;
  const int32_t* table;
  uint64_t noise_seed;
  int n, C, H, W, tiles_x, tiles_y;
  int xvec, mvec;          // 16-byte path allowed for the images / the masks
};

// t = gain * v; t = t + bias; t = t + sigma * z(lin): three separate roundings
struct AugPhoto {
  float gain, bias, sigma;
  uint64_t seed;
  bool noisy;
  __device__ __forceinline__ float operator()(float v, uint64_t lin) const {
    float t = gain * v;
    t = t + bias;
    if (noisy) {
      const uint64_t h = insar_hash64(seed, lin);
      const int S = (int)(h & 0xffffu) + (int)((h >> 16) & 0xffffu) + (int)((h >> 32) & 0xffffu) + (int)(h >> 48);
      const float z = (float)(S - 131070) * AUG_ZS;
      const float nz = sigma * z;
      t = t + nz;
    }
    return t;
  }
};

template <int MD> struct AugMask;
template <> struct AugMask<INSAR_AUG_MASK_U8> {
  typedef uint8_t T;
  __device__ __forceinline__ static int64_t widen(uint8_t v) { return (int64_t)v; }
  __device__ __forceinline__ static void quad(const uint8_t* p, int64_t* v) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (int64_t)((u >> (8 * j)) & 0xffu);
  }
};
template <> struct AugMask<INSAR_AUG_MASK_I64> {
  typedef int64_t T;
  __device__ __forceinline__ static int64_t widen(int64_t v) { return v; }
  __device__ __forceinline__ static void quad(const int64_t* p, int64_t* v) {
    const insar_i64x2 lo = *reinterpret_cast<const insar_i64x2*>(p);
    const insar_i64x2 hi = *reinterpret_cast<const insar_i64x2*>(p + 2);
    v[0] = lo.a; v[1] = lo.b; v[2] = hi.a; v[3] = hi.b;
  }
};

template <int MD>
__global__ void __launch_bounds__(AUG_THREADS) aug_apply_kernel(AugArgs a) {
  __shared__ uint32_t lds[(MD == INSAR_AUG_MASK_I64 ? 2 : 1) * AUG_PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int H = a.H, W = a.W;
  const int64_t plane = (int64_t)H * W;
  const int64_t tpp = (int64_t)a.tiles_y * a.tiles_x;
  const int64_t nimg = a.x ? (int64_t)a.n * a.C : 0;
  const int64_t nwork = (nimg + (MD != INSAR_AUG_MASK_NONE ? a.n : 0)) * tpp;
  for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    const int64_t p = w / tpp;
    const int t = (int)(w % tpp);
    const int i0 = (t / a.tiles_x) * AUG_TILE, j0 = (t % a.tiles_x) * AUG_TILE;      // origin of the OUTPUT tile
    const bool is_img = p < nimg;
    const int s = is_img ? (int)(p / a.C) : (int)(p - nimg);                          // < n either way
    const int32_t* row = a.table + 4 * (int64_t)s;
    int op = row[0] & 7;
    if (H != W) op &= 3;                       // a non-square plane has no transpose: whatever the table holds stays in bounds
    const bool tr = op & 4, fv = op & 2, fh = op & 1;
    if (is_img) {
      const float* __restrict__ src = a.x + p * plane;
      float* __restrict__ dst = a.xo + p * plane;
      AugPhoto f;
      f.gain = __int_as_float(row[1]); f.bias = __int_as_float(row[2]); f.sigma = __int_as_float(row[3]);
      f.seed = a.noise_seed; f.noisy = f.sigma != 0.f;
      const uint64_t lin0 = (uint64_t)p * (uint64_t)plane;                             // p = s * C + c
      if (tr) {
#pragma unroll 4
        for (int k = 0; k < AUG_TILE / 4; ++k) {
          const int r = wv + 4 * k;
          const int j = j0 + r, i = i0 + lane;                   // output column <- source row, output row <- source column
          if (j < W && i < H) {
            const int sj = fh ? W - 1 - j : j, si = fv ? H - 1 - i : i;
            lds[r * AUG_LDS_STRIDE + lane] = __float_as_uint(src[(int64_t)sj * W + si]);
          }
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < AUG_TILE / 4; ++k) {
          const int r = wv + 4 * k;
          const int i = i0 + r, j = j0 + lane;
          if (i < H && j < W) {
            const int64_t o = (int64_t)i * W + j;
            dst[o] = f(__uint_as_float(lds[lane * AUG_LDS_STRIDE + r]), lin0 + (uint64_t)o);
          }
        }
        __syncthreads();                                        // the tile is free for the next work item
      } else if (a.xvec) {
        const int qx = tid & 15;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + (tid >> 4) + 16 * k, j = j0 + 4 * qx;
          if (i < H && j < W) {                                  // W % 4 == 0: the quad lies whole in the row
            const int si = fv ? H - 1 - i : i, sj = fh ? W - 4 - j : j;
            const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)si * W + sj);
            float q[4] = {v.x, v.y, v.z, v.w};
            if (fh) { const float t0 = q[0], t1 = q[1]; q[0] = q[3]; q[1] = q[2]; q[2] = t1; q[3] = t0; }
            const int64_t o = (int64_t)i * W + j;
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = f(q[e], lin0 + (uint64_t)(o + e));
            *reinterpret_cast<float4*>(dst + o) = make_float4(q[0], q[1], q[2], q[3]);
          }
        }
      } else {
#pragma unroll 4
        for (int k = 0; k < AUG_TILE / 4; ++k) {
          const int i = i0 + wv + 4 * k, j = j0 + lane;
          if (i < H && j < W) {
            const int si = fv ? H - 1 - i : i, sj = fh ? W - 1 - j : j;
            const int64_t o = (int64_t)i * W + j;
            dst[o] = f(src[(int64_t)si * W + sj], lin0 + (uint64_t)o);
          }
        }
      }
    } else if constexpr (MD != INSAR_AUG_MASK_NONE) {
      typedef typename AugMask<MD>::T MT;
      const MT* __restrict__ src = reinterpret_cast<const MT*>(a.m) + (int64_t)s * plane;
      int64_t* __restrict__ dst = a.mo + (int64_t)s * plane;
      if (tr) {
#pragma unroll 4
        for (int k = 0; k < AUG_TILE / 4; ++k) {
          const int r = wv + 4 * k;
          const int j = j0 + r, i = i0 + lane;
          if (j < W && i < H) {
            const int sj = fh ? W - 1 - j : j, si = fv ? H - 1 - i : i;
            const uint64_t v = (uint64_t)AugMask<MD>::widen(src[(int64_t)sj * W + si]);
            lds[r * AUG_LDS_STRIDE + lane] = (uint32_t)v;
            if constexpr (MD == INSAR_AUG_MASK_I64) lds[AUG_PLANE + r * AUG_LDS_STRIDE + lane] = (uint32_t)(v >> 32);
          }
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < AUG_TILE / 4; ++k) {
          const int r = wv + 4 * k;
          const int i = i0 + r, j = j0 + lane;
          if (i < H && j < W) {
            uint64_t v = lds[lane * AUG_LDS_STRIDE + r];
            if constexpr (MD == INSAR_AUG_MASK_I64) v |= (uint64_t)lds[AUG_PLANE + lane * AUG_LDS_STRIDE + r] << 32;
            dst[(int64_t)i * W + j] = (int64_t)v;
          }
        }
        __syncthreads();
      } else if (a.mvec) {
        const int qx = tid & 15;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + (tid >> 4) + 16 * k, j = j0 + 4 * qx;
          if (i < H && j < W) {
            const int si = fv ? H - 1 - i : i, sj = fh ? W - 4 - j : j;
            int64_t q[4];
            AugMask<MD>::quad(src + (int64_t)si * W + sj, q);
            if (fh) { const int64_t t0 = q[0], t1 = q[1]; q[0] = q[3]; q[1] = q[2]; q[2] = t1; q[3] = t0; }
            quad_store_i64(dst + (int64_t)i * W + j, q);
          }
        }
      } else {
#pragma unroll 4
        for (int k = 0; k < AUG_TILE / 4; ++k) {
          const int i = i0 + wv + 4 * k, j = j0 + lane;
          if (i < H && j < W) {
            const int si = fv ? H - 1 - i : i, sj = fh ? W - 1 - j : j;
            dst[(int64_t)i * W + j] = AugMask<MD>::widen(src[(int64_t)si * W + sj]);
          }
        }
      }
    }
  }
}

extern "C" int insar_aug_apply(const float* x, float* xo, int32_t C, const void* m, int32_t m_dtype, int64_t* mo, int32_t n,
                               int32_t H, int32_t W, const int32_t* table, uint64_t noise_seed, void* stream) {
  if (!table) INSAR_FAIL(INSAR_E_ARG, "insar_aug_apply: null table");
  if ((x == nullptr) != (xo == nullptr)) INSAR_FAIL(INSAR_E_ARG, "insar_aug_apply: x and xo come together");
  if ((m == nullptr) != (mo == nullptr)) INSAR_FAIL(INSAR_E_ARG, "insar_aug_apply: m and mo come together");
  if (!x && !m) INSAR_FAIL(INSAR_E_ARG, "insar_aug_apply: neither images nor masks");
  if (m_dtype != INSAR_AUG_MASK_NONE && m_dtype != INSAR_AUG_MASK_U8 && m_dtype != INSAR_AUG_MASK_I64)
    INSAR_FAIL(INSAR_E_DTYPE, "insar_aug_apply: mask dtype %d (none, uint8 or int64)", m_dtype);
  if ((m != nullptr) != (m_dtype != INSAR_AUG_MASK_NONE))
    INSAR_FAIL(INSAR_E_ARG, "insar_aug_apply: mask pointers and m_dtype %d disagree", m_dtype);
  if (x && x == xo) INSAR_FAIL(INSAR_E_ARG, "insar_aug_apply: x == xo (not an in-place operation)");
  if (m && m == (const void*)mo) INSAR_FAIL(INSAR_E_ARG, "insar_aug_apply: m == mo (not an in-place operation)");
  if (n < 1 || H < 1 || W < 1 || (x && C < 1)) INSAR_FAIL(INSAR_E_SHAPE, "insar_aug_apply: n = %d, C = %d, H = %d, W = %d", n, C, H, W);
  if (H > AUG_MAX_SIDE || W > AUG_MAX_SIDE) INSAR_FAIL(INSAR_E_SHAPE, "insar_aug_apply: plane %d x %d above %d a side", H, W, AUG_MAX_SIDE);
  if ((((uintptr_t)x) | ((uintptr_t)xo) | ((uintptr_t)table)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "insar_aug_apply: x, xo or table not 4-byte aligned");
  if ((((uintptr_t)mo) & 7u) || (m_dtype == INSAR_AUG_MASK_I64 && (((uintptr_t)m) & 7u)))
    INSAR_FAIL(INSAR_E_ALIGN, "insar_aug_apply: int64 masks not 8-byte aligned");
  AugArgs a;
  a.x = x; a.xo = xo; a.m = m; a.mo = mo; a.table = table; a.noise_seed = noise_seed;
  a.n = n; a.C = x ? C : 0; a.H = H; a.W = W;
  a.tiles_x = (W + AUG_TILE - 1) / AUG_TILE;
  a.tiles_y = (H + AUG_TILE - 1) / AUG_TILE;
  a.xvec = x && W % 4 == 0 && insar_aligned16(x) && insar_aligned16(xo);
  a.mvec = m && W % 4 == 0 && insar_aligned16(mo) &&
           (m_dtype == INSAR_AUG_MASK_U8 ? ((((uintptr_t)m) & 3u) == 0) : insar_aligned16(m));
  const int64_t nwork = ((int64_t)n * a.C + (m ? n : 0)) * a.tiles_x * a.tiles_y;
  const dim3 grid(insar_grid_cap(nwork, 1 << 16)), block(AUG_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (m_dtype == INSAR_AUG_MASK_U8) hipLaunchKernelGGL(aug_apply_kernel<INSAR_AUG_MASK_U8>, grid, block, 0, s, a);
  else if (m_dtype == INSAR_AUG_MASK_I64) hipLaunchKernelGGL(aug_apply_kernel<INSAR_AUG_MASK_I64>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(aug_apply_kernel<INSAR_AUG_MASK_NONE>, grid, block, 0, s, a);
  INSAR_CHECK_LAUNCH("insar_aug_apply");
  return INSAR_OK;
}
