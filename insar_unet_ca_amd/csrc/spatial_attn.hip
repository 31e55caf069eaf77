// SpatialAttention of the SA U-Net (Unet-SpatialAttention.py:59-82), applied to each skip-concat (:131,137,143,149):
//     a   = cat(mean_c x, max_c x)                       B x 2 x H x W
//     z   = ReLU(BN2(conv1x1ch(ReLU(BN1(conv2to1(a))))))  DoubleConv(2, 1), 3x3 stencils with bias
//     out = x * sigmoid(z)                               broadcast over C
// Forward : insar_sa_compress -> insar_sa_conv(1) -> insar_bn_finalize(BN1, C = 1) -> insar_sa_conv(2)
//           -> insar_bn_finalize(BN2) -> insar_sa_gate
// Backward: insar_sa_dscale -> insar_sa_bwd_coef(2) -> insar_sa_bwd_stencil(2) -> insar_sa_bwd_coef(1)
//           -> insar_sa_bwd_stencil(1) -> insar_sa_bwd_coef(0) -> insar_sa_dx (in place over the output gradient)
// The C-channel passes (compress, gate, dscale, dx) are HBM-bound: 16-byte loads, a group of L lanes per pixel.
// The 1-channel stencil passes work on fp32 maps [B][H][W] (the compressed map has a zero halo). Every reduction
// is a fixed partition (work-group w owns image rows w, w + rows, ...) folded in a fixed order: bitwise reproducible.
#include "common.h"

#define SA_THREADS 256
#define SA_PART_COLS 20   // row stride of d.part (backward partial sums)

__device__ __forceinline__ float sa_sigmoid(float v) { return 1.f / (1.f + __expf(-v)); }

template <typename T>
__device__ __forceinline__ const uint4* sa_chunk(const ActView& v, int n, int h, int w) {
  return (const uint4*)(v.base + v.elem_offset(n, h, w) * (int64_t)sizeof(T));
}

// Sum N per-thread values over the work-group (fixed order: butterfly inside each wave, then the waves in order);
// thread 0 writes out[0..N).
template <int N>
__device__ __forceinline__ void sa_block_sum(float (&v)[N], float* out) {
  __shared__ float red[SA_THREADS / 64][N];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float t = wave_sum(v[k]);
    if (lane == 0) red[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      float t = 0.f;
      for (int q = 0; q < SA_THREADS / 64; ++q) t += red[q][k];
      out[k] = t;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int64_t sa_pix(int n, int h, int w, int H, int W) { return ((int64_t)n * H + h) * W + w; }
__device__ __forceinline__ int64_t sa_comp(int n, int h, int w, int H, int W) {   // padded [B][H+2][W+2] pixel
  return ((int64_t)n * (H + 2) + h + 1) * (W + 2) + w + 1;
}

// ---- compress: mean and first arg-max over the channels of each pixel -------------------------------------------
template <typename T, int L>
__global__ void __launch_bounds__(SA_THREADS) sa_compress_kernel(ActView x, float* __restrict__ comp, uint16_t* __restrict__ arg) {
  constexpr int CH = Chunk<T>::N;
  const int nch = x.c_len / CH;
  const int lane = threadIdx.x % L, grp = threadIdx.x / L;
  constexpr int NG = SA_THREADS / L;
  const int rows = x.B * x.H;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const int n = r / x.H, h = r - n * x.H;
    for (int w0 = 0; w0 < x.W; w0 += NG) {
      const int w = w0 + grp;
      float s = 0.f, m = -INFINITY;
      int a = 0x7fffffff;
      if (w < x.W) {
        const uint4* p = sa_chunk<T>(x, n, h, w);
#pragma unroll 4
        for (int j = lane; j < nch; j += L) {
          float f[CH];
          Chunk<T>::unpack(p[j], f);
#pragma unroll
          for (int k = 0; k < CH; ++k) {
            s += f[k];
            if (f[k] > m || a == 0x7fffffff) { m = f[k]; a = j * CH + k; }   // strictly greater: the first index stays
          }
        }
      }
#pragma unroll
      for (int o = L / 2; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        const float m2 = __shfl_xor(m, o, 64);
        const int a2 = __shfl_xor(a, o, 64);
        if (a2 != 0x7fffffff && (a == 0x7fffffff || m2 > m || (m2 == m && a2 < a))) { m = m2; a = a2; }
      }
      if (w < x.W && lane == 0) {
        *(float2*)(comp + 2 * sa_comp(n, h, w, x.H, x.W)) = make_float2(s / (float)x.c_len, m);
        arg[sa_pix(n, h, w, x.H, x.W)] = (uint16_t)a;
      }
    }
  }
}

// ---- forward stencils: z1 = conv(comp, w1) (2 -> 1), z2 = conv(ReLU(BN1(z1)), w2) (1 -> 1), no bias ----------------
// stat[blk][2] = (sum z, sum z^2) of the work-group's rows (insar_bn_finalize folds them, C = 1).
template <int WHICH>
__global__ void __launch_bounds__(SA_THREADS) sa_conv_kernel(InsarSa d) {
  const int B = d.x.B, H = d.x.H, W = d.x.W;
  float wt[18];
#pragma unroll
  for (int k = 0; k < (WHICH == 1 ? 18 : 9); ++k) wt[k] = WHICH == 1 ? d.w1[k] : d.w2[k];
  const float sc1 = WHICH == 2 ? d.bn[0] : 0.f, sh1 = WHICH == 2 ? d.bn[1] : 0.f;
  float acc[2] = {0.f, 0.f};
  for (int r = blockIdx.x; r < B * H; r += gridDim.x) {
    const int n = r / H, h = r - n * H;
    for (int w = threadIdx.x; w < W; w += SA_THREADS) {
      float z = 0.f;
      if (WHICH == 1) {
        const float2* c = (const float2*)d.comp;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float2 v = c[sa_comp(n, h + ky - 1, w + kx - 1, H, W)];   // zero halo: no branches
            z = fmaf(wt[ky * 3 + kx], v.x, z);
            z = fmaf(wt[9 + ky * 3 + kx], v.y, z);
          }
        d.z1[sa_pix(n, h, w, H, W)] = z;
      } else {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int hh = h + ky - 1, ww = w + kx - 1;
            if (hh >= 0 && hh < H && ww >= 0 && ww < W)
              z = fmaf(wt[ky * 3 + kx], fmaxf(fmaf(d.z1[sa_pix(n, hh, ww, H, W)], sc1, sh1), 0.f), z);
          }
        d.z2[sa_pix(n, h, w, H, W)] = z;
      }
      acc[0] += z;
      acc[1] = fmaf(z, z, acc[1]);
    }
  }
  if (d.training) sa_block_sum<2>(acc, (WHICH == 1 ? d.stat1 : d.stat2) + 2 * blockIdx.x);
}

// ---- gate: s = sigmoid(ReLU(BN2(z2))) (fp32 map), out = x * s -------------------------------------------------------
#define SA_EW_UNROLL 4
template <typename T>
__global__ void __launch_bounds__(SA_THREADS) sa_gate_kernel(ActView x, ActView y, InsarSa d) {
  constexpr int CH = Chunk<T>::N;
  const int nch = x.c_len / CH, H = x.H, W = x.W;
  const float sc2 = d.bn[4], sh2 = d.bn[5];
  const int items = W * nch;
  for (int r = blockIdx.x; r < x.B * H; r += gridDim.x) {
    const int n = r / H, h = r - n * H;
    for (int t0 = threadIdx.x; t0 < items; t0 += SA_EW_UNROLL * SA_THREADS) {
      uint4 v[SA_EW_UNROLL];
      float sv[SA_EW_UNROLL];
#pragma unroll
      for (int u = 0; u < SA_EW_UNROLL; ++u) {
        const int t = t0 + u * SA_THREADS;
        if (t < items) {
          const int w = t / nch, cc = t - w * nch;
          v[u] = sa_chunk<T>(x, n, h, w)[cc];
          const int64_t p = sa_pix(n, h, w, H, W);
          sv[u] = sa_sigmoid(fmaxf(fmaf(d.z2[p], sc2, sh2), 0.f));
          if (cc == 0) d.s[p] = sv[u];
        }
      }
#pragma unroll
      for (int u = 0; u < SA_EW_UNROLL; ++u) {
        const int t = t0 + u * SA_THREADS;
        if (t < items) {
          const int w = t / nch, cc = t - w * nch;
          float f[CH];
          Chunk<T>::unpack(v[u], f);
#pragma unroll
          for (int k = 0; k < CH; ++k) f[k] *= sv[u];
          ((uint4*)(y.base + y.elem_offset(n, h, w) * (int64_t)sizeof(T)))[cc] = Chunk<T>::pack(f);
        }
      }
    }
  }
}

// ---- dscale: g2 = d(loss)/d(BN2 output) = (sum_c dy * x) * s (1 - s) * [BN2(z2) > 0]; part[blk] = (sum g2, sum g2 xhat2) --
template <typename T, int L>
__global__ void __launch_bounds__(SA_THREADS) sa_dscale_kernel(ActView x, ActView dy, InsarSa d) {
  constexpr int CH = Chunk<T>::N;
  const int nch = x.c_len / CH, H = x.H, W = x.W;
  const int lane = threadIdx.x % L, grp = threadIdx.x / L;
  constexpr int NG = SA_THREADS / L;
  const float sc2 = d.bn[4], sh2 = d.bn[5], mean2 = d.bn[6], inv2 = d.bn[7];
  float acc[2] = {0.f, 0.f};
  for (int r = blockIdx.x; r < x.B * H; r += gridDim.x) {
    const int n = r / H, h = r - n * H;
    for (int w0 = 0; w0 < W; w0 += NG) {
      const int w = w0 + grp;
      float s = 0.f;
      if (w < W) {
        const uint4* px = sa_chunk<T>(x, n, h, w);
        const uint4* pd = sa_chunk<T>(dy, n, h, w);
#pragma unroll 4
        for (int j = lane; j < nch; j += L) {
          float fx[CH], fd[CH];
          Chunk<T>::unpack(px[j], fx);
          Chunk<T>::unpack(pd[j], fd);
#pragma unroll
          for (int k = 0; k < CH; ++k) s = fmaf(fd[k], fx[k], s);
        }
      }
#pragma unroll
      for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (w < W && lane == 0) {
        const int64_t p = sa_pix(n, h, w, H, W);
        const float z = d.z2[p], sg = d.s[p];
        const float g = fmaf(z, sc2, sh2) > 0.f ? s * sg * (1.f - sg) : 0.f;
        d.g2[p] = g;
        acc[0] += g;
        acc[1] = fmaf(g, (z - mean2) * inv2, acc[1]);
      }
    }
  }
  sa_block_sum<2>(acc, d.part + SA_PART_COLS * blockIdx.x);
}

// ---- backward stencils --------------------------------------------------------------------------------------------
// WHICH = 2: dz2 = BN2 backward of g2 (on load); g1 = (conv^T(dz2, w2)) * [BN1(z1) > 0];
//            part[blk] = (sum g1, sum g1 xhat1, dw2[9], db2)
// WHICH = 1: dz1 = BN1 backward of g1 (on load); dcomp = conv^T(dz1, w1) (d mean, d max);
//            part[blk] = (dw1[2][9], db1)
template <int WHICH>
__global__ void __launch_bounds__(SA_THREADS) sa_bwd_stencil_kernel(InsarSa d) {
  constexpr int NP = WHICH == 2 ? 12 : 19;
  const int B = d.x.B, H = d.x.H, W = d.x.W;
  float wt[18];
#pragma unroll
  for (int k = 0; k < (WHICH == 1 ? 18 : 9); ++k) wt[k] = WHICH == 1 ? d.w1[k] : d.w2[k];
  // BatchNorm backward of the unit whose output gradient is read: dz = scale * (g - k1 - xhat * k2)
  const float sc = WHICH == 2 ? d.bn[4] : d.bn[0], mu = WHICH == 2 ? d.bn[6] : d.bn[2], inv = WHICH == 2 ? d.bn[7] : d.bn[3];
  const float k1 = WHICH == 2 ? d.coef[0] : d.coef[2], k2 = WHICH == 2 ? d.coef[1] : d.coef[3];
  const float* g = WHICH == 2 ? d.g2 : d.g1;
  const float* z = WHICH == 2 ? d.z2 : d.z1;
  const float sc1 = d.bn[0], sh1 = d.bn[1], mean1 = d.bn[2], inv1 = d.bn[3];
  float acc[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) acc[k] = 0.f;
  for (int r = blockIdx.x; r < B * H; r += gridDim.x) {
    const int n = r / H, h = r - n * H;
    for (int w = threadIdx.x; w < W; w += SA_THREADS) {
      const int64_t q = sa_pix(n, h, w, H, W);
      float dq = 0.f;                                   // dz at q
      float dx0 = 0.f, dx1 = 0.f;                       // input gradient at q (conv^T)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          // output pixel q - (ky - 1, kx - 1) took input q with tap (ky, kx)
          const int hh = h - ky + 1, ww = w - kx + 1;
          if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
            const int64_t p = sa_pix(n, hh, ww, H, W);
            const float dz = sc * (g[p] - k1 - (z[p] - mu) * inv * k2);
            dx0 = fmaf(wt[ky * 3 + kx], dz, dx0);
            if (WHICH == 1) dx1 = fmaf(wt[9 + ky * 3 + kx], dz, dx1);
            if (ky == 1 && kx == 1) dq = dz;
          }
        }
      if (WHICH == 2) {
        const float z1 = d.z1[q];
        const float g1 = fmaf(z1, sc1, sh1) > 0.f ? dx0 : 0.f;
        d.g1[q] = g1;
        acc[0] += g1;
        acc[1] = fmaf(g1, (z1 - mean1) * inv1, acc[1]);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int hh = h + ky - 1, ww = w + kx - 1;
            const float h1 = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? fmaxf(fmaf(d.z1[sa_pix(n, hh, ww, H, W)], sc1, sh1), 0.f) : 0.f;
            acc[2 + ky * 3 + kx] = fmaf(dq, h1, acc[2 + ky * 3 + kx]);
          }
        acc[11] += dq;
      } else {
        *(float2*)(d.dcomp + 2 * q) = make_float2(dx0, dx1);
        const float2* c = (const float2*)d.comp;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float2 v = c[sa_comp(n, h + ky - 1, w + kx - 1, H, W)];
            acc[ky * 3 + kx] = fmaf(dq, v.x, acc[ky * 3 + kx]);
            acc[9 + ky * 3 + kx] = fmaf(dq, v.y, acc[9 + ky * 3 + kx]);
          }
        acc[18] += dq;
      }
    }
  }
  sa_block_sum<NP>(acc, d.part + SA_PART_COLS * blockIdx.x);
}

// ---- folds of the backward partial sums (one work-group, fixed order, fp64) -----------------------------------------
__device__ __forceinline__ double sa_fold_col(const float* part, int rows, int col) {
  __shared__ double red[SA_THREADS];
  double a = 0.0;
  for (int r = threadIdx.x; r < rows; r += SA_THREADS) a += (double)part[(int64_t)r * SA_PART_COLS + col];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = SA_THREADS / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double v = red[0];
  __syncthreads();
  return v;
}

__global__ void __launch_bounds__(SA_THREADS) sa_bwd_coef_kernel(InsarSa d, int stage, int64_t count) {
  const bool t0 = threadIdx.x == 0;
  if (stage == 2 || stage == 1) {
    // BatchNorm backward of BN2 (stage 2, from dscale) or BN1 (stage 1, from the conv 1->1 stencil)
    const double sg = sa_fold_col(d.part, d.rows, 0), sgx = sa_fold_col(d.part, d.rows, 1);
    if (t0) {
      float* dgamma = stage == 2 ? d.dgamma2 : d.dgamma1;
      float* dbeta = stage == 2 ? d.dbeta2 : d.dbeta1;
      if (dgamma) dgamma[0] = (float)sgx;
      if (dbeta) dbeta[0] = (float)sg;
      float* k = d.coef + (stage == 2 ? 0 : 2);
      k[0] = d.training ? (float)(sg / (double)count) : 0.f;
      k[1] = d.training ? (float)(sgx / (double)count) : 0.f;
    }
    if (stage == 1) {
      for (int c = 0; c < 10; ++c) {
        const double v = sa_fold_col(d.part, d.rows, 2 + c);
        if (t0) {
          if (c < 9) d.dw2[c] = (float)v;
          else if (d.db2) d.db2[0] = (float)v;
        }
      }
    }
  } else {
    for (int c = 0; c < 19; ++c) {
      const double v = sa_fold_col(d.part, d.rows, c);
      if (t0) {
        if (c < 18) d.dw1[c] = (float)v;
        else if (d.db1) d.db1[0] = (float)v;
      }
    }
  }
}

// ---- dx = dy * s + d_mean / C + [c == argmax] * d_max, in place over dy ----------------------------------------------
template <typename T>
__global__ void __launch_bounds__(SA_THREADS) sa_dx_kernel(ActView dy, InsarSa d) {
  constexpr int CH = Chunk<T>::N;
  const int nch = dy.c_len / CH, H = dy.H, W = dy.W;
  const float invC = 1.f / (float)dy.c_len;
  const int items = W * nch;
  for (int r = blockIdx.x; r < dy.B * H; r += gridDim.x) {
    const int n = r / H, h = r - n * H;
    for (int t0 = threadIdx.x; t0 < items; t0 += SA_EW_UNROLL * SA_THREADS) {
      uint4 v[SA_EW_UNROLL];
#pragma unroll
      for (int u = 0; u < SA_EW_UNROLL; ++u) {
        const int t = t0 + u * SA_THREADS;
        if (t < items) {
          const int w = t / nch, cc = t - w * nch;
          v[u] = sa_chunk<T>(dy, n, h, w)[cc];
        }
      }
#pragma unroll
      for (int u = 0; u < SA_EW_UNROLL; ++u) {
        const int t = t0 + u * SA_THREADS;
        if (t < items) {
          const int w = t / nch, cc = t - w * nch;
          const int64_t p = sa_pix(n, h, w, H, W);
          const float s = d.s[p];
          const float2 dc = *(const float2*)(d.dcomp + 2 * p);
          const float dm = dc.x * invC;
          const int a = (int)d.arg[p] - cc * CH;
          float f[CH];
          Chunk<T>::unpack(v[u], f);
#pragma unroll
          for (int k = 0; k < CH; ++k) f[k] = fmaf(f[k], s, dm) + (k == a ? dc.y : 0.f);
          ((uint4*)(dy.base + dy.elem_offset(n, h, w) * (int64_t)sizeof(T)))[cc] = Chunk<T>::pack(f);
        }
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int sa_check(const InsarSa* d, const char* who, bool need_y) {
  int rc;
  if (!d) INSAR_FAIL(INSAR_E_ARG, "%s: null descriptor", who);
  if ((rc = insar_check_act(&d->x, who, "x"))) return rc;
  if (need_y) {
    if ((rc = insar_check_act(&d->y, who, "y"))) return rc;
    if (d->y.B != d->x.B || d->y.H != d->x.H || d->y.W != d->x.W || d->y.c_len != d->x.c_len || d->y.dtype != d->x.dtype)
      INSAR_FAIL(INSAR_E_SHAPE, "%s: x and y differ in shape or dtype", who);
  }
  if (d->x.c_len % 8 || d->x.c_len < 8 || d->x.c_len > 65535)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: C=%d must be a multiple of 8 in [8, 65535]", who, d->x.c_len);
  if (d->rows < 1 || d->rows > 4096) INSAR_FAIL(INSAR_E_SHAPE, "%s: rows=%d outside 1..4096", who, d->rows);
  if ((int64_t)d->x.B * d->x.H >= 0x7fffffffLL || (int64_t)d->x.W * d->x.c_len >= 0x7fffffffLL)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: tensor too large", who);
  return INSAR_OK;
}

static int sa_rows_grid(const InsarAct& x) { return insar_grid_cap((int64_t)x.B * x.H, 16384); }

// lanes per pixel of the channel-reduction passes: a power of two <= min(16, C / elements per chunk)
static int sa_lanes(const InsarAct& x) {
  const int nch = x.c_len / (x.dtype == INSAR_BF16 ? 8 : 4);
  return nch >= 16 ? 16 : nch >= 8 ? 8 : nch >= 4 ? 4 : nch >= 2 ? 2 : 1;
}

#define SA_DISPATCH_L(KERNEL, T, L, grid, s, ...)                                                         \
  switch (L) {                                                                                             \
    case 16: hipLaunchKernelGGL((KERNEL<T, 16>), dim3(grid), dim3(SA_THREADS), 0, s, __VA_ARGS__); break; \
    case 8: hipLaunchKernelGGL((KERNEL<T, 8>), dim3(grid), dim3(SA_THREADS), 0, s, __VA_ARGS__); break;   \
    case 4: hipLaunchKernelGGL((KERNEL<T, 4>), dim3(grid), dim3(SA_THREADS), 0, s, __VA_ARGS__); break;   \
    case 2: hipLaunchKernelGGL((KERNEL<T, 2>), dim3(grid), dim3(SA_THREADS), 0, s, __VA_ARGS__); break;   \
    default: hipLaunchKernelGGL((KERNEL<T, 1>), dim3(grid), dim3(SA_THREADS), 0, s, __VA_ARGS__); break;  \
  }

extern "C" int insar_sa_compress(const InsarSa* d, void* stream) {
  int rc;
  if ((rc = sa_check(d, "insar_sa_compress", false))) return rc;
  if (!d->comp || !d->arg) INSAR_FAIL(INSAR_E_ARG, "insar_sa_compress: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int grid = sa_rows_grid(d->x), L = sa_lanes(d->x);
  if (d->x.dtype == INSAR_BF16) { SA_DISPATCH_L(sa_compress_kernel, bf16_t, L, grid, s, make_view(d->x), d->comp, d->arg) }
  else { SA_DISPATCH_L(sa_compress_kernel, float, L, grid, s, make_view(d->x), d->comp, d->arg) }
  INSAR_CHECK_LAUNCH("insar_sa_compress");
  return INSAR_OK;
}

extern "C" int insar_sa_conv(const InsarSa* d, int32_t which, void* stream) {
  int rc;
  if ((rc = sa_check(d, "insar_sa_conv", false))) return rc;
  if (which != 1 && which != 2) INSAR_FAIL(INSAR_E_ARG, "insar_sa_conv: which=%d (1 | 2)", which);
  if (!d->comp || !d->z1 || !d->z2 || !d->w1 || !d->w2 || !d->bn || (d->training && (!d->stat1 || !d->stat2)))
    INSAR_FAIL(INSAR_E_ARG, "insar_sa_conv: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (which == 1) hipLaunchKernelGGL(sa_conv_kernel<1>, dim3(d->rows), dim3(SA_THREADS), 0, s, *d);
  else hipLaunchKernelGGL(sa_conv_kernel<2>, dim3(d->rows), dim3(SA_THREADS), 0, s, *d);
  INSAR_CHECK_LAUNCH("insar_sa_conv");
  return INSAR_OK;
}

extern "C" int insar_sa_gate(const InsarSa* d, void* stream) {
  int rc;
  if ((rc = sa_check(d, "insar_sa_gate", true))) return rc;
  if (!d->z2 || !d->s || !d->bn) INSAR_FAIL(INSAR_E_ARG, "insar_sa_gate: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int grid = sa_rows_grid(d->x);
  if (d->x.dtype == INSAR_BF16) hipLaunchKernelGGL(sa_gate_kernel<bf16_t>, dim3(grid), dim3(SA_THREADS), 0, s, make_view(d->x), make_view(d->y), *d);
  else hipLaunchKernelGGL(sa_gate_kernel<float>, dim3(grid), dim3(SA_THREADS), 0, s, make_view(d->x), make_view(d->y), *d);
  INSAR_CHECK_LAUNCH("insar_sa_gate");
  return INSAR_OK;
}

extern "C" int insar_sa_dscale(const InsarSa* d, void* stream) {
  int rc;
  if ((rc = sa_check(d, "insar_sa_dscale", true))) return rc;
  if (!d->z2 || !d->s || !d->g2 || !d->bn || !d->part) INSAR_FAIL(INSAR_E_ARG, "insar_sa_dscale: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int L = sa_lanes(d->x);
  if (d->x.dtype == INSAR_BF16) { SA_DISPATCH_L(sa_dscale_kernel, bf16_t, L, d->rows, s, make_view(d->x), make_view(d->y), *d) }
  else { SA_DISPATCH_L(sa_dscale_kernel, float, L, d->rows, s, make_view(d->x), make_view(d->y), *d) }
  INSAR_CHECK_LAUNCH("insar_sa_dscale");
  return INSAR_OK;
}

extern "C" int insar_sa_bwd_coef(const InsarSa* d, int32_t stage, void* stream) {
  int rc;
  if ((rc = sa_check(d, "insar_sa_bwd_coef", false))) return rc;
  if (stage < 0 || stage > 2) INSAR_FAIL(INSAR_E_ARG, "insar_sa_bwd_coef: stage=%d (0..2)", stage);
  if (!d->part || !d->coef || (stage == 2 && (!d->dgamma2 || !d->dbeta2)) || (stage == 1 && (!d->dgamma1 || !d->dbeta1 || !d->dw2)) ||
      (stage == 0 && !d->dw1))
    INSAR_FAIL(INSAR_E_ARG, "insar_sa_bwd_coef: null pointer");
  const int64_t count = (int64_t)d->x.B * d->x.H * d->x.W;
  hipLaunchKernelGGL(sa_bwd_coef_kernel, dim3(1), dim3(SA_THREADS), 0, (hipStream_t)stream, *d, (int)stage, count);
  INSAR_CHECK_LAUNCH("insar_sa_bwd_coef");
  return INSAR_OK;
}

extern "C" int insar_sa_bwd_stencil(const InsarSa* d, int32_t which, void* stream) {
  int rc;
  if ((rc = sa_check(d, "insar_sa_bwd_stencil", false))) return rc;
  if (which != 1 && which != 2) INSAR_FAIL(INSAR_E_ARG, "insar_sa_bwd_stencil: which=%d (1 | 2)", which);
  if (!d->comp || !d->z1 || !d->z2 || !d->g1 || !d->g2 || !d->dcomp || !d->w1 || !d->w2 || !d->bn || !d->coef || !d->part)
    INSAR_FAIL(INSAR_E_ARG, "insar_sa_bwd_stencil: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (which == 2) hipLaunchKernelGGL(sa_bwd_stencil_kernel<2>, dim3(d->rows), dim3(SA_THREADS), 0, s, *d);
  else hipLaunchKernelGGL(sa_bwd_stencil_kernel<1>, dim3(d->rows), dim3(SA_THREADS), 0, s, *d);
  INSAR_CHECK_LAUNCH("insar_sa_bwd_stencil");
  return INSAR_OK;
}

extern "C" int insar_sa_dx(const InsarSa* d, void* stream) {
  int rc;
  if ((rc = sa_check(d, "insar_sa_dx", true))) return rc;
  if (!d->s || !d->dcomp || !d->arg) INSAR_FAIL(INSAR_E_ARG, "insar_sa_dx: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int grid = sa_rows_grid(d->y);
  if (d->y.dtype == INSAR_BF16) hipLaunchKernelGGL(sa_dx_kernel<bf16_t>, dim3(grid), dim3(SA_THREADS), 0, s, make_view(d->y), *d);
  else hipLaunchKernelGGL(sa_dx_kernel<float>, dim3(grid), dim3(SA_THREADS), 0, s, make_view(d->y), *d);
  INSAR_CHECK_LAUNCH("insar_sa_dx");
  return INSAR_OK;
}
