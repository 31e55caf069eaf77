// The SE-gated residual tail of the FCN-ResNet50 bottleneck (PSPNet-ChannelAttention.py:83-126, BottleneckWithSE):
//   t = bn3(conv3(.)) = y*scale + shift,  s = SEBlock(t) (per image and channel),  out = relu(s*t + identity).
// The squeeze (per-image channel sums of y), the excitation MLP and the whole backward reuse the U-Net SE kernels of
// pointwise.hip in their no-ReLU mode (relu = 0: the mask is all-ones, so sum mask*y is sum y and the SE backward sees
// the BatchNorm output itself); what they cannot do is the gated residual apply, which lives here.
// HBM-bound: 16-byte accesses, one work-group per image row, the gate chunk of an image loaded once per image.
#include "common.h"

#define SER_THREADS 256
#define SER_UNROLL 4      // 16-byte chunks in flight per thread and operand

template <typename T>
__device__ __forceinline__ const uint4* ser_chunk(const ActView& v, int n, int h, int w, int cc) {
  return (const uint4*)(v.base + (v.elem_offset(n, h, w) + (int64_t)cc * Chunk<T>::N) * (int64_t)sizeof(T));
}
template <typename T>
__device__ __forceinline__ uint4* ser_chunk_w(const ActView& v, int n, int h, int w, int cc) {
  return (uint4*)(v.base + (v.elem_offset(n, h, w) + (int64_t)cc * Chunk<T>::N) * (int64_t)sizeof(T));
}

// dst = relu(gate[n][c] * (y*scale + shift) + res). A thread owns the channel chunks cc = threadIdx.x % cstep + k * cstep
// and the pixels w = lane + k * lanes of every row it visits (cpp divides the block, or the block divides cpp).
template <typename T>
__global__ void __launch_bounds__(SER_THREADS) se_res_apply_kernel(ActView y, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, const float* __restrict__ gate,
                                                                   ActView res, ActView dst) {
  constexpr int CH = Chunk<T>::N;
  const int cpp = y.c_len / CH;
  const int rows = y.B * y.H;
  const int lanes = cpp >= (int)blockDim.x ? 1 : (int)blockDim.x / cpp;       // pixel lanes of the block
  const int cstep = cpp >= (int)blockDim.x ? (int)blockDim.x : cpp;          // chunk stride of one thread
  const int lane = (int)threadIdx.x / cstep;
  for (int cc = (int)threadIdx.x % cstep; cc < cpp; cc += cstep) {
    float a[CH], b[CH], sa[CH], sb[CH];       // sa, sb = s*scale, s*shift of the current image
#pragma unroll
    for (int j = 0; j < CH; ++j) { a[j] = scale[cc * CH + j]; b[j] = shift[cc * CH + j]; sa[j] = 0.f; sb[j] = 0.f; }
    int n_loaded = -1;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
      const int n = r / y.H, h = r - n * y.H;
      if (n != n_loaded) {
        const float* gp = gate + (int64_t)n * y.c_len + cc * CH;
#pragma unroll
        for (int j = 0; j < CH; ++j) { const float s = gp[j]; sa[j] = s * a[j]; sb[j] = s * b[j]; }
        n_loaded = n;
      }
      for (int w0 = lane; w0 < y.W; w0 += SER_UNROLL * lanes) {
        uint4 vy[SER_UNROLL], vr[SER_UNROLL];
#pragma unroll
        for (int u = 0; u < SER_UNROLL; ++u)
          if (w0 + u * lanes < y.W) {
            vy[u] = *ser_chunk<T>(y, n, h, w0 + u * lanes, cc);
            vr[u] = *ser_chunk<T>(res, n, h, w0 + u * lanes, cc);
          }
#pragma unroll
        for (int u = 0; u < SER_UNROLL; ++u)
          if (w0 + u * lanes < y.W) {
            float f[CH], q[CH];
            Chunk<T>::unpack(vy[u], f);
            Chunk<T>::unpack(vr[u], q);
#pragma unroll
            for (int j = 0; j < CH; ++j) f[j] = fmaxf(fmaf(f[j], sa[j], sb[j]) + q[j], 0.f);
            *ser_chunk_w<T>(dst, n, h, w0 + u * lanes, cc) = Chunk<T>::pack(f);
          }
      }
    }
  }
}

static int ser_same_grid(const InsarAct* a, const InsarAct* b, const char* who) {
  if (a->B != b->B || a->H != b->H || a->W != b->W || a->c_len != b->c_len || a->dtype != b->dtype)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: operands differ in shape or dtype", who);
  return INSAR_OK;
}

extern "C" int insar_se_res_apply(const InsarAct* y, const float* scale, const float* shift, const float* gate,
                                  const InsarAct* res, const InsarAct* dst, void* stream) {
  int rc;
  const char* who = "insar_se_res_apply";
  if ((rc = insar_check_act(y, who, "y"))) return rc;
  if ((rc = insar_check_act(res, who, "res"))) return rc;
  if ((rc = insar_check_act(dst, who, "dst"))) return rc;
  if (!scale || !shift || !gate) INSAR_FAIL(INSAR_E_ARG, "%s: null scale / shift / gate", who);
  if ((rc = ser_same_grid(y, res, who))) return rc;
  if ((rc = ser_same_grid(y, dst, who))) return rc;
  const int ch = y->dtype == INSAR_BF16 ? 8 : 4;
  const int cpp = y->c_len / ch;
  if (y->c_len % ch || cpp < 1 || (cpp < SER_THREADS ? SER_THREADS % cpp : cpp % SER_THREADS))
    INSAR_FAIL(INSAR_E_SHAPE, "%s: C=%d: its %d-channel chunks must divide or be a multiple of %d", who, y->c_len, ch,
               SER_THREADS);
  int grid = insar_grid_cap((int64_t)y->B * y->H);
  hipStream_t s = (hipStream_t)stream;
  if (y->dtype == INSAR_BF16)
    hipLaunchKernelGGL(se_res_apply_kernel<bf16_t>, dim3(grid), dim3(SER_THREADS), 0, s, make_view(*y), scale, shift, gate,
                       make_view(*res), make_view(*dst));
  else
    hipLaunchKernelGGL(se_res_apply_kernel<float>, dim3(grid), dim3(SER_THREADS), 0, s, make_view(*y), scale, shift, gate,
                       make_view(*res), make_view(*dst));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
