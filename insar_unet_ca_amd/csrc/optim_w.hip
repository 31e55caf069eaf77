// AdamW with a device-side global-norm clip, learning-rate schedule and EMA weights (optim.AdamW; not in the reference, whose
// optimizer is optim.Adam(lr=1e-4), loss_optim.hip). One step = at most three launches on the caller's stream:
//   gradnorm_kernel   one work-group per chunk: sum (g * grad_scale)^2 -> one float per chunk        (clip / non-finite check only)
//   optw_advance_kernel  one work-group: folds the partials, writes every per-step scalar into the InsarOptwState block
//   adamw_kernel      one work-group per chunk: decay, Adam's update, EMA, all scalars read from that block
// No launch argument changes from step to step (a captured hipGraph replays), nothing is read back, no atomics: every
// scalar is written by one launch and read by the next one on the same stream, across a kernel boundary.
#include "common.h"
#include <math.h>

// Every product and sum below is rounded on its own; the fused multiply-adds are written out where adam_kernel has them.
#pragma clang fp contract(off)

namespace {

constexpr int OW_THREADS = 256;
constexpr int OW_ROW = 8;      // int64 words per tensor-table row

__device__ __forceinline__ float row_float(const int64_t* row, int k) { return __uint_as_float((uint32_t)(uint64_t)row[k]); }

// ---- sum of squares per chunk ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OW_THREADS)
gradnorm_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ chunks, int chunk_elems, float gscale,
                float* __restrict__ partials) {
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const float* g = (const float*)table[OW_ROW * ti + 1];
  const int64_t numel = table[OW_ROW * ti + 5];
  const int64_t beg = (int64_t)ci * chunk_elems;
  int64_t end = beg + chunk_elems; if (end > numel) end = numel;
  float acc = 0.f;
  int64_t tail = beg;
  if ((((uintptr_t)g) & 15) == 0) {
    const int64_t end4 = beg + ((end - beg) & ~(int64_t)3);
    for (int64_t i = beg + threadIdx.x * 4; i < end4; i += (int64_t)OW_THREADS * 4) {
      const float4 gg = *(const float4*)(g + i);
      const float a = gg.x * gscale, b = gg.y * gscale, c = gg.z * gscale, d = gg.w * gscale;
      acc = acc + a * a; acc = acc + b * b; acc = acc + c * c; acc = acc + d * d;
    }
    tail = end4;
  }
  for (int64_t i = tail + threadIdx.x; i < end; i += OW_THREADS) {
    const float a = g[i] * gscale;
    acc = acc + a * a;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_down(acc, o, 64);
  __shared__ float wsum[OW_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ---- the per-step scalars -------------------------------------------------------------------------------------------
// lr of the step that follows `done` finished steps (done = t - 1 for step t): optim.LRSchedule.lr_at restates this.
__device__ double optw_lr(const InsarOptwConfig& c, int64_t done) {
  if (c.schedule == INSAR_SCHED_NONE) return c.lr;
  if (done < c.warmup_steps) return c.lr * (c.warmup_start + (1.0 - c.warmup_start) * ((double)done / (double)c.warmup_steps));
  if (c.schedule == INSAR_SCHED_CONSTANT) return c.lr;
  if (done >= c.total_steps) return c.min_lr;
  const double q = (double)(done - c.warmup_steps) / (double)(c.total_steps - c.warmup_steps);
  if (c.schedule == INSAR_SCHED_COSINE) return c.min_lr + (c.lr - c.min_lr) * (0.5 * (1.0 + cos(M_PI * q)));
  return c.min_lr + (c.lr - c.min_lr) * pow(1.0 - q, c.power);
}

__global__ void __launch_bounds__(OW_THREADS)
optw_advance_kernel(InsarOptwConfig cfg, const float* __restrict__ partials, int nparts, InsarOptwState* __restrict__ st) {
  // fixed order: thread k adds partials k, k + 256, ... in double, then a binary tree over the 256 threads
  __shared__ double fold[OW_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += OW_THREADS) s += (double)partials[i];
  fold[threadIdx.x] = s;
  __syncthreads();
  for (int w = OW_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) fold[threadIdx.x] += fold[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double norm = sqrt(fold[0]);
  float coef = 1.f;
  if (nparts > 0) {
    st->grad_norm = (float)norm;
    if (cfg.max_norm >= 0.0) {
      const double c = cfg.max_norm / (norm + 1e-6);       // clip_grad_norm_'s coefficient
      if (!(c >= 1.0)) coef = (float)c;                    // a NaN norm stays visible, as in torch
    }
  }
  st->coef = coef;
  if (cfg.skip_nonfinite && nparts > 0 && !isfinite(norm)) {
    st->skip = 1;
    st->skipped += 1;
    return;                                                // t, the corrections, lr and the EMA factor stay
  }
  st->skip = 0;
  const int64_t t = st->t + 1;
  st->t = t;
  st->bc1 = (float)(1.0 - pow(cfg.beta1, (double)t));
  st->bc2_sqrt = (float)sqrt(1.0 - pow(cfg.beta2, (double)t));
  st->lr = (float)optw_lr(cfg, t - 1);
  double decay = cfg.ema_decay;
  if (cfg.ema_warmup) decay = fmin(decay, (1.0 + (double)t) / (10.0 + (double)t));
  st->ema_alpha = cfg.ema_decay >= 0.0 ? (float)(1.0 - decay) : 0.f;
}

// ---- the update -----------------------------------------------------------------------------------------------------
struct OwScalars {
  float gs;        // grad_scale * coef
  float wd;        // weight_decay of this tensor (L2 form), or lr * lr_mult * weight_decay (decoupled form)
  float lr_over_bc1, inv_bc2_sqrt, b2, omb1, omb2, eps, alpha;
};

// One element. FMA_V: adam_kernel's float4 body accumulates v with one fused multiply-add, its element-wise loops with a
// product and a sum; both are kept, so that without decay, clip and EMA the result is bitwise adam_kernel's on every path.
template <bool DECOUPLED, bool FMA_V>
__device__ __forceinline__ void adamw_elem(float& p, const float g, float& m, float& v, const OwScalars& k) {
  float gj, dm;
  if constexpr (DECOUPLED) {
    p = p - k.wd * p;
    gj = g * k.gs;
    dm = __builtin_fmaf(g, k.gs, -m);                      // gj - m, as adam_kernel compiles it
  } else {
    gj = g * k.gs + k.wd * p;
    dm = gj - m;
  }
  m = __builtin_fmaf(k.omb1, dm, m);
  if constexpr (FMA_V) v = __builtin_fmaf(gj, k.omb2 * gj, k.b2 * v); else v = k.b2 * v + gj * (k.omb2 * gj);
  const float den = __builtin_fmaf(k.inv_bc2_sqrt, sqrtf(v), k.eps);
  p = __builtin_fmaf(-k.lr_over_bc1, m / den, p);
}

__device__ __forceinline__ float ema_elem(const float e, const float p, const float alpha) { return e + (p - e) * alpha; }

template <bool DECOUPLED>
__global__ void __launch_bounds__(OW_THREADS)
adamw_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ chunks, int chunk_elems, float b1, float b2,
             float eps, float gscale, const InsarOptwState* __restrict__ st) {
  if (st->skip) return;                                    // the whole work-group: nothing is touched
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const int64_t* row = table + (int64_t)OW_ROW * ti;
  float* p = (float*)row[0];
  const float* g = (const float*)row[1];
  float* m = (float*)row[2];
  float* v = (float*)row[3];
  float* ema = (float*)row[4];
  const int64_t numel = row[5];
  const float lr = st->lr * row_float(row, 7);
  OwScalars k;
  k.gs = gscale * st->coef;
  k.wd = DECOUPLED ? lr * row_float(row, 6) : row_float(row, 6);
  k.lr_over_bc1 = lr / st->bc1;
  k.inv_bc2_sqrt = 1.f / st->bc2_sqrt;
  k.b2 = b2; k.omb1 = 1.f - b1; k.omb2 = 1.f - b2; k.eps = eps; k.alpha = st->ema_alpha;
  const int64_t beg = (int64_t)ci * chunk_elems;
  int64_t end = beg + chunk_elems; if (end > numel) end = numel;
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0;
  int64_t tail = beg;
  if (vec) {
    const int64_t end4 = beg + ((end - beg) & ~(int64_t)3);
    for (int64_t i = beg + threadIdx.x * 4; i < end4; i += (int64_t)OW_THREADS * 4) {
      float4 pp = *(float4*)(p + i), gg = *(const float4*)(g + i), mm = *(float4*)(m + i), vv = *(float4*)(v + i);
      float4 ee = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ema) ee = *(float4*)(ema + i);                   // issued with the other loads, not behind the stores
      float* pa = (float*)&pp; float* ga = (float*)&gg; float* ma = (float*)&mm; float* va = (float*)&vv;
#pragma unroll
      for (int j = 0; j < 4; ++j) adamw_elem<DECOUPLED, true>(pa[j], ga[j], ma[j], va[j], k);
      *(float4*)(p + i) = pp; *(float4*)(m + i) = mm; *(float4*)(v + i) = vv;
      if (ema) {
        ee.x = ema_elem(ee.x, pp.x, k.alpha); ee.y = ema_elem(ee.y, pp.y, k.alpha);
        ee.z = ema_elem(ee.z, pp.z, k.alpha); ee.w = ema_elem(ee.w, pp.w, k.alpha);
        *(float4*)(ema + i) = ee;
      }
    }
    tail = end4;
  }
  for (int64_t i = tail + threadIdx.x; i < end; i += OW_THREADS) {
    float pj = p[i], mj = m[i], vj = v[i];
    adamw_elem<DECOUPLED, false>(pj, g[i], mj, vj, k);
    m[i] = mj; v[i] = vj; p[i] = pj;
    if (ema) ema[i] = ema_elem(ema[i], pj, k.alpha);
  }
}

int check_chunking(const char* who, const void* table, const void* chunks, int32_t nchunks, int32_t chunk_elems) {
  if (!table || !chunks) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (nchunks < 1 || chunk_elems < 4 || (chunk_elems & 3)) INSAR_FAIL(INSAR_E_SHAPE, "%s: bad chunking", who);
  return INSAR_OK;
}

}  // namespace

extern "C" int insar_gradnorm_partials(const int64_t* table, const int32_t* chunks, int32_t nchunks, int32_t chunk_elems,
                                       float grad_scale, float* partials, void* stream) {
  if (int rc = check_chunking("insar_gradnorm_partials", table, chunks, nchunks, chunk_elems)) return rc;
  if (!partials) INSAR_FAIL(INSAR_E_ARG, "insar_gradnorm_partials: null workspace");
  hipLaunchKernelGGL(gradnorm_kernel, dim3(nchunks), dim3(OW_THREADS), 0, (hipStream_t)stream, table, chunks, chunk_elems,
                     grad_scale, partials);
  INSAR_CHECK_LAUNCH("insar_gradnorm_partials");
  return INSAR_OK;
}

extern "C" int insar_optw_advance(const InsarOptwConfig* cfg, const float* partials, int32_t nparts, InsarOptwState* state,
                                  void* stream) {
  if (!cfg || !state) INSAR_FAIL(INSAR_E_ARG, "insar_optw_advance: null pointer");
  if (nparts < 0 || (nparts > 0 && !partials)) INSAR_FAIL(INSAR_E_ARG, "insar_optw_advance: %d partials without a workspace", nparts);
  if (cfg->schedule < INSAR_SCHED_NONE || cfg->schedule > INSAR_SCHED_POLY || cfg->warmup_steps < 0)
    INSAR_FAIL(INSAR_E_ARG, "insar_optw_advance: schedule=%d warmup_steps=%lld", cfg->schedule, (long long)cfg->warmup_steps);
  if (cfg->schedule >= INSAR_SCHED_COSINE && cfg->total_steps <= cfg->warmup_steps)
    INSAR_FAIL(INSAR_E_ARG, "insar_optw_advance: total_steps=%lld must exceed warmup_steps=%lld", (long long)cfg->total_steps,
               (long long)cfg->warmup_steps);
  if (!(cfg->ema_decay < 1.0)) INSAR_FAIL(INSAR_E_ARG, "insar_optw_advance: ema_decay must be below 1");
  hipLaunchKernelGGL(optw_advance_kernel, dim3(1), dim3(OW_THREADS), 0, (hipStream_t)stream, *cfg, partials, (int)nparts, state);
  INSAR_CHECK_LAUNCH("insar_optw_advance");
  return INSAR_OK;
}

extern "C" int insar_adamw_step(const int64_t* table, const int32_t* chunks, int32_t nchunks, int32_t chunk_elems, float beta1,
                                float beta2, float eps, float grad_scale, int32_t decoupled, const InsarOptwState* state,
                                void* stream) {
  if (int rc = check_chunking("insar_adamw_step", table, chunks, nchunks, chunk_elems)) return rc;
  if (!state) INSAR_FAIL(INSAR_E_ARG, "insar_adamw_step: null state block");
  if (decoupled)
    hipLaunchKernelGGL(adamw_kernel<true>, dim3(nchunks), dim3(OW_THREADS), 0, (hipStream_t)stream, table, chunks, chunk_elems,
                       beta1, beta2, eps, grad_scale, state);
  else
    hipLaunchKernelGGL(adamw_kernel<false>, dim3(nchunks), dim3(OW_THREADS), 0, (hipStream_t)stream, table, chunks, chunk_elems,
                       beta1, beta2, eps, grad_scale, state);
  INSAR_CHECK_LAUNCH("insar_adamw_step");
  return INSAR_OK;
}
