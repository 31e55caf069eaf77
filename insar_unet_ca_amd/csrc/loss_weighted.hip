// Imbalance-aware losses (build-side addition; the reference trains with the plain criterion of :465): class-weighted and
// label-smoothed cross entropy, focal loss, their fusion with soft-Dice, and the per-class pixel histogram the weights are
// derived from. Same conventions as loss_optim.hip: NCHW fp32 logits, int64 targets, caller's stream and workspace, block
// partials folded in fixed order by one block (bitwise reproducible, no float atomics). All HBM-bound streaming passes.
//
// A pixel is valid when its target is not ignore_index AND lies in [0, K): the class weight is indexed by the target, so a
// stray label is treated like an ignored pixel here instead of being read past the weight vector.
//
//   weighted / smoothed CE (torch semantics, mean reduction), W = sum_i v_i w[y_i], S = sum_c w_c:
//     L      = [(1-e) sum_i v_i w[y_i] nll_{i,y_i} + (e/K) sum_i v_i sum_c w_c nll_{i,c}] / W,   nll_{i,c} = -log p_{i,c}
//     dL/dz  = v_i [(1-e) w[y_i] (p_k - d_{k,y_i}) + (e/K) (S p_k - w_k)] / W
//   focal, q = 1 - p_t summed from the OTHER classes' exponentials (no 1 - p_t cancellation on confident pixels):
//     L      = sum_i v_i a[y_i] q^g nll_{i,t} / n_valid
//     dL/dz  = v_i a[y_i] [g q^(g-1) p_t log p_t - q^g] (d_{k,t} - p_k) / n_valid
#include "common.h"

#define LW_THREADS 256
#define LW_MAXK 16

struct LwTerm {
  float ome;     // 1 - label_smoothing
  float epk;     // label_smoothing / K
  float gamma;   // focal exponent (focal kernels only)
};

__device__ __forceinline__ float lw_block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}

// q^g without 0 * inf: g == 0 gives 1 for every q, q == 0 gives 0 for g > 0. g multiplies the ABSOLUTE error of log q, and on a
// misclassified pixel (q near 1, where the focal factor is largest) log q is small: __logf is good to about 2^-21 absolute
// there and q = so / se carries 1.2e-7 of its own, which made q^5 wrong by 4e-6 of its value. So log q comes from the
// full-precision functions, and above 1/2 from p_t = 1 - q, which is the small, relatively accurate one of the two.
__device__ __forceinline__ float lw_powg(float q, float pt, float g) {
  const float lq = q > 0.5f ? log1pf(-pt) : logf(q);
  return g == 0.f ? 1.f : (q > 0.f ? __expf(g * lq) : 0.f);
}

// -log p_t with p_t = e_t / (e_t + so), so = the other classes' exponentials. On a confident pixel e_t + so rounds to e_t and
// (mx - v_t) + log(se) returns 0 where the true value is so / e_t: there log(1 + r), r = so / e_t, comes from its series
// (r < 1/64: the first dropped term is r^4 / 5 < 1.2e-8 r). e_t == 0 makes r inf or NaN and takes the other branch.
__device__ __forceinline__ float lw_nll(float vt, float et, float so, float mx, float lg) {
  const float r = __fdividef(so, et);
  return r < 0.015625f ? r * (1.f - r * (0.5f - r * (0.33333334f - 0.25f * r))) : (mx - vt) + lg;
}

// One valid pixel, classes 0..K-1 of v / e (e_k = exp(v_k - mx)) held in registers (KM = compile-time bound, K <= KM).
// w: class weights (alpha for focal), wy = w[t]. Adds the pixel's loss numerator to num.
template <int KM, bool FOCAL>
__device__ __forceinline__ float lw_pixel_num(const float (&v)[KM], const float (&e)[KM], int K, int t, float wy, const float* w,
                                              float mx, float rse, float lg, LwTerm tm) {
  float vt = 0.f;
#pragma unroll
  for (int k = 0; k < KM; ++k) vt = (k < K && k == t) ? v[k] : vt;
  if constexpr (FOCAL) {
    float so = 0.f, et = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const bool hit = k < K && k == t;
      et = hit ? e[k] : et;
      so += (k < K && !hit) ? e[k] : 0.f;
    }
    return wy * lw_powg(so * rse, et * rse, tm.gamma) * lw_nll(vt, et, so, mx, lg);
  } else {
    const float nll_t = (mx - vt) + lg;
    float sm = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K) sm = fmaf(w[k], (mx - v[k]) + lg, sm);
    return tm.ome * wy * nll_t + tm.epk * sm;
  }
}

// The CE-like half of the gradient of one valid pixel: o[k] = dL/dz_k, inv = (outer factor) / normaliser.
template <int KM, bool FOCAL>
__device__ __forceinline__ void lw_pixel_grad(const float (&v)[KM], const float (&e)[KM], int K, int t, float wy, const float* w,
                                              float S, float mx, float rse, float lg, LwTerm tm, float inv, float (&o)[KM]) {
  if constexpr (FOCAL) {
    float vt = 0.f, et = 0.f, so = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const bool hit = k < K && k == t;
      vt = hit ? v[k] : vt;
      et = hit ? e[k] : et;
      so += (k < K && !hit) ? e[k] : 0.f;
    }
    // From the fp32 exponentials on, the coefficient is formed in double and rounded once per element. On a misclassified
    // pixel it exceeds 1 (at g = 2, p_t = 0.006 the two elements are -+1.04), and in fp32 the roundings of q^g, of
    // lead - q^g and of the product with q alone add up to 2 half-ulps of it: more than a gradient held to 4 x 2e-8 of a
    // scaled O(1) value may carry. The kernel stays bound by its loads and stores; the branches of lw_nll are kept.
    const double sed = (double)et + (double)so, rsed = 1.0 / sed;
    const double q = (double)so * rsed, pt = (double)et * rsed, g = (double)tm.gamma;
    // so / e_t < 1/64 makes t the arg-max, e_t = exp(0) = 1 and the ratio so itself
    const double logpt = -((et == 1.f && so < 0.015625f) ? log1p((double)so) : ((double)mx - (double)vt) + log(sed));
    const double qg = tm.gamma == 0.f ? 1.0 : (q > 0.0 ? exp(g * log(q)) : 0.0);
    // g q^(g-1) p_t log p_t as one guarded quantity: 0 for g == 0 and for q == 0
    const double lead = (tm.gamma == 0.f || !(q > 0.0)) ? 0.0 : g * (qg / q) * pt * logpt;
    const double c = (double)wy * (lead - qg) * (double)inv;
    // d_{k,t} - p_k: for k == t that is q itself, not 1 - p_t (which cancels on exactly the pixels the focal factor is for)
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K) o[k] = (float)(c * (k == t ? q : -((double)e[k] * rsed)));
  } else {
    const float a = tm.ome * wy;
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if (k < K) {
        const float pr = e[k] * rse;
        o[k] = (a * (pr - (k == t ? 1.f : 0.f)) + tm.epk * (S * pr - w[k])) * inv;
      }
  }
}

__device__ __forceinline__ bool lw_valid(int64_t t, int64_t ignore_index, int K) {
  return t != ignore_index && (uint64_t)t < (uint64_t)K;
}

// ---------------------------------------------------------------------------------------------
// insar_cross_entropy_w / insar_focal: the four launches of insar_cross_entropy (normaliser from the targets alone, fold,
// one pass over the logits that writes the gradient, fold).
// ws layout: [0] normaliser (W, or n_valid for focal) [1] its reciprocal [2 .. 2+nb) normaliser partials [2+nb .. 2+2nb) loss partials
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LW_THREADS) lw_norm_kernel(const int64_t* __restrict__ target, int64_t npix, int64_t ignore_index, int K,
                               const float* __restrict__ weight /*null: count*/, float* ws) {
  __shared__ float red[8];
  __shared__ float sw[LW_MAXK];
  if (threadIdx.x < LW_MAXK) sw[threadIdx.x] = (weight && (int)threadIdx.x < K) ? weight[threadIdx.x] : 1.f;
  __syncthreads();
  float c = 0.f;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = target[p];
    if (lw_valid(t, ignore_index, K)) c += sw[(int)t];
  }
  c = lw_block_sum(c, red);
  if (threadIdx.x == 0) ws[2 + blockIdx.x] = c;
}

__global__ void lw_norm_final_kernel(float* ws, int nb) {
  __shared__ float red[8];
  float c = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) c += ws[2 + i];
  c = lw_block_sum(c, red);
  if (threadIdx.x == 0) { ws[0] = c; ws[1] = 1.f / c; }
}

// KM < LW_MAXK: exactly KM classes (the class loops fold to straight code); KM == LW_MAXK: any K, predicated loops
template <int KM, bool FOCAL>
__global__ void __launch_bounds__(LW_THREADS) lw_main_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int Kin, int64_t HW,
                               int64_t npix, int64_t ignore_index, const float* __restrict__ weight /*null: ones*/, LwTerm tm,
                               float* __restrict__ dlogits, float* ws, int nb) {
  const int K = KM < LW_MAXK ? KM : Kin;
  __shared__ float red[8];
  __shared__ float sw[LW_MAXK];
  if (threadIdx.x < LW_MAXK) sw[threadIdx.x] = (int)threadIdx.x < K ? (weight ? weight[threadIdx.x] : 1.f) : 0.f;
  __syncthreads();
  float S = 0.f;
  for (int k = 0; k < K; ++k) S += sw[k];
  const float inv = ws[1];
  float lsum = 0.f;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = p / HW, hw = p - n * HW;
    const float* lp = logits + n * K * HW + hw;
    float* gp = dlogits + n * K * HW + hw;
    const int64_t t64 = target[p];
    float v[KM], e[KM], o[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) { v[k] = k < K ? lp[k * HW] : 0.f; o[k] = 0.f; }
    if (lw_valid(t64, ignore_index, K)) {
      const int t = (int)t64;
      float mx = v[0];
#pragma unroll
      for (int k = 1; k < KM; ++k) if (k < K) mx = fmaxf(mx, v[k]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < KM; ++k) { e[k] = k < K ? __expf(v[k] - mx) : 0.f; se += e[k]; }
      const float rse = 1.f / se, lg = __logf(se), wy = sw[t];
      lsum += lw_pixel_num<KM, FOCAL>(v, e, K, t, wy, sw, mx, rse, lg, tm);
      lw_pixel_grad<KM, FOCAL>(v, e, K, t, wy, sw, S, mx, rse, lg, tm, inv, o);
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) if (k < K) gp[k * HW] = o[k];
  }
  lsum = lw_block_sum(lsum, red);
  if (threadIdx.x == 0) ws[2 + nb + blockIdx.x] = lsum;
}

__global__ void lw_loss_final_kernel(float* ws, int nb, float* loss_out) {
  __shared__ float red[8];
  float c = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) c += ws[2 + nb + i];
  c = lw_block_sum(c, red);
  if (threadIdx.x == 0) loss_out[0] = c * ws[1];
}

static int lw_check(const char* who, const void* logits, const void* target, const void* dlogits, const void* loss_out,
                    const void* ws, int32_t B, int32_t K, int64_t HW) {
  if (!logits || !target || !dlogits || !loss_out || !ws) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (K < 1 || K > LW_MAXK) INSAR_FAIL(INSAR_E_SHAPE, "%s: num_classes=%d must be 1..%d", who, K, LW_MAXK);
  if (B < 1 || HW < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: bad shape", who);
  return INSAR_OK;
}

#define LW_MAIN_K(KM, FO, W)                                                                                                  \
  hipLaunchKernelGGL((lw_main_kernel<KM, FO>), dim3(nb), dim3(LW_THREADS), 0, s, logits, target, K, HW, npix, ignore_index, W, tm, \
                     dlogits, ws, nb)
#define LW_MAIN(FO, W)                        \
  do {                                        \
    if (K == 2) LW_MAIN_K(2, FO, W);          \
    else if (K == 3) LW_MAIN_K(3, FO, W);     \
    else if (K == 4) LW_MAIN_K(4, FO, W);     \
    else LW_MAIN_K(LW_MAXK, FO, W);           \
  } while (0)

extern "C" int insar_cross_entropy_w(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW,
                                     int64_t ignore_index, const float* weight, float label_smoothing, float* dlogits,
                                     float* loss_out, float* ws, void* stream) {
  if (int rc = lw_check("insar_cross_entropy_w", logits, target, dlogits, loss_out, ws, B, K, HW)) return rc;
  if (!weight) INSAR_FAIL(INSAR_E_ARG, "insar_cross_entropy_w: null pointer (weight)");
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f))
    INSAR_FAIL(INSAR_E_ARG, "insar_cross_entropy_w: label_smoothing=%g must be in [0, 1)", (double)label_smoothing);
  const int64_t npix = (int64_t)B * HW;
  const int nb = insar_ce_blocks(npix);
  hipStream_t s = (hipStream_t)stream;
  const LwTerm tm = {1.f - label_smoothing, label_smoothing / (float)K, 0.f};
  hipLaunchKernelGGL(lw_norm_kernel, dim3(nb), dim3(LW_THREADS), 0, s, target, npix, ignore_index, K, weight, ws);
  hipLaunchKernelGGL(lw_norm_final_kernel, dim3(1), dim3(LW_THREADS), 0, s, ws, nb);
  LW_MAIN(false, weight);
  hipLaunchKernelGGL(lw_loss_final_kernel, dim3(1), dim3(LW_THREADS), 0, s, ws, nb, loss_out);
  INSAR_CHECK_LAUNCH("insar_cross_entropy_w");
  return INSAR_OK;
}

extern "C" int insar_focal(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW, int64_t ignore_index,
                           float gamma, const float* alpha, float* dlogits, float* loss_out, float* ws, void* stream) {
  if (int rc = lw_check("insar_focal", logits, target, dlogits, loss_out, ws, B, K, HW)) return rc;
  if (!(gamma >= 0.f) || !(gamma <= 64.f)) INSAR_FAIL(INSAR_E_ARG, "insar_focal: gamma=%g must be in [0, 64]", (double)gamma);
  const int64_t npix = (int64_t)B * HW;
  const int nb = insar_ce_blocks(npix);
  hipStream_t s = (hipStream_t)stream;
  const LwTerm tm = {1.f, 0.f, gamma};
  hipLaunchKernelGGL(lw_norm_kernel, dim3(nb), dim3(LW_THREADS), 0, s, target, npix, ignore_index, K, (const float*)nullptr, ws);
  hipLaunchKernelGGL(lw_norm_final_kernel, dim3(1), dim3(LW_THREADS), 0, s, ws, nb);
  LW_MAIN(true, alpha);
  hipLaunchKernelGGL(lw_loss_final_kernel, dim3(1), dim3(LW_THREADS), 0, s, ws, nb, loss_out);
  INSAR_CHECK_LAUNCH("insar_focal");
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// insar_dice_ce_w: ce_weight * (weighted / smoothed CE, or focal) + dice_weight * Dice in the three launches of insar_dice_ce.
// ws layout (floats): [0] normaliser (W, or n_valid for focal) [1] its reciprocal [2] loss numerator [3] n_valid
//                     [4 .. 4+3K) totals I,P,T ; then per block: [n_valid, W, numerator, I[K], P[K], T[K]]  (3 + 3K floats each)
// ---------------------------------------------------------------------------------------------
#define LW_HEAD 4
#define LW_BLK(K) (3 + 3 * (K))

// The class weight of a runtime class out of a register array. Written with bit masks: hipcc turns a chain of selects on
// w[k] back into w[t] and moves the array to LDS for that (one ds_read per pixel); the masked OR stays in registers.
template <int KT>
__device__ __forceinline__ float lw_pick(const float (&w)[KT], int t) {
  uint32_t r = 0u;
#pragma unroll
  for (int k = 0; k < KT; ++k) r |= __float_as_uint(w[k]) & (k == t ? 0xffffffffu : 0u);
  return __uint_as_float(r);
}

// component J of a float4 by a compile-time index: the four pixels of a thread are four explicit instantiations, so no
// register array is ever indexed by a loop counter the compiler might leave rolled (it then moves the array to LDS)
template <int J> __device__ __forceinline__ float lw_get(const float4& a) {
  if constexpr (J == 0) return a.x; else if constexpr (J == 1) return a.y; else if constexpr (J == 2) return a.z; else return a.w;
}
template <int J> __device__ __forceinline__ void lw_set(float4& a, float x) {
  if constexpr (J == 0) a.x = x; else if constexpr (J == 1) a.y = x; else if constexpr (J == 2) a.z = x; else a.w = x;
}

template <int KT, bool FOCAL, int J>
__device__ __forceinline__ void lw_v4_stats(const float4 (&lv)[KT], int64_t t64, int64_t ignore_index, const float (&w)[KT],
                                            LwTerm tm, float& cnt, float& wsum, float& lsum, float (&aI)[KT], float (&aP)[KT],
                                            float (&aT)[KT]) {
  // no branch on validity: every component of the 16-byte loads is used on every path (a pixel skipped under a branch
  // lets hipcc sink that component's load into the branch and split the dwordx4 into dword + dwordx3)
  const bool ok = lw_valid(t64, ignore_index, KT);
  const int t = ok ? (int)t64 : 0;
  float v[KT], e[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) v[k] = lw_get<J>(lv[k]);
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < KT; ++k) mx = fmaxf(mx, v[k]);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) { e[k] = __expf(v[k] - mx); se += e[k]; }
  const float rse = 1.f / se, lg = __logf(se), wy = lw_pick<KT>(w, t);
  cnt += ok ? 1.f : 0.f;
  wsum += ok ? wy : 0.f;
  lsum += ok ? lw_pixel_num<KT, FOCAL>(v, e, KT, t, wy, w, mx, rse, lg, tm) : 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    const float pr = ok ? e[k] * rse : 0.f;
    aP[k] += pr;
    aI[k] += k == t ? pr : 0.f;
    aT[k] += (ok && k == t) ? 1.f : 0.f;
  }
}

template <int KT, bool FOCAL>
__global__ void __launch_bounds__(LW_THREADS)
lw_dicece_partial_v4(const float* __restrict__ logits, const int64_t* __restrict__ target, int64_t HW, int64_t npix,
                     int64_t ignore_index, const float* __restrict__ weight /*null: ones*/, LwTerm tm, float* ws) {
  __shared__ float red[8];
  float w[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) w[k] = weight ? weight[k] : 1.f;
  float aI[KT], aP[KT], aT[KT];
  float cnt = 0.f, wsum = 0.f, lsum = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) { aI[k] = 0.f; aP[k] = 0.f; aT[k] = 0.f; }
  const int64_t ngroups = npix >> 2;
  for (int64_t gi = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gi < ngroups; gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = gi << 2;
    const int64_t n = p / HW, hw = p - n * HW;
    const longlong2 t01 = *(const longlong2*)(target + p), t23 = *(const longlong2*)(target + p + 2);
    float4 lv[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) lv[k] = *(const float4*)(logits + (n * KT + k) * HW + hw);
    lw_v4_stats<KT, FOCAL, 0>(lv, t01.x, ignore_index, w, tm, cnt, wsum, lsum, aI, aP, aT);
    lw_v4_stats<KT, FOCAL, 1>(lv, t01.y, ignore_index, w, tm, cnt, wsum, lsum, aI, aP, aT);
    lw_v4_stats<KT, FOCAL, 2>(lv, t23.x, ignore_index, w, tm, cnt, wsum, lsum, aI, aP, aT);
    lw_v4_stats<KT, FOCAL, 3>(lv, t23.y, ignore_index, w, tm, cnt, wsum, lsum, aI, aP, aT);
  }
  float* out = ws + LW_HEAD + 3 * KT + (int64_t)blockIdx.x * LW_BLK(KT);
  const float c = lw_block_sum(cnt, red), ww = lw_block_sum(wsum, red), l = lw_block_sum(lsum, red);
  if (threadIdx.x == 0) { out[0] = c; out[1] = ww; out[2] = l; }
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    const float i = lw_block_sum(aI[k], red), pp = lw_block_sum(aP[k], red), t3 = lw_block_sum(aT[k], red);
    if (threadIdx.x == 0) { out[3 + k] = i; out[3 + KT + k] = pp; out[3 + 2 * KT + k] = t3; }
  }
}

__global__ void __launch_bounds__(LW_THREADS) lw_dicece_partial_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int K, int64_t HW,
                                         int64_t npix, int64_t ignore_index, const float* __restrict__ weight, LwTerm tm,
                                         int focal, float* ws) {
  __shared__ float red[8];
  __shared__ float sw[LW_MAXK];
  if (threadIdx.x < LW_MAXK) sw[threadIdx.x] = (int)threadIdx.x < K ? (weight ? weight[threadIdx.x] : 1.f) : 0.f;
  __syncthreads();
  float aI[LW_MAXK], aP[LW_MAXK], aT[LW_MAXK];
  float cnt = 0.f, wsum = 0.f, lsum = 0.f;
#pragma unroll
  for (int k = 0; k < LW_MAXK; ++k) { aI[k] = 0.f; aP[k] = 0.f; aT[k] = 0.f; }
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t64 = target[p];
    if (!lw_valid(t64, ignore_index, K)) continue;
    const int t = (int)t64;
    const int64_t n = p / HW, hw = p - n * HW;
    const float* lp = logits + n * K * HW + hw;
    float v[LW_MAXK], e[LW_MAXK];
#pragma unroll
    for (int k = 0; k < LW_MAXK; ++k) v[k] = k < K ? lp[k * HW] : 0.f;
    float mx = v[0];
#pragma unroll
    for (int k = 1; k < LW_MAXK; ++k) if (k < K) mx = fmaxf(mx, v[k]);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < LW_MAXK; ++k) { e[k] = k < K ? __expf(v[k] - mx) : 0.f; se += e[k]; }
    const float rse = 1.f / se, lg = __logf(se), wy = sw[t];
    cnt += 1.f;
    wsum += wy;
    lsum += focal ? lw_pixel_num<LW_MAXK, true>(v, e, K, t, wy, sw, mx, rse, lg, tm)
                  : lw_pixel_num<LW_MAXK, false>(v, e, K, t, wy, sw, mx, rse, lg, tm);
#pragma unroll
    for (int k = 0; k < LW_MAXK; ++k) {
      if (k < K) {
        const float pr = e[k] * rse;
        aP[k] += pr;
        if (k == t) { aI[k] += pr; aT[k] += 1.f; }
      }
    }
  }
  float* out = ws + LW_HEAD + 3 * K + (int64_t)blockIdx.x * LW_BLK(K);
  const float c = lw_block_sum(cnt, red), ww = lw_block_sum(wsum, red), l = lw_block_sum(lsum, red);
  if (threadIdx.x == 0) { out[0] = c; out[1] = ww; out[2] = l; }
#pragma unroll
  for (int k = 0; k < LW_MAXK; ++k) {
    if (k < K) {
      const float i = lw_block_sum(aI[k], red), pp = lw_block_sum(aP[k], red), t3 = lw_block_sum(aT[k], red);
      if (threadIdx.x == 0) { out[3 + k] = i; out[3 + K + k] = pp; out[3 + 2 * K + k] = t3; }
    }
  }
}

__global__ void lw_dicece_final_kernel(float* ws, int K, int nb, float smooth, float ce_w, float dice_w, int focal, float* loss_out) {
  __shared__ float red[8];
  __shared__ float tot[LW_BLK(LW_MAXK)];
  const int stride = LW_BLK(K);
  // as dicece_final_kernel: every partial this thread folds is requested before the first block sum (one round trip)
  constexpr int QM = LW_BLK(4);
  if (stride <= QM && nb <= 4 * (int)blockDim.x) {
    float v[4][QM];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = threadIdx.x + r * blockDim.x;
#pragma unroll
      for (int q = 0; q < QM; ++q) v[r][q] = (i < nb && q < stride) ? ws[LW_HEAD + 3 * K + (int64_t)i * stride + q] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < QM; ++q) {
      if (q < stride) {                       // uniform
        const float c = lw_block_sum(((v[0][q] + v[1][q]) + v[2][q]) + v[3][q], red);
        if (threadIdx.x == 0) tot[q] = c;
      }
    }
  } else {
    for (int q = 0; q < stride; ++q) {
      float c = 0.f;
      for (int i = threadIdx.x; i < nb; i += blockDim.x) c += ws[LW_HEAD + 3 * K + (int64_t)i * stride + q];
      c = lw_block_sum(c, red);
      if (threadIdx.x == 0) tot[q] = c;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = focal ? tot[0] : tot[1];
    ws[0] = norm; ws[1] = 1.f / norm; ws[2] = tot[2]; ws[3] = tot[0];
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
      ws[LW_HEAD + k] = tot[3 + k]; ws[LW_HEAD + K + k] = tot[3 + K + k]; ws[LW_HEAD + 2 * K + k] = tot[3 + 2 * K + k];
      acc += (2.f * tot[3 + k] + smooth) / (tot[3 + K + k] + tot[3 + 2 * K + k] + smooth);
    }
    const float ce = tot[2] / norm, dice = 1.f - acc / (float)K;
    loss_out[0] = ce_w * ce + dice_w * dice;
    loss_out[1] = ce;
    loss_out[2] = dice;
  }
}

template <int KT, bool FOCAL, int J>
__device__ __forceinline__ void lw_v4_grad(const float4 (&lv)[KT], float4 (&gv)[KT], int64_t t64, int64_t ignore_index,
                                           const float (&w)[KT], float S, LwTerm tm, float inv, float dice_w,
                                           const float (&g0)[KT], const float (&g1)[KT]) {
  const bool ok = lw_valid(t64, ignore_index, KT);            // branchless, as lw_v4_stats
  const int t = ok ? (int)t64 : 0;
  float v[KT], e[KT], o[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) v[k] = lw_get<J>(lv[k]);
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < KT; ++k) mx = fmaxf(mx, v[k]);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) { e[k] = __expf(v[k] - mx); se += e[k]; }
  const float rse = 1.f / se, lg = __logf(se), wy = lw_pick<KT>(w, t);
  lw_pixel_grad<KT, FOCAL>(v, e, KT, t, wy, w, S, mx, rse, lg, tm, inv, o);
  float gk[KT];
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    gk[k] = k == t ? g1[k] : g0[k];
    dot = fmaf(e[k] * rse, gk[k], dot);
  }
#pragma unroll
  for (int k = 0; k < KT; ++k) lw_set<J>(gv[k], ok ? o[k] + dice_w * (e[k] * rse) * (gk[k] - dot) : 0.f);
}

template <int KT, bool FOCAL>
__global__ void __launch_bounds__(LW_THREADS)
lw_dicece_grad_v4(const float* __restrict__ logits, const int64_t* __restrict__ target, int64_t HW, int64_t npix,
                  int64_t ignore_index, const float* __restrict__ weight, LwTerm tm, float smooth, float ce_w, float dice_w,
                  const float* __restrict__ ws, float* __restrict__ dlogits) {
  // dDice/dp_k = -(1/K) (2 [t = k] den - num) / den^2 takes two values per class: both divided out once per thread (the
  // same operations in the same order as dicece_grad_v4 performs per pixel)
  float w[KT], g0[KT], g1[KT];
  float S = 0.f;
  const float inv = ws[1] * ce_w;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    w[k] = weight ? weight[k] : 1.f;
    S += w[k];
    const float num = 2.f * ws[LW_HEAD + k] + smooth;
    const float den = ws[LW_HEAD + KT + k] + ws[LW_HEAD + 2 * KT + k] + smooth;
    g0[k] = -(0.f - num) / (den * den) / (float)KT;
    g1[k] = -(2.f * den - num) / (den * den) / (float)KT;
  }
  const int64_t ngroups = npix >> 2;
  for (int64_t gi = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gi < ngroups; gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = gi << 2;
    const int64_t n = p / HW, hw = p - n * HW;
    const longlong2 t01 = *(const longlong2*)(target + p), t23 = *(const longlong2*)(target + p + 2);
    float4 lv[KT], gv[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) lv[k] = *(const float4*)(logits + (n * KT + k) * HW + hw);
    lw_v4_grad<KT, FOCAL, 0>(lv, gv, t01.x, ignore_index, w, S, tm, inv, dice_w, g0, g1);
    lw_v4_grad<KT, FOCAL, 1>(lv, gv, t01.y, ignore_index, w, S, tm, inv, dice_w, g0, g1);
    lw_v4_grad<KT, FOCAL, 2>(lv, gv, t23.x, ignore_index, w, S, tm, inv, dice_w, g0, g1);
    lw_v4_grad<KT, FOCAL, 3>(lv, gv, t23.y, ignore_index, w, S, tm, inv, dice_w, g0, g1);
#pragma unroll
    for (int k = 0; k < KT; ++k) *(float4*)(dlogits + (n * KT + k) * HW + hw) = gv[k];
  }
}

__global__ void __launch_bounds__(LW_THREADS) lw_dicece_grad_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int K, int64_t HW,
                                      int64_t npix, int64_t ignore_index, const float* __restrict__ weight, LwTerm tm, int focal,
                                      float smooth, float ce_w, float dice_w, const float* __restrict__ ws,
                                      float* __restrict__ dlogits) {
  __shared__ float sw[LW_MAXK];
  if (threadIdx.x < LW_MAXK) sw[threadIdx.x] = (int)threadIdx.x < K ? (weight ? weight[threadIdx.x] : 1.f) : 0.f;
  __syncthreads();
  float num[LW_MAXK], den[LW_MAXK];
  float S = 0.f;
  for (int k = 0; k < K; ++k) S += sw[k];
  const float inv = ws[1] * ce_w;
#pragma unroll
  for (int k = 0; k < LW_MAXK; ++k) {
    num[k] = k < K ? 2.f * ws[LW_HEAD + k] + smooth : 0.f;
    den[k] = k < K ? ws[LW_HEAD + K + k] + ws[LW_HEAD + 2 * K + k] + smooth : 1.f;
  }
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = p / HW, hw = p - n * HW;
    const float* lp = logits + n * K * HW + hw;
    float* gp = dlogits + n * K * HW + hw;
    const int64_t t64 = target[p];
    float v[LW_MAXK], e[LW_MAXK], o[LW_MAXK];
#pragma unroll
    for (int k = 0; k < LW_MAXK; ++k) { v[k] = k < K ? lp[k * HW] : 0.f; o[k] = 0.f; }
    if (lw_valid(t64, ignore_index, K)) {
      const int t = (int)t64;
      float mx = v[0];
#pragma unroll
      for (int k = 1; k < LW_MAXK; ++k) if (k < K) mx = fmaxf(mx, v[k]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < LW_MAXK; ++k) { e[k] = k < K ? __expf(v[k] - mx) : 0.f; se += e[k]; }
      const float rse = 1.f / se, lg = __logf(se), wy = sw[t];
      if (focal) lw_pixel_grad<LW_MAXK, true>(v, e, K, t, wy, sw, S, mx, rse, lg, tm, inv, o);
      else lw_pixel_grad<LW_MAXK, false>(v, e, K, t, wy, sw, S, mx, rse, lg, tm, inv, o);
      float gk[LW_MAXK];
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < LW_MAXK; ++k) {
        if (k < K) {
          gk[k] = -((k == t ? 2.f * den[k] : 0.f) - num[k]) / (den[k] * den[k]) / (float)K;
          dot = fmaf(e[k] * rse, gk[k], dot);
        }
      }
#pragma unroll
      for (int k = 0; k < LW_MAXK; ++k)
        if (k < K) o[k] += dice_w * (e[k] * rse) * (gk[k] - dot);
    }
#pragma unroll
    for (int k = 0; k < LW_MAXK; ++k) if (k < K) gp[k * HW] = o[k];
  }
}

extern "C" int insar_dice_ce_w(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW, int64_t ignore_index,
                               float smooth, float ce_weight, float dice_weight, const float* weight, float label_smoothing,
                               float focal_gamma, float* dlogits, float* loss_out, float* ws, void* stream) {
  if (int rc = lw_check("insar_dice_ce_w", logits, target, dlogits, loss_out, ws, B, K, HW)) return rc;
  const bool focal = focal_gamma >= 0.f;
  if (focal_gamma != focal_gamma || focal_gamma > 64.f)
    INSAR_FAIL(INSAR_E_ARG, "insar_dice_ce_w: focal_gamma=%g must be negative (off) or in [0, 64]", (double)focal_gamma);
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f))
    INSAR_FAIL(INSAR_E_ARG, "insar_dice_ce_w: label_smoothing=%g must be in [0, 1)", (double)label_smoothing);
  if (focal && label_smoothing != 0.f) INSAR_FAIL(INSAR_E_ARG, "insar_dice_ce_w: label smoothing and focal do not combine");
  const int64_t npix = (int64_t)B * HW;
  const int nb = insar_ce_blocks(npix);
  hipStream_t s = (hipStream_t)stream;
  const LwTerm tm = {1.f - label_smoothing, label_smoothing / (float)K, focal ? focal_gamma : 0.f};
  const int fo = focal ? 1 : 0;
  const bool v4 = K >= 2 && K <= 4 && (HW & 3) == 0 && insar_aligned16(logits) && insar_aligned16(target) && insar_aligned16(dlogits);
#define LW_V4(KT, FO)                                                                                                              \
  do {                                                                                                                             \
    hipLaunchKernelGGL((lw_dicece_partial_v4<KT, FO>), dim3(nb), dim3(LW_THREADS), 0, s, logits, target, HW, npix, ignore_index,    \
                       weight, tm, ws);                                                                                             \
    hipLaunchKernelGGL(lw_dicece_final_kernel, dim3(1), dim3(LW_THREADS), 0, s, ws, K, nb, smooth, ce_weight, dice_weight, fo,      \
                       loss_out);                                                                                                   \
    hipLaunchKernelGGL((lw_dicece_grad_v4<KT, FO>), dim3(nb), dim3(LW_THREADS), 0, s, logits, target, HW, npix, ignore_index,       \
                       weight, tm, smooth, ce_weight, dice_weight, ws, dlogits);                                                    \
  } while (0)
  if (v4 && K == 2 && !focal) LW_V4(2, false);
  else if (v4 && K == 2) LW_V4(2, true);
  else if (v4 && K == 3 && !focal) LW_V4(3, false);
  else if (v4 && K == 3) LW_V4(3, true);
  else if (v4 && K == 4 && !focal) LW_V4(4, false);
  else if (v4 && K == 4) LW_V4(4, true);
  else {
    hipLaunchKernelGGL(lw_dicece_partial_kernel, dim3(nb), dim3(LW_THREADS), 0, s, logits, target, K, HW, npix, ignore_index, weight,
                       tm, fo, ws);
    hipLaunchKernelGGL(lw_dicece_final_kernel, dim3(1), dim3(LW_THREADS), 0, s, ws, K, nb, smooth, ce_weight, dice_weight, fo,
                       loss_out);
    hipLaunchKernelGGL(lw_dicece_grad_kernel, dim3(nb), dim3(LW_THREADS), 0, s, logits, target, K, HW, npix, ignore_index, weight, tm,
                       fo, smooth, ce_weight, dice_weight, ws, dlogits);
  }
#undef LW_V4
  INSAR_CHECK_LAUNCH("insar_dice_ce_w");
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// Per-class pixel counts of a mask batch, built like insar_confusion (32-bit LDS counters per block) but folded through
// block partials: counts[c] += pixels of class c (c < K), counts[K] += pixels equal to ignore_index. The call ADDS to
// counts, so a data set is accumulated batch by batch on the device; labels outside [0, K) other than ignore_index are
// counted nowhere (the sum then falls short of npix, which the caller can test). ws: int64[(K + 1) * blocks].
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LW_THREADS) lw_hist_kernel(const int64_t* __restrict__ target, int64_t npix, int K, int64_t ignore_index, int64_t* ws) {
  __shared__ unsigned int sc[LW_MAXK + 1];
  if (threadIdx.x <= LW_MAXK) sc[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = target[p];
    if (t == ignore_index) atomicAdd(&sc[K], 1u);
    else if ((uint64_t)t < (uint64_t)K) atomicAdd(&sc[(int)t], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x <= K) ws[(int64_t)blockIdx.x * (K + 1) + threadIdx.x] = (int64_t)sc[threadIdx.x];
}

__global__ void lw_hist_final_kernel(const int64_t* __restrict__ ws, int K, int nb, int64_t* counts) {
  const int c = threadIdx.x;
  if (c > K) return;
  int64_t s = 0;
  for (int i = 0; i < nb; ++i) s += ws[(int64_t)i * (K + 1) + c];
  counts[c] += s;
}

extern "C" int insar_label_hist(const int64_t* target, int64_t npix, int32_t K, int64_t ignore_index, int64_t* counts,
                                int64_t* ws, void* stream) {
  if (!target || !counts || !ws) INSAR_FAIL(INSAR_E_ARG, "insar_label_hist: null pointer");
  if (K < 1 || K > LW_MAXK) INSAR_FAIL(INSAR_E_SHAPE, "insar_label_hist: num_classes=%d must be 1..%d", K, LW_MAXK);
  if (npix < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_label_hist: bad shape");
  // per-block LDS counters are 32-bit: insar_ce_blocks keeps a block's share of the pixels far below 2^32 for any batch
  const int nb = insar_ce_blocks(npix);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lw_hist_kernel, dim3(nb), dim3(LW_THREADS), 0, s, target, npix, K, ignore_index, ws);
  hipLaunchKernelGGL(lw_hist_final_kernel, dim3(1), dim3(64), 0, s, (const int64_t*)ws, K, nb, counts);
  INSAR_CHECK_LAUNCH("insar_label_hist");
  return INSAR_OK;
}
