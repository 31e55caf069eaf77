// Statistics of a raster over the regions of a label map: for every label 1..max_regions and every channel of the raster
// the number of valid, invalid and clipped pixels, the sum and the EXACT square sum of the quantised values, the minimum and
// the maximum with the row-major index of the first pixel that reaches each, and optionally a histogram. Two launches per
// call whatever the map holds:
//
//   clear       the table zeroed, the minimum keys set to all ones
//   accumulate  one pass over labels and raster; every update of the table is an integer atomic
//
// Quantisation: integer rasters q = v; float32 q = rint(clamp((double)v * scale, -(2^31 - 1), 2^31 - 1)), to nearest even (the
// rule of regions.hip's confidence, generalised). A product outside the clamp counts as clipped and takes part with the clamped
// q; a pixel that is not finite, or equals `nodata` in the raster's own type, counts as invalid and takes no other part.
// Square sum: q^2 < 2^62 and fewer than 2^31 pixels need 93 bits. The low and the high 32 bits of q^2 are summed in two 64-bit
// words (each stays below 2^63), the host forms lo + (hi << 32) in integers: exact whatever the order.
// Extremes: one 64-bit key per extreme with the biased value (q ^ 2^31 as uint32) in the high word; the low word holds idx
// for the minimum (atomic min: ties go to the smallest index) and ~idx for the maximum (atomic max: the same).
// Folding before the global atomics, four levels:
//   thread      four consecutive pixels; neighbours with equal labels are merged
//   wave        runs of equal labels over the lanes (wave_runs / wave_run_reduce with add, min, max); only the head lane of a
//               run goes on
//   work-group  ONE label per work-group, the `hot` label, has a record per channel (and a histogram) in LDS; heads of that
//               label use LDS atomics. Each pass over 1024 pixels votes (an LDS atomic max of run length << 32 | label over
//               the waves' longest whole-thread runs); when the vote changes the label, the LDS record is flushed to the table.
//               A map that is one region therefore sends one record per work-group and channel to the table, not one per wave
//               and pass.
//   table       agent-scope relaxed integer atomics (the rule of overlap.hip and skeleton.hip): work-groups on different XCDs
//               add to the same records, and nothing in this kernel reads the table.
// Histogram counts of labels other than the hot one are added per pixel. No work-group waits on another, no float atomics,
// nothing is read back before the table. Labels above max_regions are counted in the header and are never an index.
#include <stddef.h>
#include "scene_common.h"

#define ZN_THREADS 256
#define ZN_MAX_CH 4
#define ZN_MAX_BINS 256
#define ZN_MAX_REGIONS (1 << 24)
#define ZN_LIMIT 2147483647.0

static_assert(sizeof(InsarZonalStat) == 64, "InsarZonalStat is four 16-byte chunks");
static_assert(offsetof(InsarZonalStat, min_key) == 24, "the clear kernel sets the upper half of chunk 1");

// what one pixel, one run or the LDS record holds; the counts of a thread or wave run are packed 12 bits each (<= 256 pixels)
struct ZnAcc {
  unsigned long long cnt;          // n | n_invalid << 12 | n_clipped << 24 | below << 36 | above << 48
  long long sum;
  unsigned long long sqlo, sqhi, mink, maxk;
};
struct ZnHot {
  unsigned int n, n_invalid, n_clipped, below, above, _pad;
  long long sum;
  unsigned long long sqlo, sqhi, mink, maxk;
};

__device__ __forceinline__ void zn_merge(ZnAcc& into, const ZnAcc& a) {
  into.cnt += a.cnt;
  into.sum += a.sum;
  into.sqlo += a.sqlo;
  into.sqhi += a.sqhi;
  into.mink = a.mink < into.mink ? a.mink : into.mink;
  into.maxk = a.maxk > into.maxk ? a.maxk : into.maxk;
}

#define ZN_ADD(p, v, scope) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, scope)
#define ZN_MIN(p, v, scope) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, scope)
#define ZN_MAX(p, v, scope) __hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, scope)

// one contribution into a record of the table: agent-scope atomics only, none for a field that would not change
__device__ __forceinline__ void zn_commit(InsarZonalStat* r, unsigned int n, unsigned int ninv, unsigned int nclip, unsigned int below,
                                          unsigned int above, long long sum, unsigned long long sqlo, unsigned long long sqhi,
                                          unsigned long long mink, unsigned long long maxk) {
  if (ninv) ZN_ADD(&r->n_invalid, (int)ninv, __HIP_MEMORY_SCOPE_AGENT);
  if (!n) return;
  ZN_ADD(&r->n, (int)n, __HIP_MEMORY_SCOPE_AGENT);
  if (nclip) ZN_ADD(&r->n_clipped, (int)nclip, __HIP_MEMORY_SCOPE_AGENT);
  if (below) ZN_ADD(&r->below, below, __HIP_MEMORY_SCOPE_AGENT);
  if (above) ZN_ADD(&r->above, above, __HIP_MEMORY_SCOPE_AGENT);
  if (sum) ZN_ADD(reinterpret_cast<long long*>(&r->sum_q), sum, __HIP_MEMORY_SCOPE_AGENT);
  if (sqlo) ZN_ADD(reinterpret_cast<unsigned long long*>(&r->sumsq_lo), sqlo, __HIP_MEMORY_SCOPE_AGENT);
  if (sqhi) ZN_ADD(reinterpret_cast<unsigned long long*>(&r->sumsq_hi), sqhi, __HIP_MEMORY_SCOPE_AGENT);
  ZN_MIN(reinterpret_cast<unsigned long long*>(&r->min_key), mink, __HIP_MEMORY_SCOPE_AGENT);
  ZN_MAX(reinterpret_cast<unsigned long long*>(&r->max_key), maxk, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void zn_hot_reset(ZnHot* h) {
  h->n = h->n_invalid = h->n_clipped = h->below = h->above = h->_pad = 0u;
  h->sum = 0ll;
  h->sqlo = h->sqhi = h->maxk = 0ull;
  h->mink = ~0ull;
}

// four raster elements as values the quantiser takes; elements past the end are never looked at (their label is background)
template <typename T> struct ZnRaster;
template <> struct ZnRaster<float> {
  typedef float V;
  __device__ __forceinline__ static void load(const float* p, int64_t i, int64_t n, bool vec, V* v) { quad_load(p, i, n, vec, 0.0f, v); }
  __device__ __forceinline__ static bool quantise(V v, double scale, bool has_nodata, double nodata, int* q, bool* clipped) {
    if (!(fabsf(v) <= 3.402823466e38f) || (has_nodata && v == (float)nodata)) return false;
    double d = (double)v * scale;
    *clipped = d > ZN_LIMIT || d < -ZN_LIMIT;
    d = d > ZN_LIMIT ? ZN_LIMIT : d < -ZN_LIMIT ? -ZN_LIMIT : d;
    *q = (int)rint(d);                                           // nearest even; |d| <= 2^31 - 1 fits
    return true;
  }
};
template <> struct ZnRaster<int> {
  typedef int V;
  __device__ __forceinline__ static void load(const int* p, int64_t i, int64_t n, bool vec, V* v) { quad_load(p, i, n, vec, 0, v); }
  __device__ __forceinline__ static bool quantise(V v, double, bool has_nodata, double nodata, int* q, bool* clipped) {
    if (has_nodata && v == (int)nodata) return false;
    *clipped = false;
    *q = v;
    return true;
  }
};
template <> struct ZnRaster<uint8_t> {
  typedef int V;
  __device__ __forceinline__ static void load(const uint8_t* p, int64_t i, int64_t n, bool vec, V* v) { quad_load_u8(p, i, n, vec, 0, v); }
  __device__ __forceinline__ static bool quantise(V v, double s, bool has_nodata, double nodata, int* q, bool* clipped) {
    return ZnRaster<int>::quantise(v, s, has_nodata, nodata, q, clipped);
  }
};

// floor(num / den) for 0 <= num < 2^42, 1 <= den <= 2^32: the double quotient is off by at most one, the products decide
__device__ __forceinline__ int zn_bin(long long num, long long den) {
  long long b = (long long)((double)num / (double)den);
  if (b * den > num) --b;
  else if ((b + 1) * den <= num) ++b;
  return (int)b;
}

__global__ void __launch_bounds__(ZN_THREADS)
zonal_clear_kernel(int4* __restrict__ table, int64_t stat_chunks, int64_t chunks) {
  for (int64_t i = blockIdx.x * (int64_t)ZN_THREADS + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * ZN_THREADS) {
    // chunk 1 of a record is {sumsq_hi, min_key}; the header (chunks 0..3) and the histograms are all zero
    const bool mink = i >= 4 && i < stat_chunks && (i & 3) == 1;
    table[i] = mink ? make_int4(0, 0, -1, -1) : make_int4(0, 0, 0, 0);
  }
}

template <typename T>
__global__ void __launch_bounds__(ZN_THREADS)
zonal_accumulate_kernel(const int* __restrict__ labels, const T* __restrict__ raster, int channels, int64_t npix, int vec, double scale,
                        int has_nodata, double nodata, int bins, long long q_lo, long long q_hi, int max_regions,
                        InsarZonalStat* table, unsigned int* hist) {
  __shared__ ZnHot hot_rec[ZN_MAX_CH];
  __shared__ unsigned int hot_hist[ZN_MAX_CH * ZN_MAX_BINS];
  __shared__ unsigned long long vote[2];
  const int tid = threadIdx.x;
  if (tid < ZN_MAX_CH) zn_hot_reset(&hot_rec[tid]);
  if (tid < 2) vote[tid] = 0ull;
  if (bins)
    for (int i = tid; i < channels * bins; i += ZN_THREADS) hot_hist[i] = 0u;
  __syncthreads();

  InsarZonalStat* stats = table + 1;
  const int64_t nquads = (npix + 3) >> 2;
  const long long width = q_hi - q_lo;
  int hot = 0;                                                   // uniform over the work-group: every thread reads the same vote
  int par = 0;
  int oor = 0;
  for (int64_t q0 = blockIdx.x * (int64_t)ZN_THREADS; q0 < nquads; q0 += (int64_t)gridDim.x * ZN_THREADS, par ^= 1) {
    const int64_t qd = q0 + tid;                                 // the loop bound is uniform over the block: shuffles, barriers
    const int64_t i0 = qd << 2;
    int key[4] = {0, 0, 0, 0};
    if (qd < nquads) {
      int l[4];
      quad_load(labels, i0, npix, vec, 0, l);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        oor += l[j] > max_regions;
        key[j] = (l[j] > 0 && l[j] <= max_regions) ? l[j] : 0;
      }
    }
    // slot j of a thread ends up holding the pixels j, j - 1, ... that share its label; `fold[j]`: slot j - 1 goes into slot j
    bool fold[4];
    int kk[4], npx[4];
    fold[0] = false;
#pragma unroll
    for (int j = 1; j < 4; ++j) fold[j] = key[j] != 0 && key[j] == key[j - 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) npx[j] = key[j] != 0;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (fold[j]) npx[j] += npx[j - 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) kk[j] = (j < 3 && fold[j + 1]) ? 0 : key[j];
    const bool any = (key[0] | key[1] | key[2] | key[3]) != 0;
    WaveRuns runs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) runs[j] = wave_runs(kk[j]);

    // ---- the vote: the longest run of whole-thread slots (slot 3) of each wave ----
    {
      const int len = wave_run_reduce(runs[3], kk[3] ? npx[3] : 0, WaveAdd());
      const unsigned long long best =
          wave_max(runs[3].head && kk[3] ? ((unsigned long long)(unsigned int)len << 32) | (unsigned int)kk[3] : 0ull);
      if (runs[3].lane == 0 && best) ZN_MAX(&vote[par], best, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();                                             // A: the votes are in; the LDS adds of the pass before are done
    const unsigned long long won = vote[par];
    const int next_hot = won ? (int)(unsigned int)won : hot;     // a pass without a candidate keeps the label
    if (next_hot != hot && hot != 0) {
      if (tid < channels) {
        ZnHot* h = &hot_rec[tid];
        zn_commit(stats + (int64_t)tid * max_regions + (hot - 1), h->n, h->n_invalid, h->n_clipped, h->below, h->above, h->sum, h->sqlo,
                  h->sqhi, h->mink, h->maxk);
        zn_hot_reset(h);
      }
      if (bins)
        for (int i = tid; i < channels * bins; i += ZN_THREADS) {
          const unsigned int v = hot_hist[i];
          if (v) {
            const int c = i / bins, b = i - c * bins;
            ZN_ADD(hist + ((int64_t)c * max_regions + (hot - 1)) * bins + b, v, __HIP_MEMORY_SCOPE_AGENT);
            hot_hist[i] = 0u;
          }
        }
    }
    if (tid == 0) vote[par ^ 1] = 0ull;                          // read last before barrier B of the pass before, voted on after this B
    __syncthreads();                                             // B: the LDS record belongs to next_hot
    hot = next_hot;

    for (int c = 0; c < channels; ++c) {
      ZnAcc a[4];
      typename ZnRaster<T>::V v[4];
      if (any) ZnRaster<T>::load(raster + (int64_t)c * npix, i0, npix, vec, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j].cnt = 0ull; a[j].sum = 0ll; a[j].sqlo = 0ull; a[j].sqhi = 0ull; a[j].mink = ~0ull; a[j].maxk = 0ull;
        if (key[j] == 0) continue;
        int q = 0;
        bool clipped = false;
        if (!ZnRaster<T>::quantise(v[j], scale, has_nodata != 0, nodata, &q, &clipped)) {
          a[j].cnt = 1ull << 12;
          continue;
        }
        const unsigned int idx = (unsigned int)(i0 + j);
        const unsigned long long biased = (unsigned long long)((unsigned int)q ^ 0x80000000u) << 32;
        const unsigned long long sq = (unsigned long long)((long long)q * (long long)q);
        a[j].cnt = 1ull | ((unsigned long long)clipped << 24);
        a[j].sum = q;
        a[j].sqlo = sq & 0xffffffffull;
        a[j].sqhi = sq >> 32;
        a[j].mink = biased | idx;
        a[j].maxk = biased | (unsigned int)~idx;
        if (bins) {
          if (q < q_lo) a[j].cnt |= 1ull << 36;
          else if (q >= q_hi) a[j].cnt |= 1ull << 48;
          else {
            const int b = zn_bin(((long long)q - q_lo) * bins, width);
            if (key[j] == hot) ZN_ADD(&hot_hist[c * bins + b], 1u, __HIP_MEMORY_SCOPE_WORKGROUP);
            else ZN_ADD(hist + ((int64_t)c * max_regions + (key[j] - 1)) * bins + b, 1u, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
#pragma unroll
      for (int j = 1; j < 4; ++j)
        if (fold[j]) zn_merge(a[j], a[j - 1]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (__ballot(kk[j] != 0) == 0) continue;
        const WaveRuns& r = runs[j];
        const unsigned long long cnt = wave_run_reduce(r, kk[j] ? a[j].cnt : 0ull, WaveAdd());
        const long long sum = wave_run_reduce(r, kk[j] ? a[j].sum : 0ll, WaveAdd());
        const unsigned long long sqlo = wave_run_reduce(r, kk[j] ? a[j].sqlo : 0ull, WaveAdd());
        const unsigned long long sqhi = wave_run_reduce(r, kk[j] ? a[j].sqhi : 0ull, WaveAdd());
        const unsigned long long mink = wave_run_reduce(r, kk[j] ? a[j].mink : ~0ull, WaveMin());
        const unsigned long long maxk = wave_run_reduce(r, kk[j] ? a[j].maxk : 0ull, WaveMax());
        if (!r.head || kk[j] == 0) continue;
        const unsigned int n = (unsigned int)(cnt & 4095u), ninv = (unsigned int)((cnt >> 12) & 4095u);
        const unsigned int nclip = (unsigned int)((cnt >> 24) & 4095u), below = (unsigned int)((cnt >> 36) & 4095u);
        const unsigned int above = (unsigned int)((cnt >> 48) & 4095u);
        if (kk[j] == hot) {
          ZnHot* h = &hot_rec[c];
          if (ninv) ZN_ADD(&h->n_invalid, ninv, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (n) {
            ZN_ADD(&h->n, n, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (nclip) ZN_ADD(&h->n_clipped, nclip, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (below) ZN_ADD(&h->below, below, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (above) ZN_ADD(&h->above, above, __HIP_MEMORY_SCOPE_WORKGROUP);
            ZN_ADD(&h->sum, sum, __HIP_MEMORY_SCOPE_WORKGROUP);
            ZN_ADD(&h->sqlo, sqlo, __HIP_MEMORY_SCOPE_WORKGROUP);
            ZN_ADD(&h->sqhi, sqhi, __HIP_MEMORY_SCOPE_WORKGROUP);
            ZN_MIN(&h->mink, mink, __HIP_MEMORY_SCOPE_WORKGROUP);
            ZN_MAX(&h->maxk, maxk, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        } else {
          zn_commit(stats + (int64_t)c * max_regions + (kk[j] - 1), n, ninv, nclip, below, above, sum, sqlo, sqhi, mink, maxk);
        }
      }
    }
  }
  __syncthreads();                                               // the LDS adds of the last pass are done
  if (hot != 0) {
    if (tid < channels) {
      const ZnHot* h = &hot_rec[tid];
      zn_commit(stats + (int64_t)tid * max_regions + (hot - 1), h->n, h->n_invalid, h->n_clipped, h->below, h->above, h->sum, h->sqlo,
                h->sqhi, h->mink, h->maxk);
    }
    if (bins)
      for (int i = tid; i < channels * bins; i += ZN_THREADS) {
        const unsigned int v = hot_hist[i];
        if (v) {
          const int c = i / bins, b = i - c * bins;
          ZN_ADD(hist + ((int64_t)c * max_regions + (hot - 1)) * bins + b, v, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
  }
  // header: the pixels whose label exceeds max_regions, one add per wave that saw any
#pragma unroll
  for (int o = INSAR_WAVE / 2; o > 0; o >>= 1) oor += __shfl_xor(oor, o, INSAR_WAVE);
  if ((int)__lane_id() == 0 && oor) ZN_ADD(reinterpret_cast<long long*>(&table[0].sum_q), (long long)oor, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct ZnLayout { int64_t stat_bytes, bytes; };

static int zonal_layout(const char* who, int32_t max_regions, int32_t bins, int32_t channels, ZnLayout* l) {
  if (max_regions < 1 || max_regions > ZN_MAX_REGIONS)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d outside 1..%d", who, max_regions, ZN_MAX_REGIONS);
  if (bins < 0 || bins > ZN_MAX_BINS) INSAR_FAIL(INSAR_E_SHAPE, "%s: bins %d outside 0..%d", who, bins, ZN_MAX_BINS);
  if (channels < 1 || channels > ZN_MAX_CH) INSAR_FAIL(INSAR_E_SHAPE, "%s: channels %d outside 1..%d", who, channels, ZN_MAX_CH);
  l->stat_bytes = (int64_t)sizeof(InsarZonalStat) * (1 + (int64_t)channels * max_regions);
  l->bytes = l->stat_bytes + ((4 * (int64_t)channels * max_regions * bins + 15) & ~(int64_t)15);
  return INSAR_OK;
}
static int zonal_check_table(const char* who, const void* table) {
  if (!table) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (table)", who);
  if (!insar_aligned16(table)) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 16-byte aligned", who);
  return INSAR_OK;
}

extern "C" int insar_zonal_scratch_bytes(int32_t max_regions, int32_t bins, int32_t channels, int64_t* table_bytes) {
  const char* who = "insar_zonal_scratch_bytes";
  if (!table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  ZnLayout l;
  if (int rc = zonal_layout(who, max_regions, bins, channels, &l)) return rc;
  *table_bytes = l.bytes;
  return INSAR_OK;
}

extern "C" int insar_zonal_clear(void* table, int32_t max_regions, int32_t bins, int32_t channels, void* stream) {
  const char* who = "insar_zonal_clear";
  ZnLayout l;
  if (int rc = zonal_layout(who, max_regions, bins, channels, &l)) return rc;
  if (int rc = zonal_check_table(who, table)) return rc;
  const int64_t chunks = l.bytes / 16;
  hipLaunchKernelGGL(zonal_clear_kernel, dim3(insar_grid_cap((chunks + ZN_THREADS - 1) / ZN_THREADS)), dim3(ZN_THREADS), 0,
                     (hipStream_t)stream, (int4*)table, l.stat_bytes / 16, chunks);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_zonal_accumulate(const int32_t* labels, const void* raster, int32_t elem_type, int32_t channels, int32_t H,
                                      int32_t W, double scale, int32_t has_nodata, double nodata, int32_t bins, int64_t q_lo,
                                      int64_t q_hi, int32_t max_regions, void* table, void* stream) {
  const char* who = "insar_zonal_accumulate";
  if (!labels || !raster) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !labels ? "labels" : "raster");
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty map %d x %d", who, H, W);
  const int64_t npix = (int64_t)H * W;
  if (npix >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: map %d x %d has 2^31 pixels or more", who, H, W);
  ZnLayout l;
  if (int rc = zonal_layout(who, max_regions, bins, channels, &l)) return rc;
  if (int rc = zonal_check_table(who, table)) return rc;
  if (elem_type != INSAR_ZONAL_F32 && elem_type != INSAR_ZONAL_U8 && elem_type != INSAR_ZONAL_I32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: element type %d", who, elem_type);
  if (!(scale > 0.0) || !(scale <= 1.7976931348623157e308)) INSAR_FAIL(INSAR_E_ARG, "%s: scale %g: positive and finite", who, scale);
  if (has_nodata && nodata != nodata) INSAR_FAIL(INSAR_E_ARG, "%s: nodata is NaN", who);
  if (has_nodata && elem_type != INSAR_ZONAL_F32 && (nodata != (double)(int64_t)nodata || nodata < -2147483648.0 || nodata > 2147483647.0))
    INSAR_FAIL(INSAR_E_ARG, "%s: nodata %g is no value of an integer raster", who, nodata);
  const int64_t lim = 2147483647;
  if (bins && (q_lo >= q_hi || q_lo < -lim - 1 || q_hi > lim + 1))
    INSAR_FAIL(INSAR_E_ARG, "%s: histogram range %lld..%lld: q_lo < q_hi inside -2^31..2^31", who, (long long)q_lo, (long long)q_hi);
  const bool wide = elem_type != INSAR_ZONAL_U8;
  if ((((uintptr_t)labels) & 3u) || (wide && (((uintptr_t)raster) & 3u)))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: labels / raster not 4-byte aligned", who);
  const int vec = (npix % 4 == 0) && insar_aligned16(labels) && (wide ? insar_aligned16(raster) : ((((uintptr_t)raster) & 3u) == 0));
  const int64_t passes = (npix / 4 + ZN_THREADS) / ZN_THREADS;
  const dim3 grid(insar_grid_cap(passes, 4 * insar_num_cus())), block(ZN_THREADS);
  InsarZonalStat* t = (InsarZonalStat*)table;
  unsigned int* hist = (unsigned int*)((char*)table + l.stat_bytes);
#define ZN_LAUNCH(T)                                                                                                              \
  hipLaunchKernelGGL(zonal_accumulate_kernel<T>, grid, block, 0, (hipStream_t)stream, (const int*)labels, (const T*)raster, (int)channels, \
                     npix, vec, scale, (int)has_nodata, nodata, (int)bins, (long long)q_lo, (long long)q_hi, (int)max_regions, t, hist)
  if (elem_type == INSAR_ZONAL_F32) ZN_LAUNCH(float);
  else if (elem_type == INSAR_ZONAL_U8) ZN_LAUNCH(uint8_t);
  else ZN_LAUNCH(int);
#undef ZN_LAUNCH
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
