// Hysteresis thresholds: a site is a connected component of {score >= low} that holds at least `min_seeds` pixels with
// score >= high. Extent comes from the permissive threshold, existence from the strict one. The rule is DESIGN.md's
// "Hysteresis thresholds"; tests/hysteresis_ref.py restates it in numpy. The components themselves come from regions.hip (the
// five insar_regions_* phases on the candidate map and its confidence plane, with min_conf = -inf so that the labelling drops
// nothing); this file adds the candidate map in front of them and the seed rule behind them. 12 launches per call, whatever
// the map holds, and ONE read-back (the compact table with its header):
//
//   classify  (1)  score planes, thresholds, optional validity -> cand uint8 (class or 0) and conf float32 (the class's score)
//   regions   (7)  insar_regions_tiles / _merge / _flatten / _number / _relabel on cand / conf: labels 1..N by ascending root
//                  over the components of area >= min_area, their InsarRegion table, mask_out = cand where labelled
//   seeds     (2)  clear     the seed table zeroed
//                  seeds     per pixel of the label map: seed = conf >= high[class]; per label the seed count (64-bit integer
//                            add) and the peak key (64-bit integer max)
//   keep      (1)  one work-group: exclusive scan of n_seed >= min_seeds over records 1..N; remap[old id] = new id or 0; the
//                  kept records and their seed fields copied into a SECOND, compact table (never in place: record k may be read
//                  by one thread while another writes its new place), whose header holds N' and N
//   apply     (1)  labels = remap[labels], mask = cand where the new label is not 0
//
// The peak key is (ordered_u32(conf) << 32) | (0xFFFFFFFF - index): ordered_u32 is the order-preserving map of float32 bits
// (all bits of a negative flipped, the sign bit of the rest), so the 64-bit maximum is the exact float32 maximum at the first
// pixel in row-major order that reaches it. No clamp, no quantisation, no float atomics.
// No work-group ever waits on another: the phases are ordered by kernel boundaries on the caller's stream. Visibility: the seed
// table is shared between the work-groups of the seeds launch, so every access to it there is an agent-scope relaxed integer
// atomic; everywhere else a kernel boundary lies between writer and reader.
// Aggregation before atomics: a thread folds those of its four pixels that share a label, the lanes of a wave fold over runs of
// equal labels, and only the first lane of a run touches the table (regions_relabel_kernel's pattern).
// Reproducibility: integer sums and maxima commute; the arrival order of the atomics changes nothing.
#include "scene_common.h"
#include "block_scan.h"
#include <limits.h>

#define HY_THREADS 256
#define HY_KEEP_THREADS 1024
#define HY_MAX_PLANES 255                 // classes 1..255: the candidate map is uint8
#define HY_THR_WORDS 512                  // low[0..255], high[256..511]

struct HySeed { long long n_seed; unsigned long long peak_key; };
static_assert(sizeof(HySeed) == 16, "one 16-byte chunk per seed record");
static_assert(sizeof(InsarRegion) == 64 && sizeof(InsarHystRegion) == 80, "a kept record is an InsarRegion and a seed record");

__device__ __forceinline__ uint32_t hy_ordered_u32(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

// ---------------------------------------------------------------------------------------------
// classify: plane p of `score` belongs to class p + 1. A class that is not selected has low = NaN, which no score reaches.
// `al` has bit 0 set where the base pointers allow 16-byte (4-byte for uint8) accesses; a quad is then vector where it lies
// wholly inside the map, and a plane where its offset p * npix keeps the alignment (every plane when npix % 4 == 0).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HY_THREADS)
hyst_classify_kernel(const float* __restrict__ score, int planes, int64_t npix, int al, const float* __restrict__ thr,
                     const uint8_t* __restrict__ valid, uint8_t* __restrict__ cand, float* __restrict__ conf) {
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q = blockIdx.x * (int64_t)HY_THREADS + threadIdx.x; q < nquads; q += (int64_t)gridDim.x * HY_THREADS) {
    const int64_t i = q << 2;
    const bool full = al && i + 4 <= npix;
    int ok[4] = {1, 1, 1, 1}, c[4] = {0, 0, 0, 0};
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) quad_load_u8(valid, i, npix, full, 0, ok);
    for (int p = 0; p < planes; ++p) {
      const int64_t off = (int64_t)p * npix;
      const float lo = thr[p + 1];
      float v[4];
      quad_load(score + off, i, npix, full && (off & 3) == 0, 0.f, v);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (v[j] >= lo && (c[j] == 0 || v[j] > best[j])) { c[j] = p + 1; best[j] = v[j]; }      // NaN compares false; ties keep the smaller class
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (!ok[j] || i + j >= npix) { c[j] = 0; best[j] = 0.f; }
    quad_store_u8(cand, i, npix, full, c);
    quad_store(conf, i, npix, full, best);
  }
}

// ---------------------------------------------------------------------------------------------
// seeds
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HY_THREADS)
hyst_clear_kernel(int4* __restrict__ seeds, int64_t chunks) {
  for (int64_t i = blockIdx.x * (int64_t)HY_THREADS + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * HY_THREADS)
    seeds[i] = make_int4(0, 0, 0, 0);
}

__global__ void __launch_bounds__(HY_THREADS)
hyst_seeds_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ cand, const float* __restrict__ conf,
                  const float* __restrict__ thr, int64_t npix, int vec, int max_regions, HySeed* seeds) {
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q0 = blockIdx.x * (int64_t)HY_THREADS; q0 < nquads; q0 += (int64_t)gridDim.x * HY_THREADS) {
    const int64_t q = q0 + threadIdx.x;                            // the loop bound is uniform over the block: shuffles below
    int id[4] = {0, 0, 0, 0}, cnt[4];
    long long ns[4] = {0, 0, 0, 0};
    unsigned long long key[4] = {0ull, 0ull, 0ull, 0ull};
    if (q < nquads) {
      const int64_t i = q << 2;
      int l[4], c[4];
      float f[4];
      quad_load(labels, i, npix, vec, 0, l);
      quad_load_u8(cand, i, npix, vec, 0, c);
      quad_load(conf, i, npix, vec, 0.f, f);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (l[j] <= 0 || l[j] > max_regions) continue;             // ids above max_regions are never an index
        id[j] = l[j];
        ns[j] = f[j] >= thr[256 + (c[j] & 255)];
        key[j] = ((unsigned long long)hy_ordered_u32(f[j]) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(i + j));      // i < 2^31
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[j] = id[j] > 0;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (id[j] > 0 && id[j] == id[j - 1]) {
        ns[j] += ns[j - 1];
        key[j] = key[j - 1] > key[j] ? key[j - 1] : key[j];
        cnt[j - 1] = 0;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = cnt[j] > 0 ? id[j] : 0;
      if (__ballot(k > 0) == 0) continue;
      const WaveRuns runs = wave_runs(k);
      const long long n = wave_run_reduce(runs, ns[j], WaveAdd());
      const unsigned long long m = wave_run_reduce(runs, key[j], WaveMax());
      if (runs.head && k > 0) {
        HySeed* s = seeds + k;
        if (n) __hip_atomic_fetch_add(&s->n_seed, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&s->peak_key, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// keep: one work-group. N is the TRUE number of components of area >= min_area, which may exceed max_regions; the scan runs
// over the records that exist, and the header carries N so that the host can refuse the result.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HY_KEEP_THREADS)
hyst_keep_kernel(const InsarRegion* __restrict__ table, const HySeed* __restrict__ seeds, long long min_seeds, int max_regions,
                 int* __restrict__ remap, InsarHystRegion* __restrict__ out) {
  __shared__ int wsum[HY_KEEP_THREADS / INSAR_WAVE];
  const long long N = table[0].area;
  const int n = (int)(N < (long long)max_regions ? N : (long long)max_regions);
  int carry = 0;                                                 // every thread keeps the same running total
  for (int base = 1; base <= n; base += HY_KEEP_THREADS) {
    const int r = base + threadIdx.x;
    HySeed s;
    s.n_seed = 0; s.peak_key = 0ull;
    if (r <= n) s = seeds[r];
    const int keep = r <= n && s.n_seed >= min_seeds;
    int total;
    const int before = block_prefix_sum<HY_KEEP_THREADS>(keep, wsum, &total);
    if (r <= n) {
      const int id = keep ? carry + before + 1 : 0;              // 1 <= id <= r: the compact table is never overrun
      remap[r] = id;
      if (keep) {
        const int4* src = reinterpret_cast<const int4*>(table + r);
        int4* dst = reinterpret_cast<int4*>(out + id);
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = src[k];
        dst[4] = make_int4((int)(uint32_t)s.n_seed, (int)(s.n_seed >> 32), (int)(uint32_t)s.peak_key, (int)(s.peak_key >> 32));
      }
    }
    carry += total;
  }
  if (threadIdx.x == 0) remap[0] = 0;
  if (threadIdx.x < 5) {                                         // header record: {N', N, 0, ...}
    int4 h = make_int4(0, 0, 0, 0);
    if (threadIdx.x == 0) h = make_int4(carry, 0, (int)(N & 0xffffffffll), (int)(N >> 32));
    reinterpret_cast<int4*>(out)[threadIdx.x] = h;
  }
}

// ---------------------------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HY_THREADS)
hyst_apply_kernel(int* __restrict__ labels, const uint8_t* __restrict__ cand, const int* __restrict__ remap, int64_t npix, int vec,
                  int max_regions, uint8_t* __restrict__ mask) {
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q = blockIdx.x * (int64_t)HY_THREADS + threadIdx.x; q < nquads; q += (int64_t)gridDim.x * HY_THREADS) {
    const int64_t i = q << 2;
    int l[4], c[4];
    quad_load(labels, i, npix, vec, 0, l);
    quad_load_u8(cand, i, npix, vec, 0, c);
    int o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j > 0 && l[j] == l[j - 1]) o[j] = o[j - 1];              // neighbours mostly share a label: one look-up
      else o[j] = (l[j] > 0 && l[j] <= max_regions) ? remap[l[j]] : 0;
      if (!o[j]) c[j] = 0;
    }
    quad_store(labels, i, npix, vec, o);
    quad_store_u8(mask, i, npix, vec, c);
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct HyLayout { int64_t npix, seed_bytes, off_remap, scratch_bytes, table_bytes; };

static int hyst_layout(const char* who, int32_t H, int32_t W, int32_t max_regions, HyLayout* L) {
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  const int64_t npix = (int64_t)H * W;
  if (npix >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^31 pixels or more", who, H, W);
  if (max_regions < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d < 1", who, max_regions);
  const int64_t recs = (int64_t)max_regions + 1;
  L->npix = npix;
  L->seed_bytes = recs * (int64_t)sizeof(HySeed);
  L->off_remap = L->seed_bytes;
  L->scratch_bytes = L->off_remap + insar_align16(recs * 4);
  L->table_bytes = recs * (int64_t)sizeof(InsarHystRegion);
  return INSAR_OK;
}
static inline bool hy_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

extern "C" int insar_hyst_scratch_bytes(int32_t H, int32_t W, int32_t max_regions, int64_t* scratch_bytes, int64_t* table_bytes) {
  const char* who = "insar_hyst_scratch_bytes";
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  HyLayout L;
  if (int rc = hyst_layout(who, H, W, max_regions, &L)) return rc;
  *scratch_bytes = L.scratch_bytes;
  *table_bytes = L.table_bytes;
  return INSAR_OK;
}

extern "C" int insar_hyst_classify(const float* score, int32_t planes, int32_t H, int32_t W, const float* thresholds,
                                   const uint8_t* valid, uint8_t* cand, float* conf, void* stream) {
  const char* who = "insar_hyst_classify";
  if (int rc = scene_check_map(who, "score", score, 4)) return rc;
  if (int rc = scene_check_map(who, "thresholds", thresholds, 4)) return rc;
  if (int rc = scene_check_map(who, "cand", cand, 1)) return rc;
  if (int rc = scene_check_map(who, "conf", conf, 4)) return rc;
  HyLayout L;
  if (int rc = hyst_layout(who, H, W, 1, &L)) return rc;
  if (planes < 1 || planes > HY_MAX_PLANES) INSAR_FAIL(INSAR_E_SHAPE, "%s: %d planes outside 1..%d", who, planes, HY_MAX_PLANES);
  const int al = insar_aligned16(score) && insar_aligned16(conf) && hy_aligned4(cand) && hy_aligned4(valid);
  hipLaunchKernelGGL(hyst_classify_kernel, scene_grid((L.npix + 3) / 4, HY_THREADS), dim3(HY_THREADS), 0, (hipStream_t)stream, score, (int)planes,
                     L.npix, al, thresholds, valid, cand, conf);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_hyst_seeds(const int32_t* labels, const uint8_t* cand, const float* conf, const float* thresholds, int32_t H,
                                int32_t W, int32_t max_regions, void* scratch, void* stream) {
  const char* who = "insar_hyst_seeds";
  if (int rc = scene_check_map(who, "labels", labels, 4)) return rc;
  if (int rc = scene_check_map(who, "cand", cand, 1)) return rc;
  if (int rc = scene_check_map(who, "conf", conf, 4)) return rc;
  if (int rc = scene_check_map(who, "thresholds", thresholds, 4)) return rc;
  HyLayout L;
  if (int rc = hyst_layout(who, H, W, max_regions, &L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = L.seed_bytes / 16;
  hipLaunchKernelGGL(hyst_clear_kernel, scene_grid(chunks, HY_THREADS), dim3(HY_THREADS), 0, s, (int4*)scratch, chunks);
  INSAR_CHECK_LAUNCH(who);
  const int vec = (L.npix % 4 == 0) && insar_aligned16(labels) && insar_aligned16(conf) && hy_aligned4(cand);
  hipLaunchKernelGGL(hyst_seeds_kernel, scene_grid((L.npix + 3) / 4, HY_THREADS), dim3(HY_THREADS), 0, s, (const int*)labels, cand, conf, thresholds,
                     L.npix, vec, (int)max_regions, (HySeed*)scratch);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_hyst_keep(const void* regions, int64_t min_seeds, int32_t max_regions, void* scratch, void* table, void* stream) {
  const char* who = "insar_hyst_keep";
  if (int rc = scene_check_buffer(who, "regions", regions)) return rc;
  HyLayout L;
  if (int rc = hyst_layout(who, 1, 1, max_regions, &L)) return rc;
  if (min_seeds < 1) INSAR_FAIL(INSAR_E_ARG, "%s: min_seeds %lld < 1", who, (long long)min_seeds);
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  if (table == regions) INSAR_FAIL(INSAR_E_ARG, "%s: the compact table must not be the region table", who);
  hipLaunchKernelGGL(hyst_keep_kernel, dim3(1), dim3(HY_KEEP_THREADS), 0, (hipStream_t)stream, (const InsarRegion*)regions,
                     (const HySeed*)scratch, (long long)min_seeds, (int)max_regions, (int*)((char*)scratch + L.off_remap),
                     (InsarHystRegion*)table);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_hyst_apply(const uint8_t* cand, int32_t H, int32_t W, int32_t max_regions, const void* scratch, int32_t* labels,
                                uint8_t* mask, void* stream) {
  const char* who = "insar_hyst_apply";
  if (int rc = scene_check_map(who, "cand", cand, 1)) return rc;
  if (int rc = scene_check_map(who, "labels", labels, 4)) return rc;
  if (int rc = scene_check_map(who, "mask", mask, 1)) return rc;
  HyLayout L;
  if (int rc = hyst_layout(who, H, W, max_regions, &L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  const int vec = (L.npix % 4 == 0) && insar_aligned16(labels) && hy_aligned4(cand) && hy_aligned4(mask);
  hipLaunchKernelGGL(hyst_apply_kernel, scene_grid((L.npix + 3) / 4, HY_THREADS), dim3(HY_THREADS), 0, (hipStream_t)stream, (int*)labels, cand,
                     (const int*)((const char*)scratch + L.off_remap), L.npix, vec, (int)max_regions, mask);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
