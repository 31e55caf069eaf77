// Overlaps of two label maps: for every pair (p, g) = (pred[i], gt[i]) != (0, 0) over the pixels of a scene that a void map
// does not drop, the number of pixels that carry it. The rows (p, 0) and columns (0, g) are part of the table, so every area
// after voiding follows from it. Three launches per call:
//
//   clear    zeroes the hash table and the header of the output
//   count    open addressing in global memory: slot = {uint64 key = p << 32 | g, int64 count}, key 0 = empty ((0, 0) is never
//            inserted). A slot is claimed with a 64-bit compare-and-swap on the key (yours if it held 0 or your key, else the
//            next slot), then the count takes an integer atomic add. The probe loop is bounded by the capacity; when it runs
//            out it raises the overflow word of the table header and drops the contribution. No thread waits for another.
//   compact  the non-empty slots as 16-byte records {int32 pred, int32 gt, int64 count} behind the header {int64 n_keys,
//            int64 overflow}; never more than max_pairs records, but n_keys is the true number of keys.
//
// Visibility (the rule of regions_merge_kernel): in `count`, work-groups on different XCDs claim and add to the same slots,
// so EVERY access to the table there is an agent-scope atomic (relaxed load / compare-exchange / fetch_add); there is no plain
// load of it in that kernel. `clear` and `compact` lie behind kernel boundaries and use plain accesses (compact's cursor, the
// n_keys word of the output, is an atomic of its own launch).
// Aggregation before atomics (the pattern of regions_relabel_kernel): a thread merges those of its four pixels that share a
// key, the lanes of a wave reduce over runs of equal keys with shuffles, only the first lane of a run probes and adds.
// Reproducibility: which slot a key lands in depends on arrival order, the counts (integer sums) do not; the host sorts the
// records by (gt, pred).
#include "scene_common.h"

#define OV_THREADS 256
#define OV_MAX_PAIRS ((int64_t)1 << 24)

struct OvSlot { unsigned long long key; long long count; };
struct OvHeader { long long overflow, reserved; };          // of the table; the slots follow it
static_assert(sizeof(OvSlot) == 16 && sizeof(OvHeader) == 16, "16-byte header, 16-byte slots");
static_assert(sizeof(InsarOverlap) == 16, "InsarOverlap is one 16-byte store");

// 1 where the pixel is dropped; pixels past the end are dropped too
__device__ __forceinline__ void ov_void4(const uint8_t* p, int void_value, int64_t i, int64_t n, bool vec, bool* drop) {
  if (vec) {
    const uint32_t u = p ? *reinterpret_cast<const uint32_t*>(p + i) : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) drop[j] = p && (int)((u >> (8 * j)) & 0xffu) == void_value;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) drop[j] = i + j >= n || (p && (int)p[i + j] == void_value);
  }
}

// add n under `key` (!= 0): at most `mask + 1` probe steps, every access to the table an agent-scope atomic. Slots are never
// freed, so the overflow word is only ever raised on a table with no empty slot left: a probe that sees it raised gives up (every
// 64th step looks), which keeps the calls that are going to be refused anyway short.
__device__ __forceinline__ void ov_insert(OvHeader* hdr, OvSlot* slots, unsigned int mask, unsigned long long key, int n) {
  unsigned int s = (unsigned int)insar_mix64(key) & mask;
  for (unsigned int step = 0; step <= mask; ++step) {
    unsigned long long cur = __hip_atomic_load(&slots[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull)           // on failure `cur` receives the key that another thread has put there since
      __hip_atomic_compare_exchange_strong(&slots[s].key, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull || cur == key) {
      __hip_atomic_fetch_add(&slots[s].count, (long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    s = (s + 1u) & mask;
    if ((step & 63u) == 63u && __hip_atomic_load(&hdr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
  __hip_atomic_fetch_or(&hdr->overflow, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(OV_THREADS)
overlap_clear_kernel(int4* __restrict__ table, int64_t table_chunks, int4* __restrict__ out) {
  const int4 z = make_int4(0, 0, 0, 0);
  for (int64_t i = blockIdx.x * (int64_t)OV_THREADS + threadIdx.x; i < table_chunks; i += (int64_t)gridDim.x * OV_THREADS) table[i] = z;
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = z;
}

__global__ void __launch_bounds__(OV_THREADS)
overlap_count_kernel(const int* __restrict__ pred, const int* __restrict__ gt, const uint8_t* __restrict__ voidmap, int void_value,
                     int64_t npix, int vec, OvHeader* hdr, OvSlot* slots, unsigned int mask) {
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q0 = blockIdx.x * (int64_t)OV_THREADS; q0 < nquads; q0 += (int64_t)gridDim.x * OV_THREADS) {
    const int64_t q = q0 + threadIdx.x;                          // the loop bound is uniform over the block: shuffles below
    unsigned long long k[4] = {0ull, 0ull, 0ull, 0ull};
    int cnt[4];
    if (q < nquads) {
      int p[4], g[4];
      bool drop[4];
      quad_load(pred, q << 2, npix, vec, 0, p);
      quad_load(gt, q << 2, npix, vec, 0, g);
      ov_void4(voidmap, void_value, q << 2, npix, vec, drop);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!drop[j]) k[j] = ((unsigned long long)(uint32_t)p[j] << 32) | (unsigned long long)(uint32_t)g[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[j] = k[j] != 0ull;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (k[j] != 0ull && k[j] == k[j - 1]) { cnt[j] += cnt[j - 1]; cnt[j - 1] = 0; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long key = cnt[j] > 0 ? k[j] : 0ull;
      if (__ballot(key != 0ull) == 0) continue;
      const WaveRuns runs = wave_runs(key);
      const int total = wave_run_reduce(runs, cnt[j], WaveAdd());
      if (runs.head && key != 0ull) ov_insert(hdr, slots, mask, key, total);
    }
  }
}

// one slot per thread and pass; a work-group claims the output positions of its non-empty slots with ONE add on the cursor
__global__ void __launch_bounds__(OV_THREADS)
overlap_compact_kernel(const OvHeader* __restrict__ hdr, const OvSlot* __restrict__ slots, int64_t capacity, int64_t max_pairs,
                       unsigned long long* out_header, InsarOverlap* __restrict__ records) {
  __shared__ int wcount[OV_THREADS / INSAR_WAVE];
  __shared__ unsigned long long base_s;
  const int lane = (int)__lane_id(), wave = threadIdx.x / INSAR_WAVE;
  for (int64_t s0 = blockIdx.x * (int64_t)OV_THREADS; s0 < capacity; s0 += (int64_t)gridDim.x * OV_THREADS) {
    const int64_t s = s0 + threadIdx.x;
    int4 v = make_int4(0, 0, 0, 0);                              // {key lo = gt, key hi = pred, count lo, count hi}
    if (s < capacity) v = *reinterpret_cast<const int4*>(slots + s);
    const bool full = (v.x | v.y) != 0;
    const unsigned long long b = __ballot(full);
    if (lane == 0) wcount[wave] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = wcount[0] + wcount[1] + wcount[2] + wcount[3];
      base_s = n ? atomicAdd(out_header, (unsigned long long)n) : 0ull;
    }
    __syncthreads();
    int64_t pos = (int64_t)base_s + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wcount[w];
    if (full && pos < max_pairs) *reinterpret_cast<int4*>(records + pos) = make_int4(v.y, v.x, v.z, v.w);
    __syncthreads();                                             // wcount and base_s are rewritten by the next pass
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out_header[1] = (unsigned long long)hdr->overflow;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int overlap_capacity(const char* who, int64_t max_pairs, int64_t* capacity) {
  if (max_pairs < 1 || max_pairs > OV_MAX_PAIRS)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_pairs %lld outside 1..%lld", who, (long long)max_pairs, (long long)OV_MAX_PAIRS);
  int64_t c = 2;
  while (c < 2 * max_pairs) c <<= 1;
  *capacity = c;
  return INSAR_OK;
}

extern "C" int insar_overlap_scratch_bytes(int64_t max_pairs, int64_t* table_bytes, int64_t* out_bytes) {
  const char* who = "insar_overlap_scratch_bytes";
  if (!table_bytes || !out_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  int64_t cap;
  if (int rc = overlap_capacity(who, max_pairs, &cap)) return rc;
  *table_bytes = (int64_t)sizeof(OvHeader) + cap * (int64_t)sizeof(OvSlot);
  *out_bytes = 16 + max_pairs * (int64_t)sizeof(InsarOverlap);
  return INSAR_OK;
}

extern "C" int insar_overlap_clear(void* table, void* out, int64_t max_pairs, void* stream) {
  const char* who = "insar_overlap_clear";
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  if (int rc = scene_check_buffer(who, "out", out)) return rc;
  int64_t cap;
  if (int rc = overlap_capacity(who, max_pairs, &cap)) return rc;
  const int64_t chunks = 1 + cap;
  hipLaunchKernelGGL(overlap_clear_kernel, dim3(insar_grid_cap((chunks + OV_THREADS - 1) / OV_THREADS)), dim3(OV_THREADS), 0,
                     (hipStream_t)stream, (int4*)table, chunks, (int4*)out);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_overlap_count(const int32_t* pred, const int32_t* gt, const uint8_t* voidmap, int32_t void_value, int32_t H,
                                   int32_t W, void* table, int64_t max_pairs, void* stream) {
  const char* who = "insar_overlap_count";
  if (!pred || !gt) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  const int64_t npix = (int64_t)H * W;
  if (npix >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^31 pixels or more", who, H, W);
  if (voidmap && (void_value < 0 || void_value > 255)) INSAR_FAIL(INSAR_E_ARG, "%s: void_value %d outside 0..255", who, void_value);
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  int64_t cap;
  if (int rc = overlap_capacity(who, max_pairs, &cap)) return rc;
  if ((((uintptr_t)pred) | ((uintptr_t)gt)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: label map not 4-byte aligned", who);
  const int vec = (npix % 4 == 0) && insar_aligned16(pred) && insar_aligned16(gt) && ((((uintptr_t)voidmap) & 3u) == 0);
  OvHeader* hdr = (OvHeader*)table;
  hipLaunchKernelGGL(overlap_count_kernel, dim3(insar_grid_cap((npix / 4 + OV_THREADS) / OV_THREADS)), dim3(OV_THREADS), 0,
                     (hipStream_t)stream, (const int*)pred, (const int*)gt, voidmap, (int)void_value, npix, vec, hdr, (OvSlot*)(hdr + 1),
                     (unsigned int)(cap - 1));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_overlap_compact(const void* table, int64_t max_pairs, void* out, void* stream) {
  const char* who = "insar_overlap_compact";
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  if (int rc = scene_check_buffer(who, "out", out)) return rc;
  int64_t cap;
  if (int rc = overlap_capacity(who, max_pairs, &cap)) return rc;
  const OvHeader* hdr = (const OvHeader*)table;
  hipLaunchKernelGGL(overlap_compact_kernel, dim3(insar_grid_cap((cap + OV_THREADS - 1) / OV_THREADS)), dim3(OV_THREADS), 0,
                     (hipStream_t)stream, hdr, (const OvSlot*)(hdr + 1), cap, max_pairs, (unsigned long long*)out,
                     (InsarOverlap*)((char*)out + 16));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
