// Overlaps of two label maps: for every pair (p, g) = (pred[i], gt[i]) != (0, 0) over the pixels of a scene that a void map
// does not drop, the number of pixels that carry it. The rows (p, 0) and columns (0, g) are part of the table, so every area
// after voiding follows from it. Three launches per call, on the pair table of pair_table.h (the slot scheme, the visibility
// rule and the aggregation before the atomics are written there):
//
//   clear    zeroes the table (its header and slots) and the header of the output
//   count    table[key = p << 32 | g] += 1 per pixel; (0, 0) is never inserted, so no key is 0
//   compact  the non-empty slots as 16-byte records {int32 pred, int32 gt, int64 count} behind the header {int64 n_keys,
//            int64 overflow}; never more than max_pairs records, but n_keys is the true number of keys.
//
// Reproducibility: the counts are integer sums; the host sorts the records by (gt, pred).
#include "pair_table.h"

#define OV_THREADS 256

struct OvHeader { long long overflow, reserved; };          // of the table; the slots follow it
static_assert(sizeof(OvHeader) == sizeof(PairSlot), "the header is cleared as one more slot");
static_assert(sizeof(InsarOverlap) == 16, "InsarOverlap is one 16-byte store");
// pair_insert takes the low dword of the little-endian overflow word (see there)
static inline int* ov_overflow(const void* table) { return reinterpret_cast<int*>(&((OvHeader*)table)->overflow); }
static inline PairSlot* ov_slots(const void* table) { return reinterpret_cast<PairSlot*>((OvHeader*)table + 1); }

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

__global__ void __launch_bounds__(OV_THREADS)
overlap_count_kernel(const int* __restrict__ pred, const int* __restrict__ gt, const uint8_t* __restrict__ voidmap, int void_value,
                     int64_t npix, int vec, int* overflow, PairSlot* slots, unsigned int mask) {
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
    pair_fold_insert<4, WaveAdd>(overflow, slots, mask, k, cnt);
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" int insar_overlap_scratch_bytes(int64_t max_pairs, int64_t* table_bytes, int64_t* out_bytes) {
  const char* who = "insar_overlap_scratch_bytes";
  if (!table_bytes || !out_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  int64_t cap;
  if (int rc = pair_table_capacity(who, max_pairs, &cap)) return rc;
  *table_bytes = (int64_t)sizeof(OvHeader) + cap * (int64_t)sizeof(PairSlot);
  *out_bytes = 16 + max_pairs * (int64_t)sizeof(InsarOverlap);
  return INSAR_OK;
}

extern "C" int insar_overlap_clear(void* table, void* out, int64_t max_pairs, void* stream) {
  const char* who = "insar_overlap_clear";
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  if (int rc = scene_check_buffer(who, "out", out)) return rc;
  int64_t cap;
  if (int rc = pair_table_capacity(who, max_pairs, &cap)) return rc;
  pair_table_clear((hipStream_t)stream, table, 1 + cap, out, 1);
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
  if (int rc = pair_table_capacity(who, max_pairs, &cap)) return rc;
  if ((((uintptr_t)pred) | ((uintptr_t)gt)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: label map not 4-byte aligned", who);
  const int vec = (npix % 4 == 0) && insar_aligned16(pred) && insar_aligned16(gt) && ((((uintptr_t)voidmap) & 3u) == 0);
  hipLaunchKernelGGL(overlap_count_kernel, dim3(insar_grid_cap((npix / 4 + OV_THREADS) / OV_THREADS)), dim3(OV_THREADS), 0,
                     (hipStream_t)stream, (const int*)pred, (const int*)gt, voidmap, (int)void_value, npix, vec, ov_overflow(table),
                     ov_slots(table), (unsigned int)(cap - 1));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_overlap_compact(const void* table, int64_t max_pairs, void* out, void* stream) {
  const char* who = "insar_overlap_compact";
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  if (int rc = scene_check_buffer(who, "out", out)) return rc;
  int64_t cap;
  if (int rc = pair_table_capacity(who, max_pairs, &cap)) return rc;
  unsigned long long* out_header = (unsigned long long*)out;      // {n_keys, overflow}; the records follow
  pair_table_compact((hipStream_t)stream, ov_slots(table), cap, max_pairs, out_header, out_header + 2, ov_overflow(table), out_header + 1);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
