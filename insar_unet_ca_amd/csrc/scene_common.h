// What the scene tools (scene.hip, scene_valid.hip, regions.hip, augment.hip, overlap.hip, distance.hip, crops.hip, outline.hip,
// skeleton.hip, raster.hip, zonal.hip, simplify.hip, contour_simplify.hip, split.hip, warp.hip, stack.hip, sieve.hip,
// hysteresis.hip, contour.hip, reconstruct.hip), the focal loss of focal.hip and the dropout kernel of deeplab.hip share: the counter hash, the guarded four-element access,
// the wave primitives (runs of equal keys, scan, max), the relaxed agent-scope word accessors and the one-add-per-wave counters,
// the image / label quads of the two gather kernels and the host side's small change (scratch layout, grids, pointer checks).
// Each file's kernels, launch geometry and argument checks are its own. pair_table.h builds the pair table of overlap.hip,
// sieve.hip and split.hip on top of this header.
#pragma once
#include "common.h"

// ---- hash ---------------------------------------------------------------------------------------------------------------
// insar_hash64(key, i) is aug_hash64 of include/insar_hip.h: splitmix64's finaliser over key + golden * (i + 1), uint64 with
// wrap-around. Everything random in the library (dropout masks, augmentation tables and noise, crop draws) is this function
// of a key and a counter; insar_unet_ca_amd/augment.py and the tests' references restate it in Python.
__host__ __device__ __forceinline__ uint64_t insar_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t insar_hash64(uint64_t key, uint64_t i) {
  return insar_mix64(key + 0x9E3779B97F4A7C15ull * (i + 1ull));
}

// ---- four consecutive elements per thread: one 16-byte (4-byte for uint8) access where `vec`, guarded scalars otherwise ----
// `vec` promises i + 4 <= n and an aligned p + i; without it, elements at or past n read as `fill` and are not written.
__device__ __forceinline__ void quad_load(const int* p, int64_t i, int64_t n, bool vec, int fill, int* v) {
  if (vec) {
    const int4 q = *reinterpret_cast<const int4*>(p + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (i + j < n) ? p[i + j] : fill;
  }
}
__device__ __forceinline__ void quad_load(const float* p, int64_t i, int64_t n, bool vec, float fill, float* v) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (i + j < n) ? p[i + j] : fill;
  }
}
__device__ __forceinline__ void quad_load_u8(const uint8_t* p, int64_t i, int64_t n, bool vec, int fill, int* v) {
  if (vec) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (int)((u >> (8 * j)) & 0xffu);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (i + j < n) ? (int)p[i + j] : fill;
  }
}
__device__ __forceinline__ void quad_store(int* p, int64_t i, int64_t n, bool vec, const int* v) {
  if (vec) {
    *reinterpret_cast<int4*>(p + i) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = v[j];
  }
}

__device__ __forceinline__ void quad_store(float* p, int64_t i, int64_t n, bool vec, const float* v) {
  if (vec) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = v[j];
  }
}
__device__ __forceinline__ void quad_store_u8(uint8_t* p, int64_t i, int64_t n, bool vec, const int* v) {
  if (vec) {
    *reinterpret_cast<uint32_t*>(p + i) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = (uint8_t)v[j];
  }
}

// ---- wave primitives, all over the INSAR_WAVE lanes of a full wave -----------------------------------------------------------
// runs of equal keys over the lanes; wave_run_reduce collects op over a run at its first lane (`head`)
struct WaveRuns { int lane, id; bool head; };
template <typename K>
__device__ __forceinline__ WaveRuns wave_runs(K key) {
  WaveRuns r;
  r.lane = (int)__lane_id();
  const K prev = __shfl_up(key, 1, INSAR_WAVE);
  r.head = r.lane == 0 || prev != key;
  const unsigned long long heads = __ballot(r.head);
  r.id = __popcll(heads & ((2ull << r.lane) - 1ull));          // lane 63: 2 << 63 wraps to 0, the mask is all ones
  return r;
}
template <typename T, typename Op>
__device__ __forceinline__ T wave_run_reduce(const WaveRuns& r, T v, Op op) {
#pragma unroll
  for (int d = 1; d < INSAR_WAVE; d <<= 1) {
    const T o = __shfl_down(v, d, INSAR_WAVE);
    const int oid = __shfl_down(r.id, d, INSAR_WAVE);
    if (r.lane + d < INSAR_WAVE && oid == r.id) v = op(v, o);
  }
  return v;
}
struct WaveAdd { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct WaveMin { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; } };
struct WaveMax { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; } };

// lane: a caller that already keeps threadIdx.x & 63 passes it; taking __lane_id() again costs crops_scan_rows_kernel 0.4 %
__device__ __forceinline__ int wave_incl_scan(int v, int lane = (int)__lane_id()) {
#pragma unroll
  for (int d = 1; d < INSAR_WAVE; d <<= 1) {
    const int o = __shfl_up(v, d, INSAR_WAVE);
    if (lane >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int o = INSAR_WAVE / 2; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, INSAR_WAVE);
    v = u > v ? u : v;
  }
  return v;
}

// a word that work-groups of one launch share (they may sit on different XCDs): relaxed, agent scope
__device__ __forceinline__ int agent_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void agent_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// one add per wave on such a word: of the lanes that raise `flag`, or of the lanes' counts `c`
__device__ __forceinline__ void wave_count(int* word, bool flag) {
  const unsigned long long b = __ballot(flag);
  if (b && (int)__lane_id() == __ffsll((long long)b) - 1)
    __hip_atomic_fetch_add(word, __popcll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wave_tally(int* word, int c) {
  if (__ballot(c != 0) == 0) return;
#pragma unroll
  for (int o = INSAR_WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, INSAR_WAVE);
  if ((int)__lane_id() == 0) __hip_atomic_fetch_add(word, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- image and label quads of the gather kernels (insar_scene_gather, insar_crops_gather) ---------------------------------------
// four uint8 at any address as one dword, element 0 in the low byte
__device__ __forceinline__ uint32_t load4_u8_any(const uint8_t* p) {
  if ((((uintptr_t)p) & 3u) == 0) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// four adjacent scene pixels as network input: uint8 gets the reference's ToTensor + Normalize (x = v / 255; (x - 0.5) / 0.5,
// data.reference_transforms), float32 is copied. The gathers' contract is bitwise: contraction is off whatever the includer set.
template <typename S>
__device__ __forceinline__ void image_quad(const S* p, float* f);
template <>
__device__ __forceinline__ void image_quad<uint8_t>(const uint8_t* p, float* f) {
#pragma clang fp contract(off)
  const uint32_t u = load4_u8_any(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x = (float)((u >> (8 * j)) & 0xffu) / 255.0f;
    f[j] = (x - 0.5f) / 0.5f;
  }
}
template <>
__device__ __forceinline__ void image_quad<float>(const float* p, float* f) {
  if ((((uintptr_t)p) & 15u) == 0) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
    f[0] = p[0]; f[1] = p[1]; f[2] = p[2]; f[3] = p[3];
  }
}

// int64 masks move as 16-byte pairs; four labels packed in a dword (element 0 in the low byte) widen into two of them
struct __attribute__((aligned(16))) insar_i64x2 { int64_t a, b; };
__device__ __forceinline__ void quad_store_i64(int64_t* p, const int64_t* v) {          // p 16-byte aligned
  insar_i64x2* o = reinterpret_cast<insar_i64x2*>(p);
  insar_i64x2 lo, hi;
  lo.a = v[0]; lo.b = v[1]; hi.a = v[2]; hi.b = v[3];
  o[0] = lo;
  o[1] = hi;
}
__device__ __forceinline__ void labels4_store_i64(int64_t* p, uint32_t u) {
  const int64_t v[4] = {(int64_t)(u & 0xffu), (int64_t)((u >> 8) & 0xffu), (int64_t)((u >> 16) & 0xffu), (int64_t)(u >> 24)};
  quad_store_i64(p, v);
}

// ---- host side: scratch layout, grids, pointer checks --------------------------------------------------------------------------
static inline int64_t insar_align16(int64_t b) { return (b + 15) & ~(int64_t)15; }
// bump allocator of a scratch layout: take(bytes) is the offset of the next 16-byte aligned piece, `at` the bytes taken so far
struct ScratchTake {
  int64_t at = 0;
  int64_t operator()(int64_t bytes) { const int64_t o = at; at += insar_align16(bytes); return o; }
};
template <typename T>
static inline T* scratch_at(void* scratch, int64_t off) { return reinterpret_cast<T*>((char*)scratch + off); }
// work-groups of `per` items: all of them (n < 2^31), or capped for a grid-stride loop
static inline unsigned scene_blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }
static inline dim3 scene_grid(int64_t items, int threads) { return dim3(insar_grid_cap((items + threads - 1) / threads)); }
// a buffer of the library's own layout (16-byte aligned), a map at its element's alignment
static inline int scene_check_buffer(const char* who, const char* what, const void* p) {
  if (!p) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, what);
  if (!insar_aligned16(p)) INSAR_FAIL(INSAR_E_ALIGN, "%s: %s not 16-byte aligned", who, what);
  return INSAR_OK;
}
static inline int scene_check_map(const char* who, const char* what, const void* p, unsigned align) {
  if (!p) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, what);
  if (((uintptr_t)p) & (align - 1u)) INSAR_FAIL(INSAR_E_ALIGN, "%s: %s not %u-byte aligned", who, what, align);
  return INSAR_OK;
}
