// The pair table of overlap.hip (pairs (pred, gt), value = pixels), sieve.hip (pairs of adjacent regions, value = shared pixel
// edges) and split.hip (pairs of adjacent basins, value = the highest saddle): open addressing in global memory over 64-bit keys,
// filled in one launch, read in the next. Each file keeps what is its own: how a key is formed, the pixel pass that forms it,
// the record type that Python sees, its scratch layout and its entry points.
//
//   clear    pair_table_clear_kernel: zeroes the slots and a second range of 16-byte chunks, the words that hold the overflow
//            flag and the cursor
//   fill     the tool's pixel kernel ends in pair_fold_insert: a thread folds those of its keys that are equal, the lanes of a
//            wave fold over runs of equal keys, and the first lane of a run calls pair_insert. slot = {uint64 key, int64 value},
//            key 0 = empty: no tool ever forms the key 0
//   compact  pair_table_compact_kernel: the non-empty slots as 16-byte records {key hi, key lo, value} behind a cursor; never
//            more than max_pairs records, but the cursor ends at the true number of keys
//
// Visibility (the rule of regions_merge_kernel): in `fill`, work-groups on different XCDs claim and update the same slots, so
// EVERY access to the table and to the overflow word there is an agent-scope atomic (relaxed load / compare-exchange /
// fetch_add or fetch_max / fetch_or); there is no plain load of either in that launch. `clear` and `compact` lie behind kernel
// boundaries and use plain accesses; compact's cursor is an atomic of its own launch.
// No thread waits for another: a slot is claimed with ONE 64-bit compare-and-swap on its key (yours if it held 0 or your key,
// else the next slot) and the probe is bounded by the capacity. A probe that runs out raises the overflow word and drops its
// contribution; the host then refuses the whole table. Slots are never freed, so the word is only ever raised on a table with
// no empty slot left, and every later probe is going to be refused too: a probe looks at the word every 64th step and gives up
// where it is raised, which keeps those calls short.
// Reproducibility: which slot a key lands in, and so the order of the records, depends on arrival order; the values (integer
// sums, maxima) do not. The host sorts the records.
// The kernels are templates or static: the header is included by three files of a library linked without relocatable device code.
#pragma once
#include "scene_common.h"

#define PAIR_TABLE_THREADS 256
#define PAIR_TABLE_MAX_PAIRS ((int64_t)1 << 24)

struct PairSlot { unsigned long long key; long long val; };
static_assert(sizeof(PairSlot) == 16, "a slot is one 16-byte load");

// slots of a table that takes max_pairs keys: a power of two, at least twice as many
static inline int pair_table_capacity(const char* who, int64_t max_pairs, int64_t* capacity) {
  if (max_pairs < 1 || max_pairs > PAIR_TABLE_MAX_PAIRS)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_pairs %lld outside 1..%lld", who, (long long)max_pairs, (long long)PAIR_TABLE_MAX_PAIRS);
  int64_t c = 2;
  while (c < 2 * max_pairs) c <<= 1;
  *capacity = c;
  return INSAR_OK;
}

__device__ __forceinline__ void pair_combine(long long* val, long long v, WaveAdd) {
  __hip_atomic_fetch_add(val, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void pair_combine(long long* val, long long v, WaveMax) {
  __hip_atomic_fetch_max(val, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// table[key] = op(table[key], v) for key != 0: at most `mask + 1` probe steps (see the head of the file).
// The overflow word is an int32 that only ever holds 0 or 1. overlap.hip keeps an int64 in its table header and passes the
// address of its low dword (little-endian): or-ing 1 into that dword and testing it for non-zero is the same as on the whole
// word, and compact reads the word only after the kernel boundary.
template <typename Op>
__device__ __forceinline__ void pair_insert(int* overflow, PairSlot* slots, unsigned int mask, unsigned long long key, int v) {
  unsigned int s = (unsigned int)insar_mix64(key) & mask;
  for (unsigned int step = 0; step <= mask; ++step) {
    unsigned long long cur = __hip_atomic_load(&slots[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull)           // on failure `cur` receives the key that another thread has put there since
      __hip_atomic_compare_exchange_strong(&slots[s].key, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull || cur == key) {
      pair_combine(&slots[s].val, (long long)v, Op());
      return;
    }
    s = (s + 1u) & mask;
    if ((step & 63u) == 63u && agent_load(overflow)) return;
  }
  __hip_atomic_fetch_or(overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The end of a fill kernel, called by every lane of the wave with the thread's N keys (0: none) and their values. Equal keys
// of the thread fold into the first of them, then key by key the lanes fold over runs of equal keys and the first lane of a
// run inserts. A wave without any key leaves after one ballot: in a map of large regions most waves do.
// The fold works on copies: folding the caller's arrays in place costs sieve_pairs_kernel 18 VGPRs, 57 instead of 39
// (profiles/pair_table_refactor_ab.txt, part 1).
template <int N, typename Op>
__device__ __forceinline__ void pair_fold_insert(int* overflow, PairSlot* slots, unsigned int mask, const unsigned long long* keys,
                                                 const int* values) {
  unsigned long long k[N], any = 0ull;
  int v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { k[j] = keys[j]; v[j] = values[j]; any |= k[j]; }
  if (__ballot(any != 0ull) == 0) return;
  if (any != 0ull) {
#pragma unroll
    for (int j = 1; j < N; ++j)
#pragma unroll
      for (int m = 0; m < j; ++m)
        if (k[j] != 0ull && k[j] == k[m]) { v[m] = Op()(v[m], v[j]); k[j] = 0ull; }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (__ballot(k[j] != 0ull) == 0) continue;
    const WaveRuns runs = wave_runs(k[j]);
    const int t = wave_run_reduce(runs, v[j], Op());
    if (runs.head && k[j] != 0ull) pair_insert<Op>(overflow, slots, mask, k[j], t);
  }
}

// `slots`: slot_chunks 16-byte chunks (overlap.hip's table header lies in front of its slots and goes with them); `words`: the
// word_chunks chunks that hold the tool's overflow word and cursor
static __global__ void __launch_bounds__(PAIR_TABLE_THREADS)
pair_table_clear_kernel(int4* __restrict__ slots, int64_t slot_chunks, int4* __restrict__ words, int word_chunks) {
  const int4 z = make_int4(0, 0, 0, 0);
  for (int64_t i = blockIdx.x * (int64_t)PAIR_TABLE_THREADS + threadIdx.x; i < slot_chunks; i += (int64_t)gridDim.x * PAIR_TABLE_THREADS)
    slots[i] = z;
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < word_chunks; i += PAIR_TABLE_THREADS) words[i] = z;
}

// One slot per thread and pass; a work-group claims the positions of its non-empty slots with ONE add on the cursor (int32 or
// uint64 as the tool's layout has it; <= capacity <= 2^25). A record is {key hi, key lo, value lo, value hi}. `overflow_out`
// (nullable): where the overflow word is copied to, in the cursor's type.
template <typename Cursor>
__global__ void __launch_bounds__(PAIR_TABLE_THREADS)
pair_table_compact_kernel(const PairSlot* __restrict__ slots, int64_t capacity, int64_t max_pairs, Cursor* cursor,
                          int4* __restrict__ records, const int* __restrict__ overflow, Cursor* overflow_out) {
  constexpr int WAVES = PAIR_TABLE_THREADS / INSAR_WAVE;
  __shared__ int wcount[WAVES];
  __shared__ Cursor base_s;
  const int lane = (int)__lane_id(), wave = threadIdx.x / INSAR_WAVE;
  for (int64_t s0 = blockIdx.x * (int64_t)PAIR_TABLE_THREADS; s0 < capacity; s0 += (int64_t)gridDim.x * PAIR_TABLE_THREADS) {
    const int64_t s = s0 + threadIdx.x;
    int4 v = make_int4(0, 0, 0, 0);                              // {key lo, key hi, value lo, value hi}
    if (s < capacity) v = *reinterpret_cast<const int4*>(slots + s);
    const bool full = (v.x | v.y) != 0;
    const unsigned long long b = __ballot(full);
    if (lane == 0) wcount[wave] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
      int n = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) n += wcount[w];
      base_s = n ? atomicAdd(cursor, (Cursor)n) : (Cursor)0;
    }
    __syncthreads();
    int64_t pos = (int64_t)base_s + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wcount[w];
    if (full && pos < max_pairs) records[pos] = make_int4(v.y, v.x, v.z, v.w);
    __syncthreads();                                             // wcount and base_s are rewritten by the next pass
  }
  if (overflow_out && blockIdx.x == 0 && threadIdx.x == 0) *overflow_out = (Cursor)*overflow;
}

// ---- host side: the two launches; the caller checks them (INSAR_CHECK_LAUNCH) -----------------------------------------------------
static inline void pair_table_clear(hipStream_t s, void* slots, int64_t slot_chunks, void* words, int word_chunks) {
  hipLaunchKernelGGL(pair_table_clear_kernel, scene_grid(slot_chunks, PAIR_TABLE_THREADS), dim3(PAIR_TABLE_THREADS), 0, s, (int4*)slots,
                     slot_chunks, (int4*)words, word_chunks);
}
template <typename Cursor>
static inline void pair_table_compact(hipStream_t s, const PairSlot* slots, int64_t capacity, int64_t max_pairs, Cursor* cursor,
                                      void* records, const int* overflow = nullptr, Cursor* overflow_out = nullptr) {
  hipLaunchKernelGGL(pair_table_compact_kernel<Cursor>, scene_grid(capacity, PAIR_TABLE_THREADS), dim3(PAIR_TABLE_THREADS), 0, s, slots,
                     capacity, max_pairs, cursor, (int4*)records, overflow, overflow_out);
}
