// What outline.hip (elements = boundary edges, records = rings) and contour.hip (elements = lattice crossings, records = lines)
// share: the tracing of a compact array of n elements, each with one successor, into numbered records of ordered positions.
// Each file keeps what is its own: how the elements are found and linked (mark / offsets / link, contour's quantise), where a
// list is cut, what goes to an element's position (scatter, outline's compact), its scratch layout and its entry points.
//
//   edges   scan     trace_scan_kernel, one work-group: the exclusive prefix sum of the tool's block counts; n goes to the table
//                    header, and the tool's first_header writes the rest of it (the first scan of a call)
//   lead    trace_lead: list_rounds(n) rounds of list_rank.h's pointer doubling on pairs (jump, min)
//   rank    trace_cut_and_rank: the tool's cut launch, then list_rounds(n) rounds of Wyllie list ranking on pairs (next, d)
//   records trace_number: count   leaders (the tool's is_leader) and their record lengths per block of 1024 elements
//                         scan    one work-group: both prefix sums; the number of records goes to the header
//                         number  per leader: record number and first position; the tool's init_record writes the record
//   write   reduce   trace_reduce at the end of the tool's reduce kernel, over the ordered array, where a record is one contiguous
//                    run: area2 and box, combined over the runs of a wave before the atomics
//
// One launch per step and no work-group ever waits on another: every round reads one pair buffer and writes the other, ordered
// by kernel boundaries on the caller's stream. The atomics add int64 / take int32 minima and maxima at agent scope, so their
// arrival order changes nothing. The kernels are templates on the tool: the header is included by two files of a library linked
// without relocatable device code. A Tool is passed to the kernels by value and supplies
//   bool is_leader(int k) const                             element k leads a record
//   void init_record(int r, int k, int start, int len) const   record r, led by k: its three 16-byte stores
//   static void first_header(int* hdr, int t, int slot, int carry, const int* a, int nblk, int first)
//                                                           thread t's share of the header behind the first scan of a call
#pragma once
#include "scene_common.h"
#include "block_scan.h"
#include "list_rank.h"
#include <limits.h>
#include <stddef.h>

#define TR_THREADS 256
#define TR_NB 1024                        // pixels / elements per numbering block (256 threads x 4)
#define TR_SCAN_THREADS 1024
#define TR_MAX_ELEMENTS (1 << 30)         // element slots, and records

// InsarRing and InsarContourLine are one 48-byte layout, written as three 16-byte stores; only slots 2 (label / level) and
// 6 (edges / closed) mean different things. trace_reduce works on either through this view of it.
struct TraceRecord {
  int64_t area2;
  int32_t own2, leader, start, count, own6, y0, x0, y1, x1, _pad;
};
#define TR_SAME_FIELD(f)                                                                                                          \
  static_assert(offsetof(InsarRing, f) == offsetof(InsarContourLine, f) && offsetof(InsarRing, f) == offsetof(TraceRecord, f), \
                "InsarRing and InsarContourLine keep " #f " at one offset")
static_assert(sizeof(InsarRing) == 48 && sizeof(InsarContourLine) == 48 && sizeof(TraceRecord) == 48, "a record is three 16-byte stores");
TR_SAME_FIELD(area2); TR_SAME_FIELD(leader); TR_SAME_FIELD(start); TR_SAME_FIELD(count);
TR_SAME_FIELD(y0); TR_SAME_FIELD(x0); TR_SAME_FIELD(y1); TR_SAME_FIELD(x1);
#undef TR_SAME_FIELD

// ---------------------------------------------------------------------------------------------
// the header scan
// ---------------------------------------------------------------------------------------------
// One work-group: a[] (and b[], nullable) become their exclusive prefix sums; the total of a[] goes to the header's int32 slot
// `slot`. `first` != 0 (the first scan of a call): the tool writes the other slots of the header too.
template <class Tool>
__global__ void __launch_bounds__(TR_SCAN_THREADS)
trace_scan_kernel(int* __restrict__ a, int* __restrict__ b, int nblk, int* __restrict__ hdr, int slot, int first) {
  __shared__ int w[TR_SCAN_THREADS / INSAR_WAVE];
  const int carry = block_scan_array<TR_SCAN_THREADS>(a, nblk, w);                   // the new a[] is visible to every thread
  if (b) block_scan_array<TR_SCAN_THREADS>(b, nblk, w);
  const int t = threadIdx.x;
  if (first) Tool::first_header(hdr, t, slot, carry, a, nblk, first);
  else if (t == slot) hdr[t] = carry;
}

// ---------------------------------------------------------------------------------------------
// records: count / scan / number
// ---------------------------------------------------------------------------------------------
template <class Tool>
__global__ void __launch_bounds__(TR_THREADS)
trace_count_kernel(Tool tool, const int2* __restrict__ dist, int n, int* __restrict__ rcnt, int* __restrict__ rlen) {
  __shared__ int wsum[TR_THREADS / INSAR_WAVE];
  const int k0 = blockIdx.x * TR_NB + threadIdx.x * 4;
  int c = 0, l = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + j;
    if (k < n && tool.is_leader(k)) { ++c; l += dist[k].y + 1; }
  }
  int tc, tl;
  block_prefix_sum<TR_THREADS>(c, wsum, &tc);
  block_prefix_sum<TR_THREADS>(l, wsum, &tl);
  if (threadIdx.x == 0) { rcnt[blockIdx.x] = tc; rlen[blockIdx.x] = tl; }
}

template <class Tool>
__global__ void __launch_bounds__(TR_THREADS)
trace_number_kernel(Tool tool, const int2* __restrict__ dist, int n, const int* __restrict__ rcnt, const int* __restrict__ rlen,
                    int2* __restrict__ info, int max_records) {
  __shared__ int wsum[TR_THREADS / INSAR_WAVE];
  const int k0 = blockIdx.x * TR_NB + threadIdx.x * 4;
  bool is[4];
  int len[4], c = 0, l = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + j;
    is[j] = k < n && tool.is_leader(k);
    len[j] = is[j] ? dist[k].y + 1 : 0;
    c += is[j]; l += len[j];
  }
  int tc, tl;
  int r = rcnt[blockIdx.x] + block_prefix_sum<TR_THREADS>(c, wsum, &tc);
  int st = rlen[blockIdx.x] + block_prefix_sum<TR_THREADS>(l, wsum, &tl);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!is[j]) continue;
    const int k = k0 + j;
    info[k] = make_int2(r, st);
    if (r < max_records) tool.init_record(r, k, st, len[j]);
    ++r; st += len[j];
  }
}

// ---------------------------------------------------------------------------------------------
// write: the end of a reduce kernel
// ---------------------------------------------------------------------------------------------
// Every lane of the wave calls it with the record of its position (key < 0: none), its shoelace term and its vertex. The runs
// of a record are combined over the wave, and the first lane of a run adds area2 and tightens the box of recs[key]; true on that
// lane, for what else the tool keeps per record.
__device__ __forceinline__ bool trace_reduce(const WaveRuns& runs, TraceRecord* recs, int key, int max_records, long long a2, int vy,
                                             int vx) {
  const long long ta = wave_run_reduce(runs, a2, WaveAdd());
  const int y0 = wave_run_reduce(runs, vy, WaveMin()), y1 = wave_run_reduce(runs, vy + 1, WaveMax());
  const int x0 = wave_run_reduce(runs, vx, WaveMin()), x1 = wave_run_reduce(runs, vx + 1, WaveMax());
  if (!(runs.head && key >= 0 && key < max_records)) return false;
  TraceRecord* r = recs + key;
  if (ta) atomicAdd(reinterpret_cast<unsigned long long*>(&r->area2), (unsigned long long)ta);
  // the box only tightens: a stale read can cost a redundant atomic, never lose an update
  if (y0 < __hip_atomic_load(&r->y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&r->y0, y0);
  if (x0 < __hip_atomic_load(&r->x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&r->x0, x0);
  if (y1 > __hip_atomic_load(&r->y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&r->y1, y1);
  if (x1 > __hip_atomic_load(&r->x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&r->x1, x1);
  return true;
}

// ---------------------------------------------------------------------------------------------
// host side: the checks and the drivers of lead, rank and the numbering of records
// ---------------------------------------------------------------------------------------------
// a capacity (`what`: "max_edges", "max_rings", ...) against its range
static inline int trace_check_capacity(const char* who, const char* what, int32_t cap) {
  if (cap < 1 || cap > TR_MAX_ELEMENTS) INSAR_FAIL(INSAR_E_SHAPE, "%s: %s %d outside 1 .. 2^30", who, what, cap);
  return INSAR_OK;
}
// the element count read back from the header (`what`) against the element slots (`cap_name`)
static inline int trace_check_count(const char* who, const char* what, int32_t n, const char* cap_name, int32_t cap) {
  if (n < 0 || n > cap) INSAR_FAIL(INSAR_E_SHAPE, "%s: %s %d outside 0 .. %s=%d", who, what, n, cap_name, cap);
  return INSAR_OK;
}
static inline int trace_check_table(const char* who, const char* what, int32_t max_records, const void* table) {
  if (int rc = trace_check_capacity(who, what, max_records)) return rc;
  return scene_check_buffer(who, "table", table);
}

// The pair buffers: `link` fills p0, `lead` runs from there, `cut` reads its result and writes the other buffer, `rank` goes on
// from there: the final distances are in p1 whatever n is, and p0 is free for the numbering (list_rank.h).
static inline int trace_lead(int2* p0, int2* p1, int n, hipStream_t s, const char* who) {
  int2* const p[2] = {p0, p1};
  return list_lead<TR_THREADS>(p, 0, n, s, who);
}
// launch_cut(in, out) launches the tool's cut kernel over n elements: `in` is where `lead` ended
template <class LaunchCut>
static inline int trace_cut_and_rank(LaunchCut launch_cut, int2* p0, int2* p1, int n, hipStream_t s, const char* who) {
  int2* const p[2] = {p0, p1};
  const int led = list_rounds(n) & 1;                            // where `lead` ended
  launch_cut((const int2*)p[led], p[led ^ 1]);
  INSAR_CHECK_LAUNCH(who);
  return list_rank<TR_THREADS>(p, led ^ 1, n, s, who);
}

// count / scan / number: 3 launches (1 for n = 0: the header's record count is written all the same)
template <class Tool>
static inline int trace_number(const Tool& tool, const int2* dist, int n, int* rcnt, int* rlen, int2* info, void* table, int slot,
                               int max_records, hipStream_t s, const char* who) {
  const int nblk = (int)scene_blocks(n, TR_NB);
  if (nblk > 0) {
    hipLaunchKernelGGL(trace_count_kernel<Tool>, dim3((unsigned)nblk), dim3(TR_THREADS), 0, s, tool, dist, n, rcnt, rlen);
    INSAR_CHECK_LAUNCH(who);
  }
  hipLaunchKernelGGL(trace_scan_kernel<Tool>, dim3(1), dim3(TR_SCAN_THREADS), 0, s, rcnt, rlen, nblk, (int*)table, slot, 0);
  INSAR_CHECK_LAUNCH(who);
  if (nblk > 0) {
    hipLaunchKernelGGL(trace_number_kernel<Tool>, dim3((unsigned)nblk), dim3(TR_THREADS), 0, s, tool, dist, n, (const int*)rcnt,
                       (const int*)rlen, info, max_records);
    INSAR_CHECK_LAUNCH(who);
  }
  return INSAR_OK;
}
