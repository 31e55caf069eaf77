// What simplify.hip (region outlines, records = rings) and contour_simplify.hip (contour lines, records = lines) share: the round
// and finish stages of Douglas-Peucker over the records of a vertex array. Every array is indexed by the POSITION of a vertex in
// the input vertex array (record after record); rings are not rotated: a segment that wraps over the end of its ring takes its
// ends from the ring's first / last kept position. Each file keeps what is its own: how a record is seeded, how far a vertex is
// from its chord, how ties among the farthest are broken, and its extern "C" entry points.
//
//   round   carry    one work-group: for every block of 256 positions the last kept position before it and the first after it
//           cross    (the file's) dp_neighbours gives every undecided vertex its chord: previous / next kept position by block
//                    scan + carry; vertices beyond the tolerance are candidates and take part in a 64-bit atomic max on the
//                    slot of their segment (= the position of its first end); the slots of the OTHER parity are reset
//           tie(s)   (the file's) atomic min among the candidates that equal the maximum
//           keep     (the file's win test) dp_keep: the winner is kept; the round's counter is raised
//   finish  count    kept positions per block of 256
//           scan     one work-group: exclusive prefix sum of the block counts; the header record
//           scatter  per kept position: vertex and input index to their compacted place; the prefix of every position
//           records  per record: start and count in the compacted array, sums and box cleared
//           reduce   per compacted vertex: shoelace term of a ring, box (folded over the runs of a wave before the atomics)
//           close    per record: half-open box, the collapsed flag
//
// A candidate is a vertex that passes the threshold ITSELF: within one segment the chord is fixed, so the maximum passes iff any
// vertex does, and then it is the maximum over the candidates; vertices within the tolerance issue no atomic and late rounds are
// almost free. A round whose predecessor kept nothing returns at once (every kernel asks dp_idle first). The kept set only
// grows; the first / last kept position of every block and record is kept up to date by the atomics of the thread that keeps a
// vertex (dp_note_kept), so no round re-derives them. No work-group waits on another: everything a kernel reads was written by
// an earlier launch; within a launch work-groups meet only in relaxed agent-scope integer atomics (max, min, add), whose arrival
// order changes nothing. The shoelace sum is added modulo 2^64, which is exact wherever the true area2 fits an int64.
// The kernels are templates (on the work-group size or the record type): the header is included by two files of a library
// linked without relocatable device code.
#pragma once
#include "scene_common.h"
#include "block_scan.h"
#include <limits.h>
#include <stddef.h>
#include <stdio.h>

#define DP_THREADS 256
#define DP_WAVES (DP_THREADS / INSAR_WAVE)
#define DP_MAX_ROUNDS 4095
#define DP_COUNTERS 4096
#define DP_MAX_VERTICES (1 << 28)

#define DP_ADD(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define DP_MIN(p, v) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define DP_MAX(p, v) __hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

typedef unsigned long long dp_u64;

// the sections of the scratch buffer that both tools have; SmBuf and CsBuf add their seeds and segment slots
struct DpCore {
  int* changed;              // [DP_COUNTERS] vertices kept per round; slot max_rounds is the probe. At offset 0 of the scratch.
  uint8_t* keep;             // [vm]
  int* lineof;               // [vm] the record of a position
  int* seg;                  // [vm] candidate: position of the first end of its segment, else -1
  dp_u64* dev;               // [vm] candidate: its deviation from the chord, in the tool's own measure
  int* pos;                  // [vm + 1] kept positions before this one
  int *bmax, *bmin;          // [blocks] last / first kept position of the block, -1 / INT_MAX
  int *cmax, *cmin;          // [blocks] last kept position before the block, first after it
  int* bsum;                 // [blocks]
  int *firstk, *lastk;       // [records] first / last kept position of the record, INT_MAX / -1
  int vm;                    // the capacity the parities of the segment slots are spaced by
};

// InsarRing and InsarContourLine share one 48-byte layout; what differs is whether a record can be open
__device__ __forceinline__ bool dp_closed(const InsarRing&) { return true; }
__device__ __forceinline__ bool dp_closed(const InsarContourLine& l) { return l.closed != 0; }
__device__ __forceinline__ void dp_clean(InsarRing&) {}
__device__ __forceinline__ void dp_clean(InsarContourLine& l) { l.closed = l.closed != 0; }

// a round whose predecessor kept nothing has nothing to do
__device__ __forceinline__ bool dp_idle(const DpCore& b, int rd) { return rd > 0 && b.changed[rd - 1] == 0; }

// position i of record r becomes a kept vertex
__device__ __forceinline__ void dp_note_kept(const DpCore& b, int i, int r) {
  DP_MIN(&b.firstk[r], i);
  DP_MAX(&b.lastk[r], i);
  DP_MAX(&b.bmax[i / DP_THREADS], i);
  DP_MIN(&b.bmin[i / DP_THREADS], i);
}

// the core's share of element i of a tool's clear kernel
__device__ __forceinline__ void dp_clear(const DpCore& b, int i, int nblk, int nrec) {
  if (i < DP_COUNTERS) b.changed[i] = 0;
  if (i < nblk) {
    b.bmax[i] = -1;
    b.bmin[i] = INT_MAX;
  }
  if (i < nrec) {
    b.firstk[i] = INT_MAX;
    b.lastk[i] = -1;
  }
}

// the last record whose start is <= i
template <typename Rec>
__device__ __forceinline__ int dp_record_of(const Rec* recs, int nrec, int i) {
  int lo = 0, hi = nrec - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (recs[mid].start <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The chord of position i, for every thread of the work-group (it synchronises): *p is the previous kept position (the id of the
// segment), (dy, dx) the next kept position and (py, px) the vertex itself, both relative to *p. False for a kept vertex, a
// position past the end, and ends out of range (never, for a record table that matches the vertex array).
struct DpChord { long long py, px, dy, dx; };
template <typename Rec>
__device__ __forceinline__ bool dp_neighbours(const DpCore& b, const int* verts, int nv, const Rec* recs, int i, int* w, int* p_out,
                                              DpChord* c) {
  const bool live = i < nv;
  const bool kept = live && b.keep[i];
  int total;
  int p = block_prefix_max<DP_THREADS>(kept ? i : -1, w, &total);
  int q = block_suffix_min<DP_THREADS>(kept ? i : INT_MAX, w, &total);
  const int cp = b.cmax[blockIdx.x], cq = b.cmin[blockIdx.x];
  p = cp > p ? cp : p;
  q = cq < q ? cq : q;
  if (!live || kept) return false;
  const int r = b.lineof[i];
  const int s = recs[r].start, e = s + recs[r].count;
  if (p < s) p = b.lastk[r];                                     // rings only: an open line keeps both of its ends
  if (q >= e) q = b.firstk[r];
  if (p < 0 || p >= nv || q < 0 || q >= nv) return false;
  const int ay = verts[2 * (int64_t)p], ax = verts[2 * (int64_t)p + 1];
  c->py = (long long)verts[2 * (int64_t)i] - ay;
  c->px = (long long)verts[2 * (int64_t)i + 1] - ax;
  c->dy = (long long)verts[2 * (int64_t)q] - ay;
  c->dx = (long long)verts[2 * (int64_t)q + 1] - ax;
  *p_out = p;
  return true;
}

// the end of a cross kernel: the largest deviation among the candidates of a segment, on the slot of this round's parity
__device__ __forceinline__ void dp_raise_max(dp_u64* segmax, int sg, dp_u64 num) {
  const WaveRuns runs = wave_runs(sg);
  const dp_u64 mx = wave_run_reduce(runs, num, WaveMax());
  if (runs.head && sg >= 0) DP_MAX(&segmax[sg], mx);
}

// the end of a keep kernel: the winner is kept (not by the probe), the round's counter counts the winners
__device__ __forceinline__ void dp_keep(const DpCore& b, int i, bool win, int apply, int rd) {
  if (win && apply) {
    b.keep[i] = 1;
    dp_note_kept(b, i, b.lineof[i]);
  }
  const int n = __popcll(__ballot(win));
  if ((int)__lane_id() == 0 && n) DP_ADD(&b.changed[rd], n);
}

// ---------------------------------------------------------------------------------------------
// one round: carry
// ---------------------------------------------------------------------------------------------
// One work-group: cmax[j] = max of bmax over the blocks before j, cmin[j] = min of bmin over the blocks after j.
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
dp_carry_kernel(DpCore b, int nblk, int rd) {
  __shared__ int w[THREADS / INSAR_WAVE];
  if (dp_idle(b, rd)) return;
  block_carry<THREADS>(b.bmax, b.bmin, b.cmax, b.cmin, nblk, w);
}

// ---------------------------------------------------------------------------------------------
// finish: count / scan / scatter / records / reduce / close
// ---------------------------------------------------------------------------------------------
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
dp_count_kernel(DpCore b, int nv) {
  __shared__ int w[THREADS / INSAR_WAVE];
  const int i = blockIdx.x * THREADS + threadIdx.x;
  int total;
  block_prefix_sum<THREADS>(i < nv ? (int)b.keep[i] : 0, w, &total);
  if (threadIdx.x == 0) b.bsum[blockIdx.x] = total;
}

// One work-group: bsum becomes its exclusive prefix sum; the header record, as 12 int32 slots: 2 = records (label / level),
// 3 = rounds (leader), 4 = converged (start), 5 = kept vertices (count), 6 = input vertices (edges / closed), the rest 0.
template <typename Rec>
__global__ void __launch_bounds__(DP_THREADS)
dp_scan_kernel(DpCore b, int nblk, int nv, int nrec, int max_rounds, Rec* __restrict__ table) {
  static_assert(sizeof(Rec) == 48 && offsetof(Rec, leader) == 12 && offsetof(Rec, start) == 16 && offsetof(Rec, count) == 20,
                "the header is written as three 16-byte stores");
  __shared__ int w[DP_WAVES];
  __shared__ int rounds;
  if (threadIdx.x == 0) rounds = 0;
  const int carry = block_scan_array<DP_THREADS>(b.bsum, nblk, w);
  int mine = 0;
  for (int r = threadIdx.x; r < max_rounds; r += DP_THREADS) mine += b.changed[r] != 0;
  if (mine) atomicAdd(&rounds, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    int4* h = reinterpret_cast<int4*>(table);
    h[0] = make_int4(0, 0, nrec, rounds);
    h[1] = make_int4(b.changed[max_rounds] == 0, carry, nv, 0);
    h[2] = make_int4(0, 0, 0, 0);
  }
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS)
dp_scatter_kernel(DpCore b, const int* __restrict__ verts, int nv, int* __restrict__ out_verts, int* __restrict__ out_kept) {
  __shared__ int w[THREADS / INSAR_WAVE];
  const int i = blockIdx.x * THREADS + threadIdx.x;
  const int k = i < nv ? (int)b.keep[i] : 0;
  int total;
  const int at = b.bsum[blockIdx.x] + block_prefix_sum<THREADS>(k, w, &total);
  if (i >= nv) return;
  b.pos[i] = at;
  if (i == nv - 1) b.pos[nv] = at + k;
  if (k) {
    *reinterpret_cast<int2*>(out_verts + 2 * (int64_t)at) = make_int2(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
    out_kept[at] = i;
  }
}

template <typename Rec>
__global__ void __launch_bounds__(DP_THREADS)
dp_records_kernel(DpCore b, const Rec* __restrict__ recs, int nrec, int nv, Rec* __restrict__ table) {
  const int r = blockIdx.x * DP_THREADS + threadIdx.x;
  if (r >= nrec) return;
  Rec o = recs[r];
  const int s = min(max(o.start, 0), nv), e = min(max(s + o.count, s), nv);     // no clamp bites on a table that matches the array
  o.area2 = 0;
  o.start = b.pos[s];
  o.count = b.pos[e] - o.start;
  dp_clean(o);
  o.y0 = o.x0 = INT_MAX;
  o.y1 = o.x1 = INT_MIN;
  o._pad = 0;
  table[1 + r] = o;
}

template <typename Rec>
__global__ void __launch_bounds__(DP_THREADS)
dp_reduce_kernel(DpCore b, const int* __restrict__ out_verts, const int* __restrict__ out_kept, int nv, Rec* __restrict__ table) {
  const int j = blockIdx.x * DP_THREADS + threadIdx.x;
  const int kept = min(table[0].count, nv);
  int r = -1, y = 0, x = 0;
  dp_u64 term = 0ull;
  if (j < kept) {
    r = b.lineof[min(max(out_kept[j], 0), nv - 1)];
    const Rec* o = table + 1 + r;
    y = out_verts[2 * (int64_t)j];
    x = out_verts[2 * (int64_t)j + 1];
    if (dp_closed(*o)) {
      int nx = j + 1 < o->start + o->count ? j + 1 : o->start;
      if (nx < 0 || nx >= kept) nx = j;                            // never, for a table that matches the array
      const int yn = out_verts[2 * (int64_t)nx], xn = out_verts[2 * (int64_t)nx + 1];
      term = (dp_u64)((long long)x * yn) - (dp_u64)((long long)xn * y);
    }
  }
  const WaveRuns runs = wave_runs(r);
  const dp_u64 sum = wave_run_reduce(runs, term, WaveAdd());
  const int y0 = wave_run_reduce(runs, y, WaveMin()), x0 = wave_run_reduce(runs, x, WaveMin());
  const int y1 = wave_run_reduce(runs, y, WaveMax()), x1 = wave_run_reduce(runs, x, WaveMax());
  if (runs.head && r >= 0) {
    Rec* o = table + 1 + r;
    if (sum) DP_ADD(reinterpret_cast<dp_u64*>(&o->area2), sum);
    DP_MIN(&o->y0, y0);
    DP_MIN(&o->x0, x0);
    DP_MAX(&o->y1, y1);
    DP_MAX(&o->x1, x1);
  }
}

template <typename Rec>
__global__ void __launch_bounds__(DP_THREADS)
dp_close_kernel(int nrec, Rec* __restrict__ table) {
  const int r = blockIdx.x * DP_THREADS + threadIdx.x;
  if (r >= nrec) return;
  Rec* o = table + 1 + r;
  o->y1 += 1;
  o->x1 += 1;
  o->_pad = dp_closed(*o) && (o->count < 3 || o->area2 == 0);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#define DP_CORE_SECTIONS 13
#define DP_MAX_OWN 8
struct DpLayout { int64_t off[DP_CORE_SECTIONS + DP_MAX_OWN]; int64_t bytes, table_bytes; };

// The capacities against their caps, then the offsets of the core's sections followed by the tool's n_own sections of own[]
// bytes, each rounded up to 16 bytes. `noun` is what the tool calls a record ("ring", "line").
static inline int dp_layout(const char* who, const char* noun, int32_t max_vertices, int32_t max_records, int32_t cap_records,
                            const int64_t* own, int n_own, DpLayout* l) {
  if (max_vertices < 1 || max_vertices > DP_MAX_VERTICES)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_vertices %d outside 1..%d", who, max_vertices, DP_MAX_VERTICES);
  if (max_records < 1 || max_records > cap_records)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_%ss %d outside 1..%d", who, noun, max_records, cap_records);
  const int64_t vm = max_vertices, rm = max_records, nb = (vm + DP_THREADS - 1) / DP_THREADS;
  // the order of DpCore: changed keep lineof seg dev pos bmax bmin cmax cmin bsum firstk lastk
  const int64_t core[DP_CORE_SECTIONS] = {4 * DP_COUNTERS, vm, 4 * vm, 4 * vm, 8 * vm, 4 * (vm + 1), 4 * nb, 4 * nb, 4 * nb, 4 * nb, 4 * nb,
                                          4 * rm, 4 * rm};
  ScratchTake take;
  for (int k = 0; k < DP_CORE_SECTIONS + n_own; ++k) l->off[k] = take(k < DP_CORE_SECTIONS ? core[k] : own[k - DP_CORE_SECTIONS]);
  l->bytes = take.at;
  l->table_bytes = (int64_t)48 * (1 + rm);
  return INSAR_OK;
}

// the core's pointers into a scratch laid out by dp_layout; the tool's own sections start at l.off[DP_CORE_SECTIONS]
static inline void dp_carve(const DpLayout& l, void* scratch, int32_t max_vertices, DpCore* b) {
  b->changed = scratch_at<int>(scratch, l.off[0]);
  b->keep = scratch_at<uint8_t>(scratch, l.off[1]);
  b->lineof = scratch_at<int>(scratch, l.off[2]);
  b->seg = scratch_at<int>(scratch, l.off[3]);
  b->dev = scratch_at<dp_u64>(scratch, l.off[4]);
  b->pos = scratch_at<int>(scratch, l.off[5]);
  b->bmax = scratch_at<int>(scratch, l.off[6]);
  b->bmin = scratch_at<int>(scratch, l.off[7]);
  b->cmax = scratch_at<int>(scratch, l.off[8]);
  b->cmin = scratch_at<int>(scratch, l.off[9]);
  b->bsum = scratch_at<int>(scratch, l.off[10]);
  b->firstk = scratch_at<int>(scratch, l.off[11]);
  b->lastk = scratch_at<int>(scratch, l.off[12]);
  b->vm = max_vertices;
}

// What setup, rounds and finish share, behind dp_layout: the vertex array, the input record table, the counts against the
// capacities, the scratch. A record has at least `least` vertices (a ring one, a line two).
static inline int dp_check(const char* who, const char* noun, const int32_t* vertices, int32_t n_vertices, const void* records,
                           int32_t n_records, int least, int32_t max_vertices, int32_t max_records, const void* scratch) {
  char nouns[16];
  snprintf(nouns, sizeof nouns, "%ss", noun);
  if (!vertices || !records || !scratch)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !vertices ? "vertices" : !records ? nouns : "scratch");
  if (n_vertices < 1 || n_vertices > max_vertices) INSAR_FAIL(INSAR_E_SHAPE, "%s: n_vertices %d outside 1..max_vertices = %d", who, n_vertices, max_vertices);
  if (n_records < 1 || n_records > max_records)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: n_%s %d outside 1..max_%s = %d", who, nouns, n_records, nouns, max_records);
  if ((int64_t)least * n_records > (int64_t)n_vertices) INSAR_FAIL(INSAR_E_SHAPE, "%s: %d %s over %d vertices", who, n_records, nouns, n_vertices);
  if (((uintptr_t)vertices) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: vertices not 8-byte aligned", who);
  if (!insar_aligned16(records) || !insar_aligned16(scratch)) INSAR_FAIL(INSAR_E_ALIGN, "%s: %s / scratch not 16-byte aligned", who, nouns);
  return INSAR_OK;
}

static inline int dp_check_max_rounds(const char* who, int32_t max_rounds) {
  if (max_rounds < 1 || max_rounds > DP_MAX_ROUNDS) INSAR_FAIL(INSAR_E_ARG, "%s: max_rounds %d outside 1..%d", who, max_rounds, DP_MAX_ROUNDS);
  return INSAR_OK;
}
static inline int dp_check_rounds(const char* who, int32_t first_round, int32_t n_rounds, int32_t max_rounds) {
  if (int rc = dp_check_max_rounds(who, max_rounds)) return rc;
  if (first_round < 0 || n_rounds < 1 || (int64_t)first_round + n_rounds > (int64_t)max_rounds + 1)
    INSAR_FAIL(INSAR_E_ARG, "%s: rounds %d..%d+%d outside 0..max_rounds = %d (the last one is the probe)", who, first_round, first_round,
               n_rounds, max_rounds);
  return INSAR_OK;
}

static inline int dp_launches(int per_call, int per_round, int32_t rounds) {
  return per_call + per_round * (rounds < 0 ? 0 : rounds > DP_MAX_ROUNDS + 1 ? DP_MAX_ROUNDS + 1 : rounds);
}

// rounds first_round .. first_round + n_rounds - 1: the carry, then the tool's own launches, tool_round(rd, apply)
template <typename F>
static inline int dp_rounds(const char* who, const DpCore& b, int nblk, int first_round, int n_rounds, int max_rounds, hipStream_t s,
                            F tool_round) {
  for (int rd = first_round; rd < first_round + n_rounds; ++rd) {
    hipLaunchKernelGGL(dp_carry_kernel<DP_THREADS>, dim3(1), dim3(DP_THREADS), 0, s, b, nblk, rd);
    tool_round(rd, (int)(rd < max_rounds));
  }
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

// the whole of a finish entry point behind dp_check: max_rounds, the outputs, the six launches
template <typename Rec>
static inline int dp_finish(const char* who, const DpCore& b, const int32_t* vertices, int32_t n_vertices, const void* records,
                            int32_t n_records, int32_t max_rounds, void* table, int32_t* out_vertices, int32_t* out_kept, void* stream) {
  if (int rc = dp_check_max_rounds(who, max_rounds)) return rc;
  if (!table || !out_vertices || !out_kept)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !table ? "table" : !out_vertices ? "out_vertices" : "out_kept");
  if (!insar_aligned16(table)) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 16-byte aligned", who);
  if ((((uintptr_t)out_vertices) & 7u) || (((uintptr_t)out_kept) & 3u))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: out_vertices not 8-byte or out_kept not 4-byte aligned", who);
  const int nv = n_vertices, nrec = n_records, nblk = (nv + DP_THREADS - 1) / DP_THREADS;
  const Rec* in = (const Rec*)records + 1;
  Rec* t = (Rec*)table;
  const dim3 grid(nblk), rgrid((nrec + DP_THREADS - 1) / DP_THREADS), block(DP_THREADS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dp_count_kernel<DP_THREADS>, grid, block, 0, s, b, nv);
  hipLaunchKernelGGL(dp_scan_kernel<Rec>, dim3(1), block, 0, s, b, nblk, nv, nrec, (int)max_rounds, t);
  hipLaunchKernelGGL(dp_scatter_kernel<DP_THREADS>, grid, block, 0, s, b, (const int*)vertices, nv, (int*)out_vertices, (int*)out_kept);
  hipLaunchKernelGGL(dp_records_kernel<Rec>, rgrid, block, 0, s, b, in, nrec, nv, t);
  hipLaunchKernelGGL(dp_reduce_kernel<Rec>, grid, block, 0, s, b, (const int*)out_vertices, (const int*)out_kept, nv, t);
  hipLaunchKernelGGL(dp_close_kernel<Rec>, rgrid, block, 0, s, nrec, t);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
