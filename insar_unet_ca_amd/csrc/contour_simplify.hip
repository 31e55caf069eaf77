// Contour simplification: Douglas-Peucker over the polylines of the contour lines (contour.hip), open lines and closed rings,
// in exact integers at coordinates up to 2^30. Semantics: include/insar_hip.h, "contour simplification". The round and finish
// stages, the scratch core and the host checks are those of dp_common.h; this file owns how a line is seeded, the deviation of
// a vertex and the tie-break. An open line keeps both ends from the start, so none of its segments ever wraps.
//
//   setup   clear    counters, both parities of the segment slots, the block and line records
//           mark     per vertex: its line; the two ends of an open line are kept; per ring the smallest key (Y << 32 | X)
//           far      per ring vertex: the squared distance from seed 1, a 64-bit atomic max per ring; the smallest position that
//                    carries the smallest key is seed 1
//           tie      per ring vertex at that distance: atomic min of its key
//           pos      per ring vertex at that distance with that key: atomic min of its position, which is seed 2
//           seed     per ring vertex: the positions of seed 1 and seed 2 are kept
//   round   cross    |cross| against the chord of dp_neighbours
//           tie      per candidate that equals the maximum: atomic min of its key on the segment's second slot
//           pos      per candidate that equals both: atomic min of its position on the segment's third slot
//           keep     the candidate at that position is kept
//
// 6 + 5 per round + 6 launches. Ties go to the smallest (Y, X), then to the smallest position.
// Exactness: coordinates in 0 .. 2^30, so differences stay within +-2^30, each product within 2^60, |cross| (twice the area of a
// triangle inside the square) <= 2^60 and d^2 <= 2^61: both fit 64 bits, and the per-segment maximum needs no square. Only the
// keep test does: cross^2 <= 2^120 against eps2 |b - a|^2 <= 2^36 * 2^61, compared as unsigned 128-bit integers. No float anywhere.
#include "dp_common.h"

#define CS_MAX_LINES (1 << 27)
#define CS_MAX_EPS 262144ll                // round(1024 * 256)

typedef unsigned __int128 cs_u128;

// the scratch: the core, the segment slots of both parities, the seeds of every ring
struct CsBuf : DpCore {
  dp_u64* segmax;            // [2][vm] largest |cross| (or squared distance from a degenerate chord) of the segment
  dp_u64* segkey;            // [2][vm] smallest key among those
  int* segpos;               // [2][vm] smallest position among those
  dp_u64 *s1key, *s2d2, *s2key;   // [lines] rings: smallest key; largest d^2 from it, the smallest key at that distance
  int *s1pos, *s2pos;        // [lines] rings: the positions of the two seeds
};

__device__ __forceinline__ dp_u64 cs_key(int y, int x) { return ((dp_u64)(unsigned int)y << 32) | (dp_u64)(unsigned int)x; }

// the squared distance of (y, x) from the point a key holds
__device__ __forceinline__ dp_u64 cs_dist2(int y, int x, dp_u64 key) {
  const long long dy = (long long)y - (long long)(int)(key >> 32), dx = (long long)x - (long long)(int)(key & 0xffffffffull);
  return (dp_u64)(dy * dy + dx * dx);
}

// ---------------------------------------------------------------------------------------------
// setup: clear / mark / far / tie / pos / seed
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DP_THREADS)
csimplify_clear_kernel(CsBuf b, int nv, int nl, int nblk) {
  const int n = max(max(nv, nl), max(nblk, DP_COUNTERS));
  for (int i = blockIdx.x * DP_THREADS + threadIdx.x; i < n; i += gridDim.x * DP_THREADS) {
    dp_clear(b, i, nblk, nl);
    if (i < nv) {
      b.segmax[i] = 0ull;
      b.segmax[(int64_t)b.vm + i] = 0ull;
      b.segkey[i] = ~0ull;
      b.segkey[(int64_t)b.vm + i] = ~0ull;
      b.segpos[i] = INT_MAX;
      b.segpos[(int64_t)b.vm + i] = INT_MAX;
    }
    if (i < nl) {
      b.s1key[i] = ~0ull;
      b.s2d2[i] = 0ull;
      b.s2key[i] = ~0ull;
      b.s1pos[i] = INT_MAX;
      b.s2pos[i] = INT_MAX;
    }
  }
}

__global__ void __launch_bounds__(DP_THREADS)
csimplify_mark_kernel(CsBuf b, const int* __restrict__ verts, int nv, const InsarContourLine* __restrict__ lines, int nl) {
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  int ring = -1;
  dp_u64 key = ~0ull;
  if (i < nv) {
    const int lo = dp_record_of(lines, nl, i);
    const int s = lines[lo].start, e = s + lines[lo].count;
    const bool closed = lines[lo].closed != 0;
    const bool end = !closed && (i == s || i == e - 1);
    b.lineof[i] = lo;
    b.keep[i] = (uint8_t)end;
    if (end) dp_note_kept(b, i, lo);
    if (closed) {
      ring = lo;
      key = cs_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
    }
  }
  const WaveRuns runs = wave_runs(ring);
  const dp_u64 mn = wave_run_reduce(runs, key, WaveMin());
  if (runs.head && ring >= 0) DP_MIN(&b.s1key[ring], mn);
}

// the ring of position i, or -1 (an open line, or past the end); its key
__device__ __forceinline__ int cs_ring_of(const CsBuf& b, const int* verts, int nv, const InsarContourLine* lines, int i, dp_u64* key) {
  if (i >= nv) return -1;
  const int r = b.lineof[i];
  if (lines[r].closed == 0) return -1;
  *key = cs_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
  return r;
}

__global__ void __launch_bounds__(DP_THREADS)
csimplify_far_kernel(CsBuf b, const int* __restrict__ verts, int nv, const InsarContourLine* __restrict__ lines) {
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  dp_u64 key = 0ull, d2 = 0ull;
  int first = INT_MAX;
  const int r = cs_ring_of(b, verts, nv, lines, i, &key);
  if (r >= 0) {
    const dp_u64 s1 = b.s1key[r];
    d2 = cs_dist2((int)(key >> 32), (int)(key & 0xffffffffull), s1);
    if (key == s1) first = i;
  }
  const WaveRuns runs = wave_runs(r);
  const dp_u64 mx = wave_run_reduce(runs, d2, WaveMax());
  const int mn = wave_run_reduce(runs, first, WaveMin());
  if (runs.head && r >= 0) {
    DP_MAX(&b.s2d2[r], mx);
    if (mn != INT_MAX) DP_MIN(&b.s1pos[r], mn);
  }
}

// with_key = 0: the smallest key among the ring's vertices at the largest distance; 1: the smallest position among those
__global__ void __launch_bounds__(DP_THREADS)
csimplify_far_tie_kernel(CsBuf b, const int* __restrict__ verts, int nv, const InsarContourLine* __restrict__ lines, int with_key) {
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  dp_u64 key = 0ull;
  int r = cs_ring_of(b, verts, nv, lines, i, &key);
  if (r >= 0) {
    const bool far = cs_dist2((int)(key >> 32), (int)(key & 0xffffffffull), b.s1key[r]) == b.s2d2[r];
    if (!far || (with_key && key != b.s2key[r])) r = -1;
  }
  const WaveRuns runs = wave_runs(r);
  if (with_key) {
    const int mn = wave_run_reduce(runs, i, WaveMin());
    if (runs.head && r >= 0) DP_MIN(&b.s2pos[r], mn);
  } else {
    const dp_u64 mn = wave_run_reduce(runs, key, WaveMin());
    if (runs.head && r >= 0) DP_MIN(&b.s2key[r], mn);
  }
}

__global__ void __launch_bounds__(DP_THREADS)
csimplify_seed_kernel(CsBuf b, int nv, const InsarContourLine* __restrict__ lines) {
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  if (i >= nv) return;
  const int r = b.lineof[i];
  if (lines[r].closed == 0) return;
  if (i == b.s1pos[r] || i == b.s2pos[r]) {
    b.keep[i] = 1;
    dp_note_kept(b, i, r);
  }
}

// ---------------------------------------------------------------------------------------------
// one round: (carry) / cross / tie / pos / keep
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DP_THREADS)
csimplify_cross_kernel(CsBuf b, const int* __restrict__ verts, int nv, const InsarContourLine* __restrict__ lines, long long eps2, int rd) {
  __shared__ int w[DP_WAVES];
  if (dp_idle(b, rd)) return;
  const int par = rd & 1;
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  int p = -1, sg = -1;
  DpChord c;
  const bool undecided = dp_neighbours(b, verts, nv, lines, i, w, &p, &c);
  dp_u64 num = 0ull;
  if (i < nv) {
    const int64_t other = (int64_t)(par ^ 1) * b.vm + i;         // nobody reads the other parity during this round
    b.segmax[other] = 0ull;
    b.segkey[other] = ~0ull;
    b.segpos[other] = INT_MAX;
    if (undecided) {
      const dp_u64 len2 = (dp_u64)(c.dy * c.dy + c.dx * c.dx);
      dp_u64 n;
      bool beyond;
      if (len2) {
        const long long cr = c.dx * c.py - c.dy * c.px;
        n = (dp_u64)(cr < 0 ? -cr : cr);
        beyond = (cs_u128)n * n > (cs_u128)(dp_u64)eps2 * len2;
      } else {                                                   // a chord whose ends coincide: the distance from that point
        n = (dp_u64)(c.py * c.py + c.px * c.px);
        beyond = n > (dp_u64)eps2;
      }
      if (beyond) {
        sg = p;
        num = n;
      }
    }
    b.seg[i] = sg;
    b.dev[i] = num;
  }
  dp_raise_max(b.segmax + (int64_t)par * b.vm, sg, num);
}

// with_key = 0: the smallest key among the candidates that equal their segment's maximum; 1: the smallest position among those
__global__ void __launch_bounds__(DP_THREADS)
csimplify_tie_kernel(CsBuf b, const int* __restrict__ verts, int nv, int rd, int with_key) {
  if (dp_idle(b, rd)) return;
  const int par = rd & 1;
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  int sg = i < nv ? b.seg[i] : -1;
  dp_u64 key = ~0ull;
  if (sg >= 0) {
    const int64_t slot = (int64_t)par * b.vm + sg;
    key = cs_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
    if (b.dev[i] != b.segmax[slot] || (with_key && key != b.segkey[slot])) {
      sg = -1;
      key = ~0ull;
    }
  }
  const WaveRuns runs = wave_runs(sg);
  if (with_key) {
    const int mn = wave_run_reduce(runs, i, WaveMin());
    if (runs.head && sg >= 0) DP_MIN(&b.segpos[(int64_t)par * b.vm + sg], mn);
  } else {
    const dp_u64 mn = wave_run_reduce(runs, key, WaveMin());
    if (runs.head && sg >= 0) DP_MIN(&b.segkey[(int64_t)par * b.vm + sg], mn);
  }
}

__global__ void __launch_bounds__(DP_THREADS)
csimplify_keep_kernel(CsBuf b, int nv, int rd, int apply) {
  if (dp_idle(b, rd)) return;
  const int par = rd & 1;
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  const int sg = i < nv ? b.seg[i] : -1;
  dp_keep(b, i, sg >= 0 && b.segpos[(int64_t)par * b.vm + sg] == i, apply, rd);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int csimplify_layout(const char* who, int32_t max_vertices, int32_t max_lines, DpLayout* l) {
  const int64_t vm = max_vertices, lm = max_lines;
  // segmax segkey segpos s1key s2d2 s2key s1pos s2pos
  const int64_t own[8] = {16 * vm, 16 * vm, 8 * vm, 8 * lm, 8 * lm, 8 * lm, 4 * lm, 4 * lm};
  return dp_layout(who, "line", max_vertices, max_lines, CS_MAX_LINES, own, 8, l);
}

static CsBuf csimplify_buf(const DpLayout& l, void* scratch, int32_t max_vertices) {
  const int64_t* own = l.off + DP_CORE_SECTIONS;
  CsBuf b;
  dp_carve(l, scratch, max_vertices, &b);
  b.segmax = scratch_at<dp_u64>(scratch, own[0]);
  b.segkey = scratch_at<dp_u64>(scratch, own[1]);
  b.segpos = scratch_at<int>(scratch, own[2]);
  b.s1key = scratch_at<dp_u64>(scratch, own[3]);
  b.s2d2 = scratch_at<dp_u64>(scratch, own[4]);
  b.s2key = scratch_at<dp_u64>(scratch, own[5]);
  b.s1pos = scratch_at<int>(scratch, own[6]);
  b.s2pos = scratch_at<int>(scratch, own[7]);
  return b;
}

static int csimplify_check(const char* who, const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines,
                           int32_t max_vertices, int32_t max_lines, const void* scratch, DpLayout* l) {
  if (int rc = csimplify_layout(who, max_vertices, max_lines, l)) return rc;
  return dp_check(who, "line", vertices, n_vertices, lines, n_lines, 2, max_vertices, max_lines, scratch);     // a line has two ends
}

extern "C" int insar_contour_simplify_scratch_bytes(int32_t max_vertices, int32_t max_lines, int64_t* scratch_bytes, int64_t* table_bytes) {
  const char* who = "insar_contour_simplify_scratch_bytes";
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  DpLayout l;
  if (int rc = csimplify_layout(who, max_vertices, max_lines, &l)) return rc;
  *scratch_bytes = l.bytes;
  *table_bytes = l.table_bytes;
  return INSAR_OK;
}

extern "C" int insar_contour_simplify_launches(int32_t rounds) { return dp_launches(12, 5, rounds); }

extern "C" int insar_contour_simplify_setup(const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines,
                                            int32_t max_vertices, int32_t max_lines, void* scratch, void* stream) {
  const char* who = "insar_contour_simplify_setup";
  DpLayout l;
  if (int rc = csimplify_check(who, vertices, n_vertices, lines, n_lines, max_vertices, max_lines, scratch, &l)) return rc;
  const CsBuf b = csimplify_buf(l, scratch, max_vertices);
  const int nv = n_vertices, nblk = (nv + DP_THREADS - 1) / DP_THREADS;
  const InsarContourLine* lin = (const InsarContourLine*)lines + 1;
  const int* v = (const int*)vertices;
  const dim3 grid(nblk), block(DP_THREADS);
  hipStream_t s = (hipStream_t)stream;
  const int nclear = nv > DP_COUNTERS ? nv : DP_COUNTERS;
  hipLaunchKernelGGL(csimplify_clear_kernel, dim3(insar_grid_cap((nclear + DP_THREADS - 1) / DP_THREADS)), block, 0, s, b, nv, (int)n_lines, nblk);
  hipLaunchKernelGGL(csimplify_mark_kernel, grid, block, 0, s, b, v, nv, lin, (int)n_lines);
  hipLaunchKernelGGL(csimplify_far_kernel, grid, block, 0, s, b, v, nv, lin);
  hipLaunchKernelGGL(csimplify_far_tie_kernel, grid, block, 0, s, b, v, nv, lin, 0);
  hipLaunchKernelGGL(csimplify_far_tie_kernel, grid, block, 0, s, b, v, nv, lin, 1);
  hipLaunchKernelGGL(csimplify_seed_kernel, grid, block, 0, s, b, nv, lin);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_contour_simplify_rounds(const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines, int64_t eps2,
                                             int32_t first_round, int32_t n_rounds, int32_t max_rounds, int32_t max_vertices,
                                             int32_t max_lines, void* scratch, void* stream) {
  const char* who = "insar_contour_simplify_rounds";
  DpLayout l;
  if (int rc = csimplify_check(who, vertices, n_vertices, lines, n_lines, max_vertices, max_lines, scratch, &l)) return rc;
  if (eps2 < 0 || eps2 > CS_MAX_EPS * CS_MAX_EPS)
    INSAR_FAIL(INSAR_E_ARG, "%s: eps2 %lld outside 0..%lld", who, (long long)eps2, CS_MAX_EPS * CS_MAX_EPS);
  if (int rc = dp_check_rounds(who, first_round, n_rounds, max_rounds)) return rc;
  const CsBuf b = csimplify_buf(l, scratch, max_vertices);
  const int nv = n_vertices, nblk = (nv + DP_THREADS - 1) / DP_THREADS;
  const InsarContourLine* lin = (const InsarContourLine*)lines + 1;
  const int* v = (const int*)vertices;
  const dim3 grid(nblk), block(DP_THREADS);
  hipStream_t s = (hipStream_t)stream;
  return dp_rounds(who, b, nblk, first_round, n_rounds, max_rounds, s, [&](int rd, int apply) {
    hipLaunchKernelGGL(csimplify_cross_kernel, grid, block, 0, s, b, v, nv, lin, (long long)eps2, rd);
    hipLaunchKernelGGL(csimplify_tie_kernel, grid, block, 0, s, b, v, nv, rd, 0);
    hipLaunchKernelGGL(csimplify_tie_kernel, grid, block, 0, s, b, v, nv, rd, 1);
    hipLaunchKernelGGL(csimplify_keep_kernel, grid, block, 0, s, b, nv, rd, apply);
  });
}

extern "C" int insar_contour_simplify_finish(const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines,
                                             int32_t max_rounds, int32_t max_vertices, int32_t max_lines, void* scratch, void* table,
                                             int32_t* out_vertices, int32_t* out_kept, void* stream) {
  const char* who = "insar_contour_simplify_finish";
  DpLayout l;
  if (int rc = csimplify_check(who, vertices, n_vertices, lines, n_lines, max_vertices, max_lines, scratch, &l)) return rc;
  return dp_finish<InsarContourLine>(who, csimplify_buf(l, scratch, max_vertices), vertices, n_vertices, lines, n_lines, max_rounds,
                                     table, out_vertices, out_kept, stream);
}
