// Contour simplification: Douglas-Peucker over the polylines of the contour lines (contour.hip), open lines and closed rings,
// in exact integers at coordinates up to 2^30. Semantics: include/insar_hip.h, "contour simplification". The round structure is
// that of simplify.hip: every array below is indexed by the POSITION of a vertex in the input vertex array (line after line);
// rings are not rotated: a segment that wraps over the end of its ring takes its ends from the ring's first / last kept
// position. An open line keeps both ends from the start, so none of its segments ever wraps.
//
//   setup   clear    counters, both parities of the segment slots, the block and line records
//           mark     per vertex: its line (binary search in the line table); the two ends of an open line are kept; per ring
//                    the smallest key (Y << 32 | X)
//           far      per ring vertex: the squared distance from seed 1, a 64-bit atomic max per ring; the smallest position that
//                    carries the smallest key is seed 1
//           tie      per ring vertex at that distance: atomic min of its key
//           pos      per ring vertex at that distance with that key: atomic min of its position, which is seed 2
//           seed     per ring vertex: the positions of seed 1 and seed 2 are kept
//   round   carry    one work-group: for every block of 256 positions the last kept position before it and the first after it
//           cross    per vertex: previous / next kept position (block scan + carry; a wrap takes the ring's last / first kept
//                    position), |cross| against that chord; vertices beyond the tolerance are candidates and take part in a
//                    64-bit atomic max on the slot of their segment (= the position of its first end); the slots of the
//                    OTHER parity are reset for the next round
//           tie      per candidate that equals the maximum: atomic min of its key on the segment's second slot
//           pos      per candidate that equals both: atomic min of its position on the segment's third slot
//           keep     the candidate at that position is kept; the round's counter is raised
//   finish  count    kept positions per block of 256
//           scan     one work-group: exclusive prefix sum of the block counts; the header record
//           scatter  per kept position: vertex and input index to their compacted place; the prefix of every position
//           lines    per line: the record with start and count, sums and box cleared
//           reduce   per compacted vertex: shoelace term, box (folded over the runs of a wave before the atomics)
//           close    per line: half-open box, the collapsed flag
//
// 6 + 5 per round + 6 launches. A candidate is a vertex that passes the threshold ITSELF: within one segment the chord is fixed,
// so the maximum of |cross| passes iff any vertex does, and then it is the maximum over the candidates; vertices within the
// tolerance issue no atomic and late rounds are almost free. A round whose predecessor kept nothing returns at once.
// Exactness: coordinates in 0 .. 2^30, so differences stay within +-2^30, each product within 2^60, |cross| (twice the area of a
// triangle inside the square) <= 2^60 and d^2 <= 2^61: both fit 64 bits, and the per-segment maximum needs no square. Only the
// keep test does: cross^2 <= 2^120 against eps2 |b - a|^2 <= 2^36 * 2^61, compared as unsigned 128-bit integers. The shoelace sum
// is added modulo 2^64 (unsigned), which is exact wherever the true area2 fits an int64. No work-group waits on another:
// everything a kernel reads was written by an earlier launch; within a launch work-groups meet only in relaxed agent-scope
// integer atomics (max, min, add), whose arrival order changes nothing. No float anywhere.
#include "scene_common.h"
#include "block_scan.h"
#include <limits.h>

#define CS_THREADS 256
#define CS_WAVES (CS_THREADS / INSAR_WAVE)
#define CS_MAX_ROUNDS 4095
#define CS_COUNTERS 4096
#define CS_MAX_VERTICES (1 << 28)
#define CS_MAX_LINES (1 << 27)
#define CS_MAX_EPS 262144ll                // round(1024 * 256)

static_assert(sizeof(InsarContourLine) == 48, "InsarContourLine is three 16-byte stores");

#define CS_ADD(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CS_MIN(p, v) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CS_MAX(p, v) __hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

typedef unsigned long long cs_u64;
typedef unsigned __int128 cs_u128;

// the sections of the scratch buffer; vm is the capacity the parities of the segment slots are spaced by
struct CsBuf {
  int* changed;              // [CS_COUNTERS] vertices kept per round; slot max_rounds is the probe
  uint8_t* keep;             // [vm]
  int* lineof;               // [vm]
  int* seg;                  // [vm] candidate: position of the first end of its segment, else -1
  cs_u64* dev;               // [vm] candidate: |cross| (or the squared distance from a degenerate chord)
  cs_u64* segmax;            // [2][vm]
  cs_u64* segkey;            // [2][vm]
  int* segpos;               // [2][vm]
  int* pos;                  // [vm + 1] kept positions before this one
  int *bmax, *bmin;          // [blocks] last / first kept position of the block, -1 / INT_MAX
  int *cmax, *cmin;          // [blocks] last kept position before the block, first after it
  int* bsum;                 // [blocks]
  cs_u64 *s1key, *s2d2, *s2key;   // [lines] rings: smallest key; largest d^2 from it, the smallest key at that distance
  int *s1pos, *s2pos;        // [lines] rings: the positions of the two seeds
  int *firstk, *lastk;       // [lines] first / last kept position of the line, INT_MAX / -1
  int vm;
};

__device__ __forceinline__ cs_u64 cs_key(int y, int x) { return ((cs_u64)(unsigned int)y << 32) | (cs_u64)(unsigned int)x; }

// the squared distance of (y, x) from the point a key holds
__device__ __forceinline__ cs_u64 cs_dist2(int y, int x, cs_u64 key) {
  const long long dy = (long long)y - (long long)(int)(key >> 32), dx = (long long)x - (long long)(int)(key & 0xffffffffull);
  return (cs_u64)(dy * dy + dx * dx);
}

// position i of line r becomes a kept vertex
__device__ __forceinline__ void cs_note_kept(const CsBuf& b, int i, int r) {
  CS_MIN(&b.firstk[r], i);
  CS_MAX(&b.lastk[r], i);
  CS_MAX(&b.bmax[i / CS_THREADS], i);
  CS_MIN(&b.bmin[i / CS_THREADS], i);
}

// ---------------------------------------------------------------------------------------------
// setup: clear / mark / far / tie / pos / seed
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CS_THREADS)
csimplify_clear_kernel(CsBuf b, int nv, int nl, int nblk) {
  const int n = max(max(nv, nl), max(nblk, CS_COUNTERS));
  for (int i = blockIdx.x * CS_THREADS + threadIdx.x; i < n; i += gridDim.x * CS_THREADS) {
    if (i < CS_COUNTERS) b.changed[i] = 0;
    if (i < nv) {
      b.segmax[i] = 0ull;
      b.segmax[(int64_t)b.vm + i] = 0ull;
      b.segkey[i] = ~0ull;
      b.segkey[(int64_t)b.vm + i] = ~0ull;
      b.segpos[i] = INT_MAX;
      b.segpos[(int64_t)b.vm + i] = INT_MAX;
    }
    if (i < nblk) {
      b.bmax[i] = -1;
      b.bmin[i] = INT_MAX;
    }
    if (i < nl) {
      b.s1key[i] = ~0ull;
      b.s2d2[i] = 0ull;
      b.s2key[i] = ~0ull;
      b.s1pos[i] = INT_MAX;
      b.s2pos[i] = INT_MAX;
      b.firstk[i] = INT_MAX;
      b.lastk[i] = -1;
    }
  }
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_mark_kernel(CsBuf b, const int* __restrict__ verts, int nv, const InsarContourLine* __restrict__ lines, int nl) {
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  int ring = -1;
  cs_u64 key = ~0ull;
  if (i < nv) {
    int lo = 0, hi = nl - 1;                                     // the last line whose start is <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (lines[mid].start <= i) lo = mid;
      else hi = mid - 1;
    }
    const int s = lines[lo].start, e = s + lines[lo].count;
    const bool closed = lines[lo].closed != 0;
    const bool end = !closed && (i == s || i == e - 1);
    b.lineof[i] = lo;
    b.keep[i] = (uint8_t)end;
    if (end) cs_note_kept(b, i, lo);
    if (closed) {
      ring = lo;
      key = cs_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
    }
  }
  const WaveRuns runs = wave_runs(ring);
  const cs_u64 mn = wave_run_reduce(runs, key, WaveMin());
  if (runs.head && ring >= 0) CS_MIN(&b.s1key[ring], mn);
}

// the ring of position i, or -1 (an open line, or past the end); its key
__device__ __forceinline__ int cs_ring_of(const CsBuf& b, const int* verts, int nv, const InsarContourLine* lines, int i, cs_u64* key) {
  if (i >= nv) return -1;
  const int r = b.lineof[i];
  if (lines[r].closed == 0) return -1;
  *key = cs_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
  return r;
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_far_kernel(CsBuf b, const int* __restrict__ verts, int nv, const InsarContourLine* __restrict__ lines) {
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  cs_u64 key = 0ull, d2 = 0ull;
  int first = INT_MAX;
  const int r = cs_ring_of(b, verts, nv, lines, i, &key);
  if (r >= 0) {
    const cs_u64 s1 = b.s1key[r];
    d2 = cs_dist2((int)(key >> 32), (int)(key & 0xffffffffull), s1);
    if (key == s1) first = i;
  }
  const WaveRuns runs = wave_runs(r);
  const cs_u64 mx = wave_run_reduce(runs, d2, WaveMax());
  const int mn = wave_run_reduce(runs, first, WaveMin());
  if (runs.head && r >= 0) {
    CS_MAX(&b.s2d2[r], mx);
    if (mn != INT_MAX) CS_MIN(&b.s1pos[r], mn);
  }
}

// with_key = 0: the smallest key among the ring's vertices at the largest distance; 1: the smallest position among those
__global__ void __launch_bounds__(CS_THREADS)
csimplify_far_tie_kernel(CsBuf b, const int* __restrict__ verts, int nv, const InsarContourLine* __restrict__ lines, int with_key) {
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  cs_u64 key = 0ull;
  int r = cs_ring_of(b, verts, nv, lines, i, &key);
  if (r >= 0) {
    const bool far = cs_dist2((int)(key >> 32), (int)(key & 0xffffffffull), b.s1key[r]) == b.s2d2[r];
    if (!far || (with_key && key != b.s2key[r])) r = -1;
  }
  const WaveRuns runs = wave_runs(r);
  if (with_key) {
    const int mn = wave_run_reduce(runs, i, WaveMin());
    if (runs.head && r >= 0) CS_MIN(&b.s2pos[r], mn);
  } else {
    const cs_u64 mn = wave_run_reduce(runs, key, WaveMin());
    if (runs.head && r >= 0) CS_MIN(&b.s2key[r], mn);
  }
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_seed_kernel(CsBuf b, int nv, const InsarContourLine* __restrict__ lines) {
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  if (i >= nv) return;
  const int r = b.lineof[i];
  if (lines[r].closed == 0) return;
  if (i == b.s1pos[r] || i == b.s2pos[r]) {
    b.keep[i] = 1;
    cs_note_kept(b, i, r);
  }
}

// ---------------------------------------------------------------------------------------------
// one round: carry / cross / tie / pos / keep
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CS_THREADS)
csimplify_carry_kernel(CsBuf b, int nblk, int rd) {
  __shared__ int w[CS_WAVES];
  if (rd > 0 && b.changed[rd - 1] == 0) return;
  block_carry<CS_THREADS>(b.bmax, b.bmin, b.cmax, b.cmin, nblk, w);
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_cross_kernel(CsBuf b, const int* __restrict__ verts, int nv, const InsarContourLine* __restrict__ lines, long long eps2, int rd) {
  __shared__ int w[CS_WAVES];
  if (rd > 0 && b.changed[rd - 1] == 0) return;
  const int par = rd & 1;
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  const bool live = i < nv;
  const bool kept = live && b.keep[i];
  int total;
  int p = block_prefix_max<CS_THREADS>(kept ? i : -1, w, &total);
  int q = block_suffix_min<CS_THREADS>(kept ? i : INT_MAX, w, &total);
  const int cp = b.cmax[blockIdx.x], cq = b.cmin[blockIdx.x];
  p = cp > p ? cp : p;
  q = cq < q ? cq : q;
  int sg = -1;
  cs_u64 num = 0ull;
  if (live) {
    const int64_t other = (int64_t)(par ^ 1) * b.vm + i;         // nobody reads the other parity during this round
    b.segmax[other] = 0ull;
    b.segkey[other] = ~0ull;
    b.segpos[other] = INT_MAX;
    if (!kept) {
      const int r = b.lineof[i];
      const int s = lines[r].start, e = s + lines[r].count;
      if (p < s) p = b.lastk[r];                                 // rings only: an open line keeps both of its ends
      if (q >= e) q = b.firstk[r];
      if (p >= 0 && p < nv && q >= 0 && q < nv) {                // always, for a line table that matches the vertex array
        const int ay = verts[2 * (int64_t)p], ax = verts[2 * (int64_t)p + 1];
        const int by = verts[2 * (int64_t)q], bx = verts[2 * (int64_t)q + 1];
        const long long py = (long long)verts[2 * (int64_t)i] - ay, px = (long long)verts[2 * (int64_t)i + 1] - ax;
        const long long dy = (long long)by - ay, dx = (long long)bx - ax;
        const cs_u64 len2 = (cs_u64)(dy * dy + dx * dx);
        cs_u64 n;
        bool beyond;
        if (len2) {
          const long long cr = dx * py - dy * px;
          n = (cs_u64)(cr < 0 ? -cr : cr);
          beyond = (cs_u128)n * n > (cs_u128)(cs_u64)eps2 * len2;
        } else {                                                 // a chord whose ends coincide: the distance from that point
          n = (cs_u64)(py * py + px * px);
          beyond = n > (cs_u64)eps2;
        }
        if (beyond) {
          sg = p;
          num = n;
        }
      }
    }
    b.seg[i] = sg;
    b.dev[i] = num;
  }
  const WaveRuns runs = wave_runs(sg);
  const cs_u64 mx = wave_run_reduce(runs, num, WaveMax());
  if (runs.head && sg >= 0) CS_MAX(&b.segmax[(int64_t)par * b.vm + sg], mx);
}

// with_key = 0: the smallest key among the candidates that equal their segment's maximum; 1: the smallest position among those
__global__ void __launch_bounds__(CS_THREADS)
csimplify_tie_kernel(CsBuf b, const int* __restrict__ verts, int nv, int rd, int with_key) {
  if (rd > 0 && b.changed[rd - 1] == 0) return;
  const int par = rd & 1;
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  int sg = i < nv ? b.seg[i] : -1;
  cs_u64 key = ~0ull;
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
    if (runs.head && sg >= 0) CS_MIN(&b.segpos[(int64_t)par * b.vm + sg], mn);
  } else {
    const cs_u64 mn = wave_run_reduce(runs, key, WaveMin());
    if (runs.head && sg >= 0) CS_MIN(&b.segkey[(int64_t)par * b.vm + sg], mn);
  }
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_keep_kernel(CsBuf b, int nv, int rd, int apply) {
  if (rd > 0 && b.changed[rd - 1] == 0) return;
  const int par = rd & 1;
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  const int sg = i < nv ? b.seg[i] : -1;
  const bool win = sg >= 0 && b.segpos[(int64_t)par * b.vm + sg] == i;
  if (win && apply) {
    b.keep[i] = 1;
    cs_note_kept(b, i, b.lineof[i]);
  }
  const int n = __popcll(__ballot(win));
  if ((int)__lane_id() == 0 && n) CS_ADD(&b.changed[rd], n);
}

// ---------------------------------------------------------------------------------------------
// finish: count / scan / scatter / lines / reduce / close
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CS_THREADS)
csimplify_count_kernel(CsBuf b, int nv) {
  __shared__ int w[CS_WAVES];
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  int total;
  block_prefix_sum<CS_THREADS>(i < nv ? (int)b.keep[i] : 0, w, &total);
  if (threadIdx.x == 0) b.bsum[blockIdx.x] = total;
}

// One work-group: bsum becomes its exclusive prefix sum; the header: level = n_lines, leader = rounds, start = converged,
// count = kept vertices, closed = input vertices.
__global__ void __launch_bounds__(CS_THREADS)
csimplify_scan_kernel(CsBuf b, int nblk, int nv, int nl, int max_rounds, InsarContourLine* __restrict__ table) {
  __shared__ int w[CS_WAVES];
  __shared__ int rounds;
  if (threadIdx.x == 0) rounds = 0;
  const int carry = block_scan_array<CS_THREADS>(b.bsum, nblk, w);
  int mine = 0;
  for (int r = threadIdx.x; r < max_rounds; r += CS_THREADS) mine += b.changed[r] != 0;
  if (mine) atomicAdd(&rounds, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    InsarContourLine h;
    h.area2 = 0;
    h.level = nl;
    h.leader = rounds;
    h.start = b.changed[max_rounds] == 0;
    h.count = carry;
    h.closed = nv;
    h.y0 = h.x0 = h.y1 = h.x1 = h._pad = 0;
    table[0] = h;
  }
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_scatter_kernel(CsBuf b, const int* __restrict__ verts, int nv, int* __restrict__ out_verts, int* __restrict__ out_kept) {
  __shared__ int w[CS_WAVES];
  const int i = blockIdx.x * CS_THREADS + threadIdx.x;
  const int k = i < nv ? (int)b.keep[i] : 0;
  int total;
  const int at = b.bsum[blockIdx.x] + block_prefix_sum<CS_THREADS>(k, w, &total);
  if (i >= nv) return;
  b.pos[i] = at;
  if (i == nv - 1) b.pos[nv] = at + k;
  if (k) {
    *reinterpret_cast<int2*>(out_verts + 2 * (int64_t)at) = make_int2(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
    out_kept[at] = i;
  }
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_lines_kernel(CsBuf b, const InsarContourLine* __restrict__ lines, int nl, int nv, InsarContourLine* __restrict__ table) {
  const int r = blockIdx.x * CS_THREADS + threadIdx.x;
  if (r >= nl) return;
  InsarContourLine o = lines[r];
  const int s = min(max(o.start, 0), nv), e = min(max(s + o.count, s), nv);     // no clamp bites on a table that matches the array
  o.area2 = 0;
  o.start = b.pos[s];
  o.count = b.pos[e] - o.start;
  o.closed = o.closed != 0;
  o.y0 = o.x0 = INT_MAX;
  o.y1 = o.x1 = INT_MIN;
  o._pad = 0;
  table[1 + r] = o;
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_reduce_kernel(CsBuf b, const int* __restrict__ out_verts, const int* __restrict__ out_kept, int nv, InsarContourLine* __restrict__ table) {
  const int j = blockIdx.x * CS_THREADS + threadIdx.x;
  const int kept = min(table[0].count, nv);
  int r = -1, y = 0, x = 0;
  cs_u64 term = 0ull;
  if (j < kept) {
    const int at = out_kept[j];
    r = b.lineof[min(max(at, 0), nv - 1)];
    const InsarContourLine* o = table + 1 + r;
    y = out_verts[2 * (int64_t)j];
    x = out_verts[2 * (int64_t)j + 1];
    if (o->closed) {
      int nx = j + 1 < o->start + o->count ? j + 1 : o->start;
      if (nx < 0 || nx >= kept) nx = j;                          // never, for a table that matches the array
      const int yn = out_verts[2 * (int64_t)nx], xn = out_verts[2 * (int64_t)nx + 1];
      term = (cs_u64)((long long)x * yn) - (cs_u64)((long long)xn * y);
    }
  }
  const WaveRuns runs = wave_runs(r);
  const cs_u64 sum = wave_run_reduce(runs, term, WaveAdd());
  const int y0 = wave_run_reduce(runs, y, WaveMin()), x0 = wave_run_reduce(runs, x, WaveMin());
  const int y1 = wave_run_reduce(runs, y, WaveMax()), x1 = wave_run_reduce(runs, x, WaveMax());
  if (runs.head && r >= 0) {
    InsarContourLine* o = table + 1 + r;
    if (sum) CS_ADD(reinterpret_cast<cs_u64*>(&o->area2), sum);
    CS_MIN(&o->y0, y0);
    CS_MIN(&o->x0, x0);
    CS_MAX(&o->y1, y1);
    CS_MAX(&o->x1, x1);
  }
}

__global__ void __launch_bounds__(CS_THREADS)
csimplify_close_kernel(int nl, InsarContourLine* __restrict__ table) {
  const int r = blockIdx.x * CS_THREADS + threadIdx.x;
  if (r >= nl) return;
  InsarContourLine* o = table + 1 + r;
  o->y1 += 1;
  o->x1 += 1;
  o->_pad = o->closed && (o->count < 3 || o->area2 == 0);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#define CS_SECTIONS 21
struct CsLayout { int64_t off[CS_SECTIONS]; int64_t bytes, table_bytes; };

static int csimplify_layout(const char* who, int32_t max_vertices, int32_t max_lines, CsLayout* l) {
  if (max_vertices < 1 || max_vertices > CS_MAX_VERTICES)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_vertices %d outside 1..%d", who, max_vertices, CS_MAX_VERTICES);
  if (max_lines < 1 || max_lines > CS_MAX_LINES) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_lines %d outside 1..%d", who, max_lines, CS_MAX_LINES);
  const int64_t vm = max_vertices, lm = max_lines, nb = (vm + CS_THREADS - 1) / CS_THREADS;
  // the order of CsBuf: changed keep lineof seg dev segmax segkey segpos pos bmax bmin cmax cmin bsum s1key s2d2 s2key s1pos s2pos
  // firstk lastk
  const int64_t size[CS_SECTIONS] = {4 * CS_COUNTERS, vm, 4 * vm, 4 * vm, 8 * vm, 16 * vm, 16 * vm, 8 * vm, 4 * (vm + 1), 4 * nb, 4 * nb,
                                     4 * nb, 4 * nb, 4 * nb, 8 * lm, 8 * lm, 8 * lm, 4 * lm, 4 * lm, 4 * lm, 4 * lm};
  int64_t at = 0;
  for (int k = 0; k < CS_SECTIONS; ++k) {
    l->off[k] = at;
    at += (size[k] + 15) & ~(int64_t)15;
  }
  l->bytes = at;
  l->table_bytes = (int64_t)sizeof(InsarContourLine) * (1 + lm);
  return INSAR_OK;
}

static CsBuf csimplify_buf(const CsLayout& l, void* scratch, int32_t max_vertices) {
  char* s = (char*)scratch;
  CsBuf b;
  b.changed = (int*)(s + l.off[0]);
  b.keep = (uint8_t*)(s + l.off[1]);
  b.lineof = (int*)(s + l.off[2]);
  b.seg = (int*)(s + l.off[3]);
  b.dev = (cs_u64*)(s + l.off[4]);
  b.segmax = (cs_u64*)(s + l.off[5]);
  b.segkey = (cs_u64*)(s + l.off[6]);
  b.segpos = (int*)(s + l.off[7]);
  b.pos = (int*)(s + l.off[8]);
  b.bmax = (int*)(s + l.off[9]);
  b.bmin = (int*)(s + l.off[10]);
  b.cmax = (int*)(s + l.off[11]);
  b.cmin = (int*)(s + l.off[12]);
  b.bsum = (int*)(s + l.off[13]);
  b.s1key = (cs_u64*)(s + l.off[14]);
  b.s2d2 = (cs_u64*)(s + l.off[15]);
  b.s2key = (cs_u64*)(s + l.off[16]);
  b.s1pos = (int*)(s + l.off[17]);
  b.s2pos = (int*)(s + l.off[18]);
  b.firstk = (int*)(s + l.off[19]);
  b.lastk = (int*)(s + l.off[20]);
  b.vm = max_vertices;
  return b;
}

// what setup, rounds and finish share: the vertex array, the input line table, the counts against the capacities, the scratch
static int csimplify_check(const char* who, const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines,
                           int32_t max_vertices, int32_t max_lines, const void* scratch, CsLayout* l) {
  if (int rc = csimplify_layout(who, max_vertices, max_lines, l)) return rc;
  if (!vertices || !lines || !scratch)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !vertices ? "vertices" : !lines ? "lines" : "scratch");
  if (n_vertices < 1 || n_vertices > max_vertices) INSAR_FAIL(INSAR_E_SHAPE, "%s: n_vertices %d outside 1..max_vertices = %d", who, n_vertices, max_vertices);
  if (n_lines < 1 || n_lines > max_lines) INSAR_FAIL(INSAR_E_SHAPE, "%s: n_lines %d outside 1..max_lines = %d", who, n_lines, max_lines);
  if ((int64_t)2 * n_lines > (int64_t)n_vertices) INSAR_FAIL(INSAR_E_SHAPE, "%s: %d lines over %d vertices", who, n_lines, n_vertices);
  if (((uintptr_t)vertices) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: vertices not 8-byte aligned", who);
  if (!insar_aligned16(lines) || !insar_aligned16(scratch)) INSAR_FAIL(INSAR_E_ALIGN, "%s: lines / scratch not 16-byte aligned", who);
  return INSAR_OK;
}

static int csimplify_check_rounds(const char* who, int32_t max_rounds) {
  if (max_rounds < 1 || max_rounds > CS_MAX_ROUNDS) INSAR_FAIL(INSAR_E_ARG, "%s: max_rounds %d outside 1..%d", who, max_rounds, CS_MAX_ROUNDS);
  return INSAR_OK;
}

extern "C" int insar_contour_simplify_scratch_bytes(int32_t max_vertices, int32_t max_lines, int64_t* scratch_bytes, int64_t* table_bytes) {
  const char* who = "insar_contour_simplify_scratch_bytes";
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  CsLayout l;
  if (int rc = csimplify_layout(who, max_vertices, max_lines, &l)) return rc;
  *scratch_bytes = l.bytes;
  *table_bytes = l.table_bytes;
  return INSAR_OK;
}

extern "C" int insar_contour_simplify_launches(int32_t rounds) {
  return 12 + 5 * (rounds < 0 ? 0 : rounds > CS_MAX_ROUNDS + 1 ? CS_MAX_ROUNDS + 1 : rounds);
}

extern "C" int insar_contour_simplify_setup(const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines,
                                            int32_t max_vertices, int32_t max_lines, void* scratch, void* stream) {
  const char* who = "insar_contour_simplify_setup";
  CsLayout l;
  if (int rc = csimplify_check(who, vertices, n_vertices, lines, n_lines, max_vertices, max_lines, scratch, &l)) return rc;
  const CsBuf b = csimplify_buf(l, scratch, max_vertices);
  const int nblk = (n_vertices + CS_THREADS - 1) / CS_THREADS;
  const InsarContourLine* lin = (const InsarContourLine*)lines + 1;
  const int* v = (const int*)vertices;
  const int nv = n_vertices;
  const dim3 grid(nblk), block(CS_THREADS);
  hipStream_t s = (hipStream_t)stream;
  const int nclear = n_vertices > CS_COUNTERS ? n_vertices : CS_COUNTERS;
  hipLaunchKernelGGL(csimplify_clear_kernel, dim3(insar_grid_cap((nclear + CS_THREADS - 1) / CS_THREADS)), block, 0, s, b, nv, (int)n_lines, nblk);
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
  CsLayout l;
  if (int rc = csimplify_check(who, vertices, n_vertices, lines, n_lines, max_vertices, max_lines, scratch, &l)) return rc;
  if (eps2 < 0 || eps2 > CS_MAX_EPS * CS_MAX_EPS)
    INSAR_FAIL(INSAR_E_ARG, "%s: eps2 %lld outside 0..%lld", who, (long long)eps2, CS_MAX_EPS * CS_MAX_EPS);
  if (int rc = csimplify_check_rounds(who, max_rounds)) return rc;
  if (first_round < 0 || n_rounds < 1 || (int64_t)first_round + n_rounds > (int64_t)max_rounds + 1)
    INSAR_FAIL(INSAR_E_ARG, "%s: rounds %d..%d+%d outside 0..max_rounds = %d (the last one is the probe)", who, first_round, first_round,
               n_rounds, max_rounds);
  const CsBuf b = csimplify_buf(l, scratch, max_vertices);
  const int nblk = (n_vertices + CS_THREADS - 1) / CS_THREADS;
  const InsarContourLine* lin = (const InsarContourLine*)lines + 1;
  const int* v = (const int*)vertices;
  const int nv = n_vertices;
  const dim3 grid(nblk), block(CS_THREADS);
  hipStream_t s = (hipStream_t)stream;
  for (int rd = first_round; rd < first_round + n_rounds; ++rd) {
    hipLaunchKernelGGL(csimplify_carry_kernel, dim3(1), block, 0, s, b, nblk, rd);
    hipLaunchKernelGGL(csimplify_cross_kernel, grid, block, 0, s, b, v, nv, lin, (long long)eps2, rd);
    hipLaunchKernelGGL(csimplify_tie_kernel, grid, block, 0, s, b, v, nv, rd, 0);
    hipLaunchKernelGGL(csimplify_tie_kernel, grid, block, 0, s, b, v, nv, rd, 1);
    hipLaunchKernelGGL(csimplify_keep_kernel, grid, block, 0, s, b, nv, rd, (int)(rd < max_rounds));
  }
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_contour_simplify_finish(const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines,
                                             int32_t max_rounds, int32_t max_vertices, int32_t max_lines, void* scratch, void* table,
                                             int32_t* out_vertices, int32_t* out_kept, void* stream) {
  const char* who = "insar_contour_simplify_finish";
  CsLayout l;
  if (int rc = csimplify_check(who, vertices, n_vertices, lines, n_lines, max_vertices, max_lines, scratch, &l)) return rc;
  if (int rc = csimplify_check_rounds(who, max_rounds)) return rc;
  if (!table || !out_vertices || !out_kept)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !table ? "table" : !out_vertices ? "out_vertices" : "out_kept");
  if (!insar_aligned16(table)) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 16-byte aligned", who);
  if ((((uintptr_t)out_vertices) & 7u) || (((uintptr_t)out_kept) & 3u))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: out_vertices not 8-byte or out_kept not 4-byte aligned", who);
  const CsBuf b = csimplify_buf(l, scratch, max_vertices);
  const int nblk = (n_vertices + CS_THREADS - 1) / CS_THREADS;
  const InsarContourLine* lin = (const InsarContourLine*)lines + 1;
  InsarContourLine* t = (InsarContourLine*)table;
  const int nv = n_vertices;
  const dim3 grid(nblk), lgrid((n_lines + CS_THREADS - 1) / CS_THREADS), block(CS_THREADS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(csimplify_count_kernel, grid, block, 0, s, b, nv);
  hipLaunchKernelGGL(csimplify_scan_kernel, dim3(1), block, 0, s, b, nblk, nv, (int)n_lines, (int)max_rounds, t);
  hipLaunchKernelGGL(csimplify_scatter_kernel, grid, block, 0, s, b, (const int*)vertices, nv, (int*)out_vertices, (int*)out_kept);
  hipLaunchKernelGGL(csimplify_lines_kernel, lgrid, block, 0, s, b, lin, (int)n_lines, nv, t);
  hipLaunchKernelGGL(csimplify_reduce_kernel, grid, block, 0, s, b, (const int*)out_vertices, (const int*)out_kept, nv, t);
  hipLaunchKernelGGL(csimplify_close_kernel, lgrid, block, 0, s, (int)n_lines, t);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
