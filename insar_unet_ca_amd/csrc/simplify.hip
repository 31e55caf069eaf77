// Outline simplification: Douglas-Peucker over the rings of the region outlines (outline.hip), in exact integers and aware of
// shared borders. Semantics: include/insar_hip.h, "outline simplification". Every array below is indexed by the POSITION of a
// vertex in the input vertex array (ring after ring); rings are not rotated: a segment that wraps over the end of its ring
// takes its ends from the ring's first / last kept position.
//
//   setup   clear    counters, both parities of the segment slots, the block and ring records
//           mark     per vertex: its ring (binary search in the ring table), the anchor flag from four label reads; per ring
//                    the anchor count, the anchor's key and the smallest key (y << 16 | x)
//           far      per vertex of a ring with fewer than two anchors: squared distance from seed 1, a 64-bit atomic max of
//                    (d2 << 32 | 2^31 - 1 - key) per ring: the farthest vertex, ties to the smallest key
//           seed     per vertex: every position that carries the coordinates of seed 1 or seed 2 is kept
//   round   carry    one work-group: for every block of 256 positions the last kept position before it and the first after it
//           cross    per vertex: previous / next kept position (block scan + carry; a wrap takes the ring's last / first kept
//                    position), cross^2 against that chord; vertices beyond the tolerance are candidates and take part in a
//                    64-bit atomic max on the slot of their segment (= the position of its first end); the slots of the
//                    OTHER parity are reset for the next round
//           tie      per candidate that equals the maximum: atomic min of its key on the segment's second slot
//           keep     per candidate that equals both: kept; the round's counter is raised
//   finish  count    kept positions per block of 256
//           scan     one work-group: exclusive prefix sum of the block counts; the header record
//           scatter  per kept position: vertex and input index to their compacted place; the prefix of every position
//           rings    per ring: the record with start and count, sums and box cleared
//           reduce   per compacted vertex: shoelace term, box (folded over the runs of a wave before the atomics)
//           close    per ring: half-open box, the collapsed flag
//
// 4 + 4 per round + 6 launches. A candidate is a vertex that passes the threshold ITSELF: the maximum of a segment passes iff
// any of its vertices does, and then it is the maximum over the candidates, so vertices within the tolerance issue no atomic
// and late rounds are almost free. A round whose predecessor kept nothing returns at once (every kernel reads the
// predecessor's counter first). The kept set only grows; the first / last kept position of every block and ring is kept up to
// date by the atomics of the thread that keeps a vertex, so no round re-derives them.
// Exactness: coordinates <= 2^14, so |cross| < 2^30 and cross^2 < 2^60 fit 64 bits; 256 cross^2 > eps2q |b - a|^2 is tested as
// cross^2 > floor(eps2q |b - a|^2 / 256), the same for integers, with eps2q |b - a|^2 < 2^58. No work-group waits on another:
// everything a kernel reads was written by an earlier launch; within a launch work-groups meet only in relaxed agent-scope
// integer atomics (max, min, add), whose arrival order changes nothing. No float anywhere.
#include "scene_common.h"
#include "block_scan.h"
#include <limits.h>

#define SM_THREADS 256
#define SM_WAVES (SM_THREADS / INSAR_WAVE)
#define SM_MAX_ROUNDS 4095
#define SM_COUNTERS 4096
#define SM_MAX_VERTICES (1 << 28)
#define SM_MAX_RINGS (1 << 26)
#define SM_MAX_DIM 16384
#define SM_MAX_EPSQ 16384ll                // round(1024 * 16)

static_assert(sizeof(InsarRing) == 48, "InsarRing is three 16-byte stores");

#define SM_ADD(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SM_MIN(p, v) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SM_MAX(p, v) __hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

typedef unsigned long long sm_u64;

// the sections of the scratch buffer; vm is the capacity the parities of the segment slots are spaced by
struct SmBuf {
  int* changed;              // [SM_COUNTERS] vertices kept per round; slot max_rounds is the probe
  uint8_t* keep;             // [vm]
  int* ringof;               // [vm]
  int* seg;                  // [vm] candidate: position of the first end of its segment, else -1
  sm_u64* c2;                // [vm] candidate: cross^2 (or the squared distance from a degenerate chord)
  sm_u64* segmax;            // [2][vm]
  unsigned int* segmin;      // [2][vm]
  int* pos;                  // [vm + 1] kept positions before this one
  int *bmax, *bmin;          // [blocks] last / first kept position of the block, -1 / INT_MAX
  int *cmax, *cmin;          // [blocks] last kept position before the block, first after it
  int* bsum;                 // [blocks]
  int* nanch;                // [rings]
  unsigned int *akey, *s1key;
  sm_u64* s2key;
  int *firstk, *lastk;       // [rings] first / last kept position of the ring, INT_MAX / -1
  int vm;
};

__device__ __forceinline__ unsigned int sm_key(int y, int x) { return ((unsigned int)y << 16) | (unsigned int)x; }

// position i of ring r becomes a kept vertex
__device__ __forceinline__ void sm_note_kept(const SmBuf& b, int i, int r) {
  SM_MIN(&b.firstk[r], i);
  SM_MAX(&b.lastk[r], i);
  SM_MAX(&b.bmax[i / SM_THREADS], i);
  SM_MIN(&b.bmin[i / SM_THREADS], i);
}

// ---------------------------------------------------------------------------------------------
// setup: clear / mark / far / seed
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SM_THREADS)
simplify_clear_kernel(SmBuf b, int nv, int nr, int nblk) {
  const int n = max(max(nv, nr), max(nblk, SM_COUNTERS));
  for (int i = blockIdx.x * SM_THREADS + threadIdx.x; i < n; i += gridDim.x * SM_THREADS) {
    if (i < SM_COUNTERS) b.changed[i] = 0;
    if (i < nv) {
      b.segmax[i] = 0ull;
      b.segmax[(int64_t)b.vm + i] = 0ull;
      b.segmin[i] = ~0u;
      b.segmin[(int64_t)b.vm + i] = ~0u;
    }
    if (i < nblk) {
      b.bmax[i] = -1;
      b.bmin[i] = INT_MAX;
    }
    if (i < nr) {
      b.nanch[i] = 0;
      b.akey[i] = ~0u;
      b.s1key[i] = ~0u;
      b.s2key[i] = 0ull;
      b.firstk[i] = INT_MAX;
      b.lastk[i] = -1;
    }
  }
}

__device__ __forceinline__ int sm_label(const int* labels, int H, int W, int y, int x) {
  return (y >= 0 && y < H && x >= 0 && x < W) ? labels[(int64_t)y * W + x] : 0;
}
// three or more distinct values among the four pixels of vertex (y, x), or a two-label saddle without background
__device__ __forceinline__ bool sm_anchor(const int* labels, int H, int W, int y, int x) {
  const int p00 = sm_label(labels, H, W, y - 1, x - 1), p01 = sm_label(labels, H, W, y - 1, x);
  const int p10 = sm_label(labels, H, W, y, x - 1), p11 = sm_label(labels, H, W, y, x);
  const int distinct = 1 + (p01 != p00) + (p10 != p00 && p10 != p01) + (p11 != p00 && p11 != p01 && p11 != p10);
  return distinct >= 3 || (p00 == p11 && p01 == p10 && p00 != p01 && p00 != 0 && p01 != 0);
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_mark_kernel(SmBuf b, const int* __restrict__ verts, int nv, const InsarRing* __restrict__ rings, int nr,
                     const int* __restrict__ labels, int H, int W) {
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  const bool live = i < nv;
  int r = -1, anchor = 0;
  unsigned int key = ~0u;
  if (live) {
    int lo = 0, hi = nr - 1;                                     // the last ring whose start is <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (rings[mid].start <= i) lo = mid;
      else hi = mid - 1;
    }
    r = lo;
    const int y = verts[2 * (int64_t)i], x = verts[2 * (int64_t)i + 1];
    key = sm_key(y, x);
    anchor = labels ? (int)sm_anchor(labels, H, W, y, x) : 0;
    b.ringof[i] = r;
    b.keep[i] = (uint8_t)anchor;
    if (anchor) sm_note_kept(b, i, r);
  }
  const WaveRuns runs = wave_runs(r);
  const unsigned int mn = wave_run_reduce(runs, key, WaveMin());
  const int na = wave_run_reduce(runs, anchor, WaveAdd());
  const unsigned int ak = wave_run_reduce(runs, anchor ? key : ~0u, WaveMin());
  if (runs.head && r >= 0) {
    SM_MIN(&b.s1key[r], mn);
    if (na) {
      SM_ADD(&b.nanch[r], na);
      SM_MIN(&b.akey[r], ak);
    }
  }
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_far_kernel(SmBuf b, const int* __restrict__ verts, int nv) {
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  int r = -1;
  sm_u64 k = 0ull;
  if (i < nv) {
    const int ring = b.ringof[i];
    const int na = b.nanch[ring];
    if (na < 2) {
      r = ring;
      const unsigned int s1 = na == 1 ? b.akey[ring] : b.s1key[ring];
      const int y = verts[2 * (int64_t)i], x = verts[2 * (int64_t)i + 1];
      const long long dy = y - (int)(s1 >> 16), dx = x - (int)(s1 & 0xffffu);
      k = ((sm_u64)(dy * dy + dx * dx) << 32) | (sm_u64)(0x7fffffffu - sm_key(y, x));
    }
  }
  const WaveRuns runs = wave_runs(r);
  const sm_u64 mx = wave_run_reduce(runs, k, WaveMax());
  if (runs.head && r >= 0) SM_MAX(&b.s2key[r], mx);
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_seed_kernel(SmBuf b, const int* __restrict__ verts, int nv) {
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= nv) return;
  const int r = b.ringof[i];
  const int na = b.nanch[r];
  if (na >= 2 || b.keep[i]) return;
  const unsigned int s1 = na == 1 ? b.akey[r] : b.s1key[r];
  const unsigned int s2 = 0x7fffffffu - (unsigned int)(b.s2key[r] & 0xffffffffull);
  const unsigned int key = sm_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
  if (key == s1 || key == s2) {
    b.keep[i] = 1;
    sm_note_kept(b, i, r);
  }
}

// ---------------------------------------------------------------------------------------------
// one round: carry / cross / tie / keep
// ---------------------------------------------------------------------------------------------
// One work-group: cmax[j] = max of bmax over the blocks before j, cmin[j] = min of bmin over the blocks after j.
__global__ void __launch_bounds__(SM_THREADS)
simplify_carry_kernel(SmBuf b, int nblk, int rd) {
  __shared__ int w[SM_WAVES];
  if (rd > 0 && b.changed[rd - 1] == 0) return;
  block_carry<SM_THREADS>(b.bmax, b.bmin, b.cmax, b.cmin, nblk, w);
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_cross_kernel(SmBuf b, const int* __restrict__ verts, int nv, const InsarRing* __restrict__ rings, long long eps2q, int rd) {
  __shared__ int w[SM_WAVES];
  if (rd > 0 && b.changed[rd - 1] == 0) return;
  const int par = rd & 1;
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  const bool live = i < nv;
  const bool kept = live && b.keep[i];
  int total;
  int p = block_prefix_max<SM_THREADS>(kept ? i : -1, w, &total);
  int q = block_suffix_min<SM_THREADS>(kept ? i : INT_MAX, w, &total);
  const int cp = b.cmax[blockIdx.x], cq = b.cmin[blockIdx.x];
  p = cp > p ? cp : p;
  q = cq < q ? cq : q;
  int sg = -1;
  sm_u64 num = 0ull;
  if (live) {
    const int64_t other = (int64_t)(par ^ 1) * b.vm + i;         // nobody reads the other parity during this round
    b.segmax[other] = 0ull;
    b.segmin[other] = ~0u;
    if (!kept) {
      const int r = b.ringof[i];
      const int s = rings[r].start, e = s + rings[r].count;
      if (p < s) p = b.lastk[r];
      if (q >= e) q = b.firstk[r];
      if (p >= 0 && p < nv && q >= 0 && q < nv) {                // always, for a ring table that matches the vertex array
        const int ay = verts[2 * (int64_t)p], ax = verts[2 * (int64_t)p + 1];
        const int by = verts[2 * (int64_t)q], bx = verts[2 * (int64_t)q + 1];
        const long long py = verts[2 * (int64_t)i] - ay, px = verts[2 * (int64_t)i + 1] - ax;
        const long long dy = by - ay, dx = bx - ax;
        const long long len2 = dy * dy + dx * dx;
        const long long cr = dx * py - dy * px;
        // a chord whose ends coincide: the distance from that point takes the place of the distance from the line
        const sm_u64 n = len2 ? (sm_u64)(cr * cr) : (sm_u64)(py * py + px * px);
        const sm_u64 thr = (sm_u64)(eps2q * (len2 ? len2 : 1ll)) >> 8;
        if (n > thr) {
          sg = p;
          num = n;
        }
      }
    }
    b.seg[i] = sg;
    b.c2[i] = num;
  }
  const WaveRuns runs = wave_runs(sg);
  const sm_u64 mx = wave_run_reduce(runs, num, WaveMax());
  if (runs.head && sg >= 0) SM_MAX(&b.segmax[(int64_t)par * b.vm + sg], mx);
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_tie_kernel(SmBuf b, const int* __restrict__ verts, int nv, int rd) {
  if (rd > 0 && b.changed[rd - 1] == 0) return;
  const int par = rd & 1;
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  int sg = i < nv ? b.seg[i] : -1;
  unsigned int key = ~0u;
  if (sg >= 0) {
    if (b.c2[i] == b.segmax[(int64_t)par * b.vm + sg]) key = sm_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
    else sg = -1;
  }
  const WaveRuns runs = wave_runs(sg);
  const unsigned int mn = wave_run_reduce(runs, key, WaveMin());
  if (runs.head && sg >= 0) SM_MIN(&b.segmin[(int64_t)par * b.vm + sg], mn);
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_keep_kernel(SmBuf b, const int* __restrict__ verts, int nv, int rd, int apply) {
  if (rd > 0 && b.changed[rd - 1] == 0) return;
  const int par = rd & 1;
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  const int sg = i < nv ? b.seg[i] : -1;
  bool win = false;
  if (sg >= 0) {
    const int64_t slot = (int64_t)par * b.vm + sg;
    win = b.c2[i] == b.segmax[slot] && sm_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]) == b.segmin[slot];
  }
  if (win && apply) {
    b.keep[i] = 1;
    sm_note_kept(b, i, b.ringof[i]);
  }
  const int n = __popcll(__ballot(win));
  if ((int)__lane_id() == 0 && n) SM_ADD(&b.changed[rd], n);
}

// ---------------------------------------------------------------------------------------------
// finish: count / scan / scatter / rings / reduce / close
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SM_THREADS)
simplify_count_kernel(SmBuf b, int nv) {
  __shared__ int w[SM_WAVES];
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  int total;
  block_prefix_sum<SM_THREADS>(i < nv ? (int)b.keep[i] : 0, w, &total);
  if (threadIdx.x == 0) b.bsum[blockIdx.x] = total;
}

// One work-group: bsum becomes its exclusive prefix sum; the header: label = R, leader = rounds, start = converged,
// count = kept vertices, edges = input vertices.
__global__ void __launch_bounds__(SM_THREADS)
simplify_scan_kernel(SmBuf b, int nblk, int nv, int nr, int max_rounds, InsarRing* __restrict__ table) {
  __shared__ int w[SM_WAVES];
  __shared__ int rounds;
  if (threadIdx.x == 0) rounds = 0;
  const int carry = block_scan_array<SM_THREADS>(b.bsum, nblk, w);
  int mine = 0;
  for (int r = threadIdx.x; r < max_rounds; r += SM_THREADS) mine += b.changed[r] != 0;
  if (mine) atomicAdd(&rounds, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    InsarRing h;
    h.area2 = 0;
    h.label = nr;
    h.leader = rounds;
    h.start = b.changed[max_rounds] == 0;
    h.count = carry;
    h.edges = nv;
    h.y0 = h.x0 = h.y1 = h.x1 = h._pad = 0;
    table[0] = h;
  }
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_scatter_kernel(SmBuf b, const int* __restrict__ verts, int nv, int* __restrict__ out_verts, int* __restrict__ out_kept) {
  __shared__ int w[SM_WAVES];
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  const int k = i < nv ? (int)b.keep[i] : 0;
  int total;
  const int at = b.bsum[blockIdx.x] + block_prefix_sum<SM_THREADS>(k, w, &total);
  if (i >= nv) return;
  b.pos[i] = at;
  if (i == nv - 1) b.pos[nv] = at + k;
  if (k) {
    *reinterpret_cast<int2*>(out_verts + 2 * (int64_t)at) = make_int2(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]);
    out_kept[at] = i;
  }
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_rings_kernel(SmBuf b, const InsarRing* __restrict__ rings, int nr, int nv, InsarRing* __restrict__ table) {
  const int r = blockIdx.x * SM_THREADS + threadIdx.x;
  if (r >= nr) return;
  InsarRing o = rings[r];
  const int s = min(max(o.start, 0), nv), e = min(max(s + o.count, s), nv);     // no clamp bites on a table that matches the array
  o.area2 = 0;
  o.start = b.pos[s];
  o.count = b.pos[e] - o.start;
  o.y0 = o.x0 = INT_MAX;
  o.y1 = o.x1 = INT_MIN;
  o._pad = 0;
  table[1 + r] = o;
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_reduce_kernel(SmBuf b, const int* __restrict__ out_verts, const int* __restrict__ out_kept, int nv, InsarRing* __restrict__ table) {
  const int j = blockIdx.x * SM_THREADS + threadIdx.x;
  const int kept = min(table[0].count, nv);
  int r = -1, y = 0, x = 0;
  long long term = 0;
  if (j < kept) {
    r = b.ringof[out_kept[j]];
    const InsarRing* o = table + 1 + r;
    int nx = j + 1 < o->start + o->count ? j + 1 : o->start;
    if (nx >= kept) nx = j;                                      // never, for a table that matches the array
    y = out_verts[2 * (int64_t)j];
    x = out_verts[2 * (int64_t)j + 1];
    const int yn = out_verts[2 * (int64_t)nx], xn = out_verts[2 * (int64_t)nx + 1];
    term = (long long)x * yn - (long long)xn * y;
  }
  const WaveRuns runs = wave_runs(r);
  const long long sum = wave_run_reduce(runs, term, WaveAdd());
  const int y0 = wave_run_reduce(runs, y, WaveMin()), x0 = wave_run_reduce(runs, x, WaveMin());
  const int y1 = wave_run_reduce(runs, y, WaveMax()), x1 = wave_run_reduce(runs, x, WaveMax());
  if (runs.head && r >= 0) {
    InsarRing* o = table + 1 + r;
    if (sum) SM_ADD(reinterpret_cast<long long*>(&o->area2), sum);
    SM_MIN(&o->y0, y0);
    SM_MIN(&o->x0, x0);
    SM_MAX(&o->y1, y1);
    SM_MAX(&o->x1, x1);
  }
}

__global__ void __launch_bounds__(SM_THREADS)
simplify_close_kernel(int nr, InsarRing* __restrict__ table) {
  const int r = blockIdx.x * SM_THREADS + threadIdx.x;
  if (r >= nr) return;
  InsarRing* o = table + 1 + r;
  o->y1 += 1;
  o->x1 += 1;
  o->_pad = o->count < 3 || o->area2 == 0;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct SmLayout { int64_t off[19]; int64_t bytes, table_bytes; };

static int simplify_layout(const char* who, int32_t max_vertices, int32_t max_rings, SmLayout* l) {
  if (max_vertices < 1 || max_vertices > SM_MAX_VERTICES)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_vertices %d outside 1..%d", who, max_vertices, SM_MAX_VERTICES);
  if (max_rings < 1 || max_rings > SM_MAX_RINGS) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_rings %d outside 1..%d", who, max_rings, SM_MAX_RINGS);
  const int64_t vm = max_vertices, rm = max_rings, nb = (vm + SM_THREADS - 1) / SM_THREADS;
  // the order of SmBuf: changed keep ringof seg c2 segmax segmin pos bmax bmin cmax cmin bsum nanch akey s1key s2key firstk lastk
  const int64_t size[19] = {4 * SM_COUNTERS, vm, 4 * vm, 4 * vm, 8 * vm, 16 * vm, 8 * vm, 4 * (vm + 1), 4 * nb, 4 * nb, 4 * nb, 4 * nb, 4 * nb,
                            4 * rm, 4 * rm, 4 * rm, 8 * rm, 4 * rm, 4 * rm};
  int64_t at = 0;
  for (int k = 0; k < 19; ++k) {
    l->off[k] = at;
    at += (size[k] + 15) & ~(int64_t)15;
  }
  l->bytes = at;
  l->table_bytes = (int64_t)sizeof(InsarRing) * (1 + rm);
  return INSAR_OK;
}

static SmBuf simplify_buf(const SmLayout& l, void* scratch, int32_t max_vertices) {
  char* s = (char*)scratch;
  SmBuf b;
  b.changed = (int*)(s + l.off[0]);
  b.keep = (uint8_t*)(s + l.off[1]);
  b.ringof = (int*)(s + l.off[2]);
  b.seg = (int*)(s + l.off[3]);
  b.c2 = (sm_u64*)(s + l.off[4]);
  b.segmax = (sm_u64*)(s + l.off[5]);
  b.segmin = (unsigned int*)(s + l.off[6]);
  b.pos = (int*)(s + l.off[7]);
  b.bmax = (int*)(s + l.off[8]);
  b.bmin = (int*)(s + l.off[9]);
  b.cmax = (int*)(s + l.off[10]);
  b.cmin = (int*)(s + l.off[11]);
  b.bsum = (int*)(s + l.off[12]);
  b.nanch = (int*)(s + l.off[13]);
  b.akey = (unsigned int*)(s + l.off[14]);
  b.s1key = (unsigned int*)(s + l.off[15]);
  b.s2key = (sm_u64*)(s + l.off[16]);
  b.firstk = (int*)(s + l.off[17]);
  b.lastk = (int*)(s + l.off[18]);
  b.vm = max_vertices;
  return b;
}

// what setup, rounds and finish share: the vertex array, the input ring table, the counts against the capacities, the scratch
static int simplify_check(const char* who, const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings,
                          int32_t max_vertices, int32_t max_rings, const void* scratch, SmLayout* l) {
  if (int rc = simplify_layout(who, max_vertices, max_rings, l)) return rc;
  if (!vertices || !rings || !scratch)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !vertices ? "vertices" : !rings ? "rings" : "scratch");
  if (n_vertices < 1 || n_vertices > max_vertices) INSAR_FAIL(INSAR_E_SHAPE, "%s: n_vertices %d outside 1..max_vertices = %d", who, n_vertices, max_vertices);
  if (n_rings < 1 || n_rings > max_rings) INSAR_FAIL(INSAR_E_SHAPE, "%s: n_rings %d outside 1..max_rings = %d", who, n_rings, max_rings);
  if (n_rings > n_vertices) INSAR_FAIL(INSAR_E_SHAPE, "%s: %d rings over %d vertices", who, n_rings, n_vertices);
  if (((uintptr_t)vertices) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: vertices not 8-byte aligned", who);
  if (!insar_aligned16(rings) || !insar_aligned16(scratch)) INSAR_FAIL(INSAR_E_ALIGN, "%s: rings / scratch not 16-byte aligned", who);
  return INSAR_OK;
}

extern "C" int insar_simplify_scratch_bytes(int32_t max_vertices, int32_t max_rings, int64_t* scratch_bytes, int64_t* table_bytes) {
  const char* who = "insar_simplify_scratch_bytes";
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  SmLayout l;
  if (int rc = simplify_layout(who, max_vertices, max_rings, &l)) return rc;
  *scratch_bytes = l.bytes;
  *table_bytes = l.table_bytes;
  return INSAR_OK;
}

extern "C" int insar_simplify_launches(int32_t rounds) { return 10 + 4 * (rounds < 0 ? 0 : rounds > SM_MAX_ROUNDS + 1 ? SM_MAX_ROUNDS + 1 : rounds); }

extern "C" int insar_simplify_setup(const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings, const int32_t* labels,
                                    int32_t H, int32_t W, int32_t max_vertices, int32_t max_rings, void* scratch, void* stream) {
  const char* who = "insar_simplify_setup";
  SmLayout l;
  if (int rc = simplify_check(who, vertices, n_vertices, rings, n_rings, max_vertices, max_rings, scratch, &l)) return rc;
  if (labels && (H < 1 || W < 1 || H > SM_MAX_DIM || W > SM_MAX_DIM))
    INSAR_FAIL(INSAR_E_SHAPE, "%s: label map %d x %d: 1 <= H, W <= %d", who, H, W, SM_MAX_DIM);
  if (((uintptr_t)labels) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: labels not 4-byte aligned", who);
  const SmBuf b = simplify_buf(l, scratch, max_vertices);
  const int nblk = (n_vertices + SM_THREADS - 1) / SM_THREADS;
  const InsarRing* rin = (const InsarRing*)rings + 1;
  const dim3 grid(nblk), block(SM_THREADS);
  hipStream_t s = (hipStream_t)stream;
  const int nclear = n_vertices > SM_COUNTERS ? n_vertices : SM_COUNTERS;
  hipLaunchKernelGGL(simplify_clear_kernel, dim3(insar_grid_cap((nclear + SM_THREADS - 1) / SM_THREADS)), block, 0, s, b, (int)n_vertices,
                     (int)n_rings, nblk);
  hipLaunchKernelGGL(simplify_mark_kernel, grid, block, 0, s, b, (const int*)vertices, (int)n_vertices, rin, (int)n_rings, (const int*)labels,
                     (int)H, (int)W);
  hipLaunchKernelGGL(simplify_far_kernel, grid, block, 0, s, b, (const int*)vertices, (int)n_vertices);
  hipLaunchKernelGGL(simplify_seed_kernel, grid, block, 0, s, b, (const int*)vertices, (int)n_vertices);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_simplify_rounds(const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings, int64_t eps2q,
                                     int32_t first_round, int32_t n_rounds, int32_t max_rounds, int32_t max_vertices, int32_t max_rings,
                                     void* scratch, void* stream) {
  const char* who = "insar_simplify_rounds";
  SmLayout l;
  if (int rc = simplify_check(who, vertices, n_vertices, rings, n_rings, max_vertices, max_rings, scratch, &l)) return rc;
  if (eps2q < 0 || eps2q > SM_MAX_EPSQ * SM_MAX_EPSQ)
    INSAR_FAIL(INSAR_E_ARG, "%s: eps2q %lld outside 0..%lld", who, (long long)eps2q, SM_MAX_EPSQ * SM_MAX_EPSQ);
  if (max_rounds < 1 || max_rounds > SM_MAX_ROUNDS) INSAR_FAIL(INSAR_E_ARG, "%s: max_rounds %d outside 1..%d", who, max_rounds, SM_MAX_ROUNDS);
  if (first_round < 0 || n_rounds < 1 || (int64_t)first_round + n_rounds > (int64_t)max_rounds + 1)
    INSAR_FAIL(INSAR_E_ARG, "%s: rounds %d..%d+%d outside 0..max_rounds = %d (the last one is the probe)", who, first_round, first_round,
               n_rounds, max_rounds);
  const SmBuf b = simplify_buf(l, scratch, max_vertices);
  const int nblk = (n_vertices + SM_THREADS - 1) / SM_THREADS;
  const InsarRing* rin = (const InsarRing*)rings + 1;
  const dim3 grid(nblk), block(SM_THREADS);
  hipStream_t s = (hipStream_t)stream;
  for (int rd = first_round; rd < first_round + n_rounds; ++rd) {
    hipLaunchKernelGGL(simplify_carry_kernel, dim3(1), block, 0, s, b, nblk, rd);
    hipLaunchKernelGGL(simplify_cross_kernel, grid, block, 0, s, b, (const int*)vertices, (int)n_vertices, rin, (long long)eps2q, rd);
    hipLaunchKernelGGL(simplify_tie_kernel, grid, block, 0, s, b, (const int*)vertices, (int)n_vertices, rd);
    hipLaunchKernelGGL(simplify_keep_kernel, grid, block, 0, s, b, (const int*)vertices, (int)n_vertices, rd, (int)(rd < max_rounds));
  }
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_simplify_finish(const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings, int32_t max_rounds,
                                     int32_t max_vertices, int32_t max_rings, void* scratch, void* table, int32_t* out_vertices,
                                     int32_t* out_kept, void* stream) {
  const char* who = "insar_simplify_finish";
  SmLayout l;
  if (int rc = simplify_check(who, vertices, n_vertices, rings, n_rings, max_vertices, max_rings, scratch, &l)) return rc;
  if (max_rounds < 1 || max_rounds > SM_MAX_ROUNDS) INSAR_FAIL(INSAR_E_ARG, "%s: max_rounds %d outside 1..%d", who, max_rounds, SM_MAX_ROUNDS);
  if (!table || !out_vertices || !out_kept)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !table ? "table" : !out_vertices ? "out_vertices" : "out_kept");
  if (!insar_aligned16(table)) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 16-byte aligned", who);
  if ((((uintptr_t)out_vertices) & 7u) || (((uintptr_t)out_kept) & 3u))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: out_vertices not 8-byte or out_kept not 4-byte aligned", who);
  const SmBuf b = simplify_buf(l, scratch, max_vertices);
  const int nblk = (n_vertices + SM_THREADS - 1) / SM_THREADS;
  const InsarRing* rin = (const InsarRing*)rings + 1;
  InsarRing* t = (InsarRing*)table;
  const dim3 grid(nblk), rgrid((n_rings + SM_THREADS - 1) / SM_THREADS), block(SM_THREADS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(simplify_count_kernel, grid, block, 0, s, b, (int)n_vertices);
  hipLaunchKernelGGL(simplify_scan_kernel, dim3(1), block, 0, s, b, nblk, (int)n_vertices, (int)n_rings, (int)max_rounds, t);
  hipLaunchKernelGGL(simplify_scatter_kernel, grid, block, 0, s, b, (const int*)vertices, (int)n_vertices, (int*)out_vertices, (int*)out_kept);
  hipLaunchKernelGGL(simplify_rings_kernel, rgrid, block, 0, s, b, rin, (int)n_rings, (int)n_vertices, t);
  hipLaunchKernelGGL(simplify_reduce_kernel, grid, block, 0, s, b, (const int*)out_vertices, (const int*)out_kept, (int)n_vertices, t);
  hipLaunchKernelGGL(simplify_close_kernel, rgrid, block, 0, s, (int)n_rings, t);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
