// Outline simplification: Douglas-Peucker over the rings of the region outlines (outline.hip), in exact integers and aware of
// shared borders. Semantics: include/insar_hip.h, "outline simplification". The round and finish stages, the scratch core and
// the host checks are those of dp_common.h; this file owns how a ring is seeded, the deviation of a vertex and the tie-break.
//
//   setup   clear    counters, both parities of the segment slots, the block and ring records
//           mark     per vertex: its ring, the anchor flag from four label reads; per ring the anchor count, the anchor's key
//                    and the smallest key (y << 16 | x)
//           far      per vertex of a ring with fewer than two anchors: squared distance from seed 1, a 64-bit atomic max of
//                    (d2 << 32 | 2^31 - 1 - key) per ring: the farthest vertex, ties to the smallest key
//           seed     per vertex: every position that carries the coordinates of seed 1 or seed 2 is kept
//   round   cross    cross^2 against the chord of dp_neighbours
//           tie      per candidate that equals the maximum: atomic min of its key on the segment's second slot
//           keep     per candidate that equals both: kept
//
// 4 + 4 per round + 6 launches. Ties go to the smallest (y, x), never to the smallest position, so that both directions of a
// shared arc agree.
// Exactness: coordinates <= 2^14, so |cross| < 2^30 and cross^2 < 2^60 fit 64 bits; 256 cross^2 > eps2q |b - a|^2 is tested as
// cross^2 > floor(eps2q |b - a|^2 / 256), the same for integers, with eps2q |b - a|^2 < 2^58. No float anywhere.
#include "dp_common.h"

#define SM_MAX_RINGS (1 << 26)
#define SM_MAX_DIM 16384
#define SM_MAX_EPSQ 16384ll                // round(1024 * 16)

// the scratch: the core, the segment slots of both parities, the seeds of every ring
struct SmBuf : DpCore {
  dp_u64* segmax;            // [2][vm] largest cross^2 (or squared distance from a degenerate chord) of the segment
  unsigned int* segmin;      // [2][vm] smallest key among those
  int* nanch;                // [rings]
  unsigned int *akey, *s1key;
  dp_u64* s2key;
};

__device__ __forceinline__ unsigned int sm_key(int y, int x) { return ((unsigned int)y << 16) | (unsigned int)x; }
__device__ __forceinline__ unsigned int sm_key_at(const int* verts, int i) { return sm_key(verts[2 * (int64_t)i], verts[2 * (int64_t)i + 1]); }

// ---------------------------------------------------------------------------------------------
// setup: clear / mark / far / seed
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DP_THREADS)
simplify_clear_kernel(SmBuf b, int nv, int nr, int nblk) {
  const int n = max(max(nv, nr), max(nblk, DP_COUNTERS));
  for (int i = blockIdx.x * DP_THREADS + threadIdx.x; i < n; i += gridDim.x * DP_THREADS) {
    dp_clear(b, i, nblk, nr);
    if (i < nv) {
      b.segmax[i] = 0ull;
      b.segmax[(int64_t)b.vm + i] = 0ull;
      b.segmin[i] = ~0u;
      b.segmin[(int64_t)b.vm + i] = ~0u;
    }
    if (i < nr) {
      b.nanch[i] = 0;
      b.akey[i] = ~0u;
      b.s1key[i] = ~0u;
      b.s2key[i] = 0ull;
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

__global__ void __launch_bounds__(DP_THREADS)
simplify_mark_kernel(SmBuf b, const int* __restrict__ verts, int nv, const InsarRing* __restrict__ rings, int nr,
                     const int* __restrict__ labels, int H, int W) {
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  int r = -1, anchor = 0;
  unsigned int key = ~0u;
  if (i < nv) {
    r = dp_record_of(rings, nr, i);
    const int y = verts[2 * (int64_t)i], x = verts[2 * (int64_t)i + 1];
    key = sm_key(y, x);
    anchor = labels ? (int)sm_anchor(labels, H, W, y, x) : 0;
    b.lineof[i] = r;
    b.keep[i] = (uint8_t)anchor;
    if (anchor) dp_note_kept(b, i, r);
  }
  const WaveRuns runs = wave_runs(r);
  const unsigned int mn = wave_run_reduce(runs, key, WaveMin());
  const int na = wave_run_reduce(runs, anchor, WaveAdd());
  const unsigned int ak = wave_run_reduce(runs, anchor ? key : ~0u, WaveMin());
  if (runs.head && r >= 0) {
    DP_MIN(&b.s1key[r], mn);
    if (na) {
      DP_ADD(&b.nanch[r], na);
      DP_MIN(&b.akey[r], ak);
    }
  }
}

__global__ void __launch_bounds__(DP_THREADS)
simplify_far_kernel(SmBuf b, const int* __restrict__ verts, int nv) {
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  int r = -1;
  dp_u64 k = 0ull;
  if (i < nv) {
    const int ring = b.lineof[i];
    const int na = b.nanch[ring];
    if (na < 2) {
      r = ring;
      const unsigned int s1 = na == 1 ? b.akey[ring] : b.s1key[ring];
      const int y = verts[2 * (int64_t)i], x = verts[2 * (int64_t)i + 1];
      const long long dy = y - (int)(s1 >> 16), dx = x - (int)(s1 & 0xffffu);
      k = ((dp_u64)(dy * dy + dx * dx) << 32) | (dp_u64)(0x7fffffffu - sm_key(y, x));
    }
  }
  const WaveRuns runs = wave_runs(r);
  const dp_u64 mx = wave_run_reduce(runs, k, WaveMax());
  if (runs.head && r >= 0) DP_MAX(&b.s2key[r], mx);
}

__global__ void __launch_bounds__(DP_THREADS)
simplify_seed_kernel(SmBuf b, const int* __restrict__ verts, int nv) {
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  if (i >= nv) return;
  const int r = b.lineof[i];
  const int na = b.nanch[r];
  if (na >= 2 || b.keep[i]) return;
  const unsigned int s1 = na == 1 ? b.akey[r] : b.s1key[r];
  const unsigned int s2 = 0x7fffffffu - (unsigned int)(b.s2key[r] & 0xffffffffull);
  const unsigned int key = sm_key_at(verts, i);
  if (key == s1 || key == s2) {
    b.keep[i] = 1;
    dp_note_kept(b, i, r);
  }
}

// ---------------------------------------------------------------------------------------------
// one round: (carry) / cross / tie / keep
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DP_THREADS)
simplify_cross_kernel(SmBuf b, const int* __restrict__ verts, int nv, const InsarRing* __restrict__ rings, long long eps2q, int rd) {
  __shared__ int w[DP_WAVES];
  if (dp_idle(b, rd)) return;
  const int par = rd & 1;
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  int p = -1, sg = -1;
  DpChord c;
  const bool undecided = dp_neighbours(b, verts, nv, rings, i, w, &p, &c);
  dp_u64 num = 0ull;
  if (i < nv) {
    const int64_t other = (int64_t)(par ^ 1) * b.vm + i;         // nobody reads the other parity during this round
    b.segmax[other] = 0ull;
    b.segmin[other] = ~0u;
    if (undecided) {
      const long long len2 = c.dy * c.dy + c.dx * c.dx;
      const long long cr = c.dx * c.py - c.dy * c.px;
      // a chord whose ends coincide: the distance from that point takes the place of the distance from the line
      const dp_u64 n = len2 ? (dp_u64)(cr * cr) : (dp_u64)(c.py * c.py + c.px * c.px);
      const dp_u64 thr = (dp_u64)(eps2q * (len2 ? len2 : 1ll)) >> 8;
      if (n > thr) {
        sg = p;
        num = n;
      }
    }
    b.seg[i] = sg;
    b.dev[i] = num;
  }
  dp_raise_max(b.segmax + (int64_t)par * b.vm, sg, num);
}

__global__ void __launch_bounds__(DP_THREADS)
simplify_tie_kernel(SmBuf b, const int* __restrict__ verts, int nv, int rd) {
  if (dp_idle(b, rd)) return;
  const int par = rd & 1;
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  int sg = i < nv ? b.seg[i] : -1;
  unsigned int key = ~0u;
  if (sg >= 0) {
    if (b.dev[i] == b.segmax[(int64_t)par * b.vm + sg]) key = sm_key_at(verts, i);
    else sg = -1;
  }
  const WaveRuns runs = wave_runs(sg);
  const unsigned int mn = wave_run_reduce(runs, key, WaveMin());
  if (runs.head && sg >= 0) DP_MIN(&b.segmin[(int64_t)par * b.vm + sg], mn);
}

__global__ void __launch_bounds__(DP_THREADS)
simplify_keep_kernel(SmBuf b, const int* __restrict__ verts, int nv, int rd, int apply) {
  if (dp_idle(b, rd)) return;
  const int par = rd & 1;
  const int i = blockIdx.x * DP_THREADS + threadIdx.x;
  const int sg = i < nv ? b.seg[i] : -1;
  bool win = false;
  if (sg >= 0) {
    const int64_t slot = (int64_t)par * b.vm + sg;
    win = b.dev[i] == b.segmax[slot] && sm_key_at(verts, i) == b.segmin[slot];
  }
  dp_keep(b, i, win, apply, rd);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int simplify_layout(const char* who, int32_t max_vertices, int32_t max_rings, DpLayout* l) {
  const int64_t vm = max_vertices, rm = max_rings;
  const int64_t own[6] = {16 * vm, 8 * vm, 4 * rm, 4 * rm, 4 * rm, 8 * rm};      // segmax segmin nanch akey s1key s2key
  return dp_layout(who, "ring", max_vertices, max_rings, SM_MAX_RINGS, own, 6, l);
}

static SmBuf simplify_buf(const DpLayout& l, void* scratch, int32_t max_vertices) {
  const int64_t* own = l.off + DP_CORE_SECTIONS;
  SmBuf b;
  dp_carve(l, scratch, max_vertices, &b);
  b.segmax = scratch_at<dp_u64>(scratch, own[0]);
  b.segmin = scratch_at<unsigned int>(scratch, own[1]);
  b.nanch = scratch_at<int>(scratch, own[2]);
  b.akey = scratch_at<unsigned int>(scratch, own[3]);
  b.s1key = scratch_at<unsigned int>(scratch, own[4]);
  b.s2key = scratch_at<dp_u64>(scratch, own[5]);
  return b;
}

static int simplify_check(const char* who, const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings,
                          int32_t max_vertices, int32_t max_rings, const void* scratch, DpLayout* l) {
  if (int rc = simplify_layout(who, max_vertices, max_rings, l)) return rc;
  return dp_check(who, "ring", vertices, n_vertices, rings, n_rings, 1, max_vertices, max_rings, scratch);     // a ring of one vertex is one
}

extern "C" int insar_simplify_scratch_bytes(int32_t max_vertices, int32_t max_rings, int64_t* scratch_bytes, int64_t* table_bytes) {
  const char* who = "insar_simplify_scratch_bytes";
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  DpLayout l;
  if (int rc = simplify_layout(who, max_vertices, max_rings, &l)) return rc;
  *scratch_bytes = l.bytes;
  *table_bytes = l.table_bytes;
  return INSAR_OK;
}

extern "C" int insar_simplify_launches(int32_t rounds) { return dp_launches(10, 4, rounds); }

extern "C" int insar_simplify_setup(const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings, const int32_t* labels,
                                    int32_t H, int32_t W, int32_t max_vertices, int32_t max_rings, void* scratch, void* stream) {
  const char* who = "insar_simplify_setup";
  DpLayout l;
  if (int rc = simplify_check(who, vertices, n_vertices, rings, n_rings, max_vertices, max_rings, scratch, &l)) return rc;
  if (labels && (H < 1 || W < 1 || H > SM_MAX_DIM || W > SM_MAX_DIM))
    INSAR_FAIL(INSAR_E_SHAPE, "%s: label map %d x %d: 1 <= H, W <= %d", who, H, W, SM_MAX_DIM);
  if (((uintptr_t)labels) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: labels not 4-byte aligned", who);
  const SmBuf b = simplify_buf(l, scratch, max_vertices);
  const int nblk = (n_vertices + DP_THREADS - 1) / DP_THREADS;
  const InsarRing* rin = (const InsarRing*)rings + 1;
  const dim3 grid(nblk), block(DP_THREADS);
  hipStream_t s = (hipStream_t)stream;
  const int nclear = n_vertices > DP_COUNTERS ? n_vertices : DP_COUNTERS;
  hipLaunchKernelGGL(simplify_clear_kernel, dim3(insar_grid_cap((nclear + DP_THREADS - 1) / DP_THREADS)), block, 0, s, b, (int)n_vertices,
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
  DpLayout l;
  if (int rc = simplify_check(who, vertices, n_vertices, rings, n_rings, max_vertices, max_rings, scratch, &l)) return rc;
  if (eps2q < 0 || eps2q > SM_MAX_EPSQ * SM_MAX_EPSQ)
    INSAR_FAIL(INSAR_E_ARG, "%s: eps2q %lld outside 0..%lld", who, (long long)eps2q, SM_MAX_EPSQ * SM_MAX_EPSQ);
  if (int rc = dp_check_rounds(who, first_round, n_rounds, max_rounds)) return rc;
  const SmBuf b = simplify_buf(l, scratch, max_vertices);
  const int nv = n_vertices, nblk = (nv + DP_THREADS - 1) / DP_THREADS;
  const InsarRing* rin = (const InsarRing*)rings + 1;
  const int* v = (const int*)vertices;
  const dim3 grid(nblk), block(DP_THREADS);
  hipStream_t s = (hipStream_t)stream;
  return dp_rounds(who, b, nblk, first_round, n_rounds, max_rounds, s, [&](int rd, int apply) {
    hipLaunchKernelGGL(simplify_cross_kernel, grid, block, 0, s, b, v, nv, rin, (long long)eps2q, rd);
    hipLaunchKernelGGL(simplify_tie_kernel, grid, block, 0, s, b, v, nv, rd);
    hipLaunchKernelGGL(simplify_keep_kernel, grid, block, 0, s, b, v, nv, rd, apply);
  });
}

extern "C" int insar_simplify_finish(const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings, int32_t max_rounds,
                                     int32_t max_vertices, int32_t max_rings, void* scratch, void* table, int32_t* out_vertices,
                                     int32_t* out_kept, void* stream) {
  const char* who = "insar_simplify_finish";
  DpLayout l;
  if (int rc = simplify_check(who, vertices, n_vertices, rings, n_rings, max_vertices, max_rings, scratch, &l)) return rc;
  return dp_finish<InsarRing>(who, simplify_buf(l, scratch, max_vertices), vertices, n_vertices, rings, n_rings, max_rounds, table,
                              out_vertices, out_kept, stream);
}
