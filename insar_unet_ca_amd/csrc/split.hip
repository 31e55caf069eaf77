// Splitting touching sites: a watershed of a height map h int32 [H][W] (by default the squared distance to the region border)
// inside every label of a label map, with basins merged across saddles that lie within `min_depth` of the lower summit.
// Integers only; the rule is DESIGN.md's "Splitting touching sites", tests/split_ref.py restates it in numpy.
//
//   basins   clear     zeroes the saddle table and the control words
//            ascent    ptr[i] = the greatest-key pixel among i and its 8 neighbours of the same label, key = (h, -index);
//                      -1 on background
//            resolve   ptr[i] <- the root of i's chain (its basin), in place
//            saddles   every basin root initialises its piece state; every pixel looks E, SW, S, SE and, where the neighbour has
//                      its label but another basin, raises table[(min root, max root)] to min(h[p], h[q])
//            compact   the table's slots as an edge list {a, b, saddle}
//   rounds   per round, over the edge list only: best1 (atomic max of (saddle, peak of the neighbour)), best2 (ties: the
//            smallest root index), decide (nxt[u] = v, one count per merge), compress (up[basin] <- the end of its nxt chain;
//            the best words of the surviving roots are reset)
//   finish   best1 once more (the remaining saddle of every piece), piece (ptr[i] <- its piece's root, minimum index per
//            piece), count / scan / number (ids 1..M by ascending smallest pixel index), relabel (label map and table)
//
// No work-group ever waits on another: the phases are ordered by kernel boundaries on the caller's stream. Chases follow
// pointers along which the key strictly rises (ptr, nxt), so they end. `resolve` and `compress` replace a pointer by the end
// of its chain while other threads may still read it: either value leads to the same end (regions_flatten_kernel's argument).
// Visibility: the saddle table, the best words, the control words and (in compress) `up` are shared between work-groups of
// one launch, so every access to them in those launches is an agent-scope atomic.
// The saddle table, its clear and compact launches and the aggregation of a thread's four neighbour pairs before the atomics
// (pair_fold_insert) are pair_table.h's.
// Reproducibility: max, min and integer sums commute; which slot a pair lands in, and the order of the edge list, depend on
// arrival order, but every result taken from them is a maximum or minimum under a total order.
#include "pair_table.h"
#include "block_scan.h"
#include <limits.h>

#define SP_THREADS 256
#define SP_NB 1024                        // pixels per numbering block (256 threads x 4 pixels)
#define SP_SCAN_THREADS 1024
#define SP_MAX_ROUNDS 4096
#define SP_CTRL_WORDS 8                   // n_pairs, overflow, bad_height, raw_basins, pieces, 3 spare; then one word per round
#define SP_MAX_T (1 << 20)

// a record of pair_table_compact_kernel. pad, the high half of the slot's value, is 0: a value starts at 0 and only ever takes
// the maximum with an int32, so it stays in 0..2^31-1
struct SpEdge { int a, b, s, pad; };
static_assert(sizeof(SpEdge) == 16, "an edge is one record of pair_table_compact_kernel");
static_assert(sizeof(InsarSplitRegion) == 80, "InsarSplitRegion is five 16-byte stores");

enum { SP_NPAIRS = 0, SP_OVERFLOW = 1, SP_BADH = 2, SP_BASINS = 3, SP_PIECES = 4 };

// ---------------------------------------------------------------------------------------------
// basins
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_THREADS)
split_ascent_kernel(const int* __restrict__ labels, const int* __restrict__ h, int H, int W, int* __restrict__ ptr, int* ctrl) {
  const int64_t npix = (int64_t)H * W;
  for (int64_t i0 = blockIdx.x * (int64_t)SP_THREADS; i0 < npix; i0 += (int64_t)gridDim.x * SP_THREADS) {
    const int64_t i = i0 + threadIdx.x;
    bool bad = false;
    if (i < npix) {
      const int l = labels[i];
      int best = -1;
      if (l > 0) {
        const int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);
        int bh = h[i];
        bad = bh < 0;
        best = (int)i;
        for (int dy = -1; dy <= 1; ++dy) {
          const int yy = y + dy;
          if (yy < 0 || yy >= H) continue;
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W || (dy == 0 && dx == 0)) continue;
            const int j = yy * W + xx;
            if (labels[j] != l) continue;
            const int hj = h[j];
            if (hj > bh || (hj == bh && j < best)) { bh = hj; best = j; }
          }
        }
      }
      ptr[i] = best;
    }
    wave_count(ctrl + SP_BADH, bad);
  }
}

__global__ void __launch_bounds__(SP_THREADS)
split_resolve_kernel(int* ptr, int64_t npix) {
  for (int64_t i = blockIdx.x * (int64_t)SP_THREADS + threadIdx.x; i < npix; i += (int64_t)gridDim.x * SP_THREADS) {
    int a = ptr[i];
    if (a < 0) continue;
    for (;;) { const int p = ptr[a]; if (p == a) break; a = p; }      // the key rises strictly along ptr: the chase ends at a root
    ptr[i] = a;
  }
}

__global__ void __launch_bounds__(SP_THREADS)
split_saddles_kernel(const int* __restrict__ labels, const int* __restrict__ h, const int* __restrict__ basin, int H, int W,
                     int* __restrict__ up, int* __restrict__ nxt, int* __restrict__ bidx, unsigned long long* __restrict__ best,
                     int* ctrl, PairSlot* slots, unsigned int mask) {
  const int64_t npix = (int64_t)H * W;
  for (int64_t i0 = blockIdx.x * (int64_t)SP_THREADS; i0 < npix; i0 += (int64_t)gridDim.x * SP_THREADS) {
    const int64_t i = i0 + threadIdx.x;                            // the loop bound is uniform over the block: shuffles below
    unsigned long long k[4] = {0ull, 0ull, 0ull, 0ull};
    int v[4] = {0, 0, 0, 0};
    bool root = false;
    if (i < npix) {
      const int b = basin[i];
      if (b >= 0) {
        root = b == (int)i;
        if (root) { up[i] = b; nxt[i] = b; bidx[i] = INT_MAX; best[i] = 0ull; }
        const int l = labels[i], hi = h[i];
        const int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);
        const int qy[4] = {y, y + 1, y + 1, y + 1}, qx[4] = {x + 1, x - 1, x, x + 1};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (qy[j] >= H || qx[j] < 0 || qx[j] >= W) continue;
          const int q = qy[j] * W + qx[j];
          if (labels[q] != l) continue;
          const int bq = basin[q];
          if (bq == b) continue;
          const int lo = min(b, bq), hi2 = max(b, bq);              // hi2 >= 1: the key is never 0, the empty slot
          k[j] = ((unsigned long long)(uint32_t)lo << 32) | (unsigned long long)(uint32_t)hi2;
          v[j] = min(hi, h[q]);
        }
      }
    }
    wave_count(ctrl + SP_BASINS, root);
    pair_fold_insert<4, WaveMax>(ctrl + SP_OVERFLOW, slots, mask, k, v);
  }
}

// ---------------------------------------------------------------------------------------------
// rounds: over the edge list. up[a] is the root of basin a's piece at the start of the round.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long sp_pack(int s, int hv) {          // (saddle + 1, peak of the neighbour); 0: none
  return ((unsigned long long)((uint32_t)s + 1u) << 32) | (unsigned long long)(uint32_t)hv;
}
__device__ __forceinline__ long long sp_isqrt(long long x) {                     // exact for 0 <= x < 2^52
  long long r = (long long)sqrt((double)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}
// sixteenths of a pixel between two squared distances (256 * (2^31 - 1) needs 64 bits), or the plain difference
__device__ __forceinline__ long long sp_depth(int P, int S, int squared) {
  const long long p = max(P, 0), s = max(S, 0);
  return squared ? sp_isqrt(256ll * p) - sp_isqrt(256ll * s) : p - s;
}
__device__ __forceinline__ int sp_edge_count(const int* ctrl, int64_t max_pairs) {
  const int64_t n = ctrl[SP_NPAIRS];                              // written by `compact`, a launch before
  return (int)(n < max_pairs ? n : max_pairs);
}

__global__ void __launch_bounds__(SP_THREADS)
split_best1_kernel(const SpEdge* __restrict__ edges, const int* __restrict__ ctrl, int64_t max_pairs, const int* __restrict__ up,
                   const int* __restrict__ h, unsigned long long* best) {
  const int n = sp_edge_count(ctrl, max_pairs);
  for (int t = blockIdx.x * SP_THREADS + threadIdx.x; t < n; t += gridDim.x * SP_THREADS) {
    const SpEdge e = edges[t];
    const int u = up[e.a], v = up[e.b];
    if (u == v) continue;
    __hip_atomic_fetch_max(best + u, sp_pack(e.s, h[v]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(best + v, sp_pack(e.s, h[u]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(SP_THREADS)
split_best2_kernel(const SpEdge* __restrict__ edges, const int* __restrict__ ctrl, int64_t max_pairs, const int* __restrict__ up,
                   const int* __restrict__ h, const unsigned long long* __restrict__ best, int* bidx) {
  const int n = sp_edge_count(ctrl, max_pairs);
  for (int t = blockIdx.x * SP_THREADS + threadIdx.x; t < n; t += gridDim.x * SP_THREADS) {
    const SpEdge e = edges[t];
    const int u = up[e.a], v = up[e.b];
    if (u == v) continue;
    if (best[u] == sp_pack(e.s, h[v])) __hip_atomic_fetch_min(bidx + u, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (best[v] == sp_pack(e.s, h[u])) __hip_atomic_fetch_min(bidx + v, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// u merges into its best neighbour v iff depth(peak u, saddle) <= T and key(v) > key(u). Several edges may realise the same
// (u, v, saddle): they write the same nxt[u] and each count one, so the round's word is zero iff nothing merged.
__device__ __forceinline__ bool sp_decide(int u, int v, int s, const int* __restrict__ h, const unsigned long long* __restrict__ best,
                                          const int* __restrict__ bidx, int squared, long long T, int* __restrict__ nxt) {
  const int hu = h[u], hv = h[v];
  if (best[u] != sp_pack(s, hv) || bidx[u] != v) return false;
  if (sp_depth(hu, s, squared) > T || !(hv > hu || (hv == hu && v < u))) return false;
  nxt[u] = v;
  return true;
}
__global__ void __launch_bounds__(SP_THREADS)
split_decide_kernel(const SpEdge* __restrict__ edges, int* ctrl, int64_t max_pairs, const int* __restrict__ up,
                    const int* __restrict__ h, const unsigned long long* __restrict__ best, const int* __restrict__ bidx,
                    int squared, long long T, int* __restrict__ nxt, int round) {
  const int n = sp_edge_count(ctrl, max_pairs);
  for (int t0 = blockIdx.x * SP_THREADS; t0 < n; t0 += gridDim.x * SP_THREADS) {
    const int t = t0 + threadIdx.x;
    bool merged = false;
    if (t < n) {
      const SpEdge e = edges[t];
      const int u = up[e.a], v = up[e.b];
      if (u != v) {
        merged = sp_decide(u, v, e.s, h, best, bidx, squared, T, nxt);
        merged |= sp_decide(v, u, e.s, h, best, bidx, squared, T, nxt);
      }
    }
    wave_count(ctrl + SP_CTRL_WORDS + round, merged);
  }
}

__global__ void __launch_bounds__(SP_THREADS)
split_compress_kernel(const SpEdge* __restrict__ edges, const int* __restrict__ ctrl, int64_t max_pairs, int* up,
                      const int* __restrict__ nxt, int* __restrict__ bidx, unsigned long long* __restrict__ best) {
  const int n = sp_edge_count(ctrl, max_pairs);
  for (int t = blockIdx.x * SP_THREADS + threadIdx.x; t < n; t += gridDim.x * SP_THREADS) {
    const SpEdge e = edges[t];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int x = side ? e.b : e.a;
      int r = agent_load(up + x);                                  // the old root or, from another edge of x, already the new one
      for (;;) { const int m = nxt[r]; if (m == r) break; r = m; }
      agent_store(up + x, r);
      bidx[r] = INT_MAX;                                           // every writer of these two stores the same values
      best[r] = 0ull;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// finish
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_THREADS)
split_piece_kernel(int* __restrict__ basin, const int* __restrict__ up, int* bidx, int64_t npix) {
  for (int64_t i0 = blockIdx.x * (int64_t)SP_THREADS; i0 < npix; i0 += (int64_t)gridDim.x * SP_THREADS) {
    const int64_t i = i0 + threadIdx.x;
    int pc = -1;
    if (i < npix) {
      const int b = basin[i];
      if (b >= 0) { pc = up[b]; basin[i] = pc; }                  // basin[r] of a root r is read by pixel r alone
    }
    if (__ballot(pc >= 0) == 0) continue;
    const WaveRuns runs = wave_runs(pc);
    const int first = wave_run_reduce(runs, pc >= 0 ? (int)i : INT_MAX, WaveMin());
    if (runs.head && pc >= 0) __hip_atomic_fetch_min(bidx + pc, first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ int sp_block_firsts(const int* __restrict__ piece, const int* __restrict__ bidx, int64_t i, int64_t npix,
                                               bool* first) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pc = i + j < npix ? piece[i + j] : -1;
    first[j] = pc >= 0 && bidx[pc] == (int)(i + j);
    c += first[j];
  }
  return c;
}

__global__ void __launch_bounds__(SP_THREADS)
split_count_kernel(const int* __restrict__ piece, const int* __restrict__ bidx, int64_t npix, int* __restrict__ counts,
                   InsarSplitRegion* __restrict__ table, int max_regions) {
  __shared__ int wsum[SP_THREADS / INSAR_WAVE];
  const int64_t i = (int64_t)blockIdx.x * SP_NB + threadIdx.x * 4;
  bool first[4];
  int total;
  block_prefix_sum<SP_THREADS>(sp_block_firsts(piece, bidx, i, npix, first), wsum, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
  // the table's records (the header is written by the scan): empty sums, an empty box
  int4* t4 = reinterpret_cast<int4*>(table + 1);
  for (int64_t r = blockIdx.x * (int64_t)SP_THREADS + threadIdx.x; r < max_regions; r += (int64_t)gridDim.x * SP_THREADS) {
    t4[5 * r + 0] = make_int4(0, 0, 0, 0);
    t4[5 * r + 1] = make_int4(0, 0, 0, 0);
    t4[5 * r + 2] = make_int4(INT_MAX, INT_MAX, 0, 0);
    t4[5 * r + 3] = make_int4(-1, 0, 0, 0);
    t4[5 * r + 4] = make_int4(-1, -1, 0, 0);
  }
}

__global__ void __launch_bounds__(SP_SCAN_THREADS)
split_scan_kernel(int* __restrict__ counts, int nblk, int* __restrict__ ctrl, InsarSplitRegion* __restrict__ table) {
  __shared__ int wsum[SP_SCAN_THREADS / INSAR_WAVE];
  const int carry = block_scan_array<SP_SCAN_THREADS>(counts, nblk, wsum);
  if (threadIdx.x == 0) {                                          // header record: {M, pairs, overflow, bad heights; raw basins}
    InsarSplitRegion hd = {};
    hd.area = carry;
    hd.sum_y = ctrl[SP_NPAIRS];
    hd.sum_x = ctrl[SP_OVERFLOW];
    hd.sum_conf = ctrl[SP_BADH];
    hd.y0 = ctrl[SP_BASINS];
    table[0] = hd;
    ctrl[SP_PIECES] = carry;
  }
}

__global__ void __launch_bounds__(SP_THREADS)
split_number_kernel(const int* __restrict__ piece, const int* __restrict__ bidx, const unsigned long long* __restrict__ best,
                    const int* __restrict__ labels, const int* __restrict__ h, const uint8_t* __restrict__ mask, int64_t npix,
                    const int* __restrict__ counts, int* __restrict__ ids, InsarSplitRegion* __restrict__ table, int max_regions) {
  __shared__ int wsum[SP_THREADS / INSAR_WAVE];
  const int64_t i = (int64_t)blockIdx.x * SP_NB + threadIdx.x * 4;
  bool first[4];
  const int c = sp_block_firsts(piece, bidx, i, npix, first);
  int total;
  int id = counts[blockIdx.x] + block_prefix_sum<SP_THREADS>(c, wsum, &total);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!first[j]) continue;
    const int pc = piece[i + j];
    ids[pc] = ++id;
    if (id <= max_regions) {
      int4* r = reinterpret_cast<int4*>(table + id);
      r[3] = make_int4((int)(i + j), mask ? (int)mask[i + j] : 0, labels[i + j], h[pc]);
      r[4] = make_int4(pc, (int)((long long)(best[pc] >> 32) - 1ll), 0, 0);
    }
  }
}

// labels_out[i] = ids[piece(i)] and the statistics of the pieces: lanes of a wave combine over runs of a label, the first
// lane of a run issues the atomics. Ids above max_regions write labels (scene-sized) but never the table.
__global__ void __launch_bounds__(SP_THREADS)
split_relabel_kernel(const int* __restrict__ piece, const int* __restrict__ ids, const float* __restrict__ conf, int64_t npix, int W,
                     int* __restrict__ labels_out, InsarSplitRegion* __restrict__ table, int max_regions) {
  for (int64_t i0 = blockIdx.x * (int64_t)SP_THREADS; i0 < npix; i0 += (int64_t)gridDim.x * SP_THREADS) {
    const int64_t i = i0 + threadIdx.x;
    int id = 0, y = 0, x = 0;
    long long sc = 0;
    if (i < npix) {
      const int pc = piece[i];
      id = pc >= 0 ? ids[pc] : 0;
      labels_out[i] = id;
      y = (int)((uint32_t)i / (uint32_t)W);
      x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);
      if (conf && id) sc = __float2ll_rn(fminf(fmaxf(conf[i], 0.f), 1.f) * 1073741824.0f);
    }
    if (__ballot(id > 0) == 0) continue;
    const WaveRuns runs = wave_runs(id);
    const long long n = wave_run_reduce(runs, (long long)(id > 0), WaveAdd());
    const long long ty = wave_run_reduce(runs, (long long)y, WaveAdd());
    const long long tx = wave_run_reduce(runs, (long long)x, WaveAdd());
    const long long tc = conf ? wave_run_reduce(runs, sc, WaveAdd()) : 0;
    const int by0 = wave_run_reduce(runs, y, WaveMin()), by1 = wave_run_reduce(runs, y + 1, WaveMax());
    const int bx0 = wave_run_reduce(runs, x, WaveMin()), bx1 = wave_run_reduce(runs, x + 1, WaveMax());
    if (runs.head && id > 0 && id <= max_regions) {
      InsarSplitRegion* r = table + id;
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->area), (unsigned long long)n);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_y), (unsigned long long)ty);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_x), (unsigned long long)tx);
      if (conf) atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_conf), (unsigned long long)tc);
      atomicMin(&r->y0, by0); atomicMin(&r->x0, bx0);
      atomicMax(&r->y1, by1); atomicMax(&r->x1, bx1);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side: scratch layout and the four entry points
// ---------------------------------------------------------------------------------------------
struct SpLayout {
  int64_t npix, seg, nblk, cap, ctrl_words;
  int64_t off_up, off_nxt, off_bidx, off_best, off_counts, off_ctrl, off_slots, off_edges, bytes;
};

static int split_layout(const char* who, int32_t H, int32_t W, int64_t max_pairs, int32_t max_rounds, SpLayout* L) {
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  const int64_t npix = (int64_t)H * W;
  if (npix >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^31 pixels or more", who, H, W);
  if (int rc = pair_table_capacity(who, max_pairs, &L->cap)) return rc;
  if (max_rounds < 1 || max_rounds > SP_MAX_ROUNDS)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_rounds %d outside 1..%d", who, max_rounds, SP_MAX_ROUNDS);
  L->npix = npix;
  L->seg = insar_align16(npix * 4);
  L->nblk = (npix + SP_NB - 1) / SP_NB;
  L->ctrl_words = insar_align16((SP_CTRL_WORDS + (int64_t)max_rounds) * 4) / 4;
  L->off_up = L->seg;
  L->off_nxt = 2 * L->seg;
  L->off_bidx = 3 * L->seg;
  L->off_best = 4 * L->seg;
  L->off_counts = 6 * L->seg;
  L->off_ctrl = L->off_counts + insar_align16(L->nblk * 4);
  L->off_slots = L->off_ctrl + L->ctrl_words * 4;
  L->off_edges = L->off_slots + L->cap * (int64_t)sizeof(PairSlot);
  L->bytes = L->off_edges + max_pairs * (int64_t)sizeof(SpEdge);
  return INSAR_OK;
}

extern "C" int insar_split_scratch_bytes(int32_t H, int32_t W, int32_t max_regions, int64_t max_pairs, int32_t max_rounds,
                                         int64_t* scratch_bytes, int64_t* table_bytes, int64_t* ctrl_offset, int64_t* ctrl_bytes) {
  const char* who = "insar_split_scratch_bytes";
  if (!scratch_bytes || !table_bytes || !ctrl_offset || !ctrl_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  SpLayout L;
  if (int rc = split_layout(who, H, W, max_pairs, max_rounds, &L)) return rc;
  if (max_regions < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d < 1", who, max_regions);
  *scratch_bytes = L.bytes;
  *table_bytes = (int64_t)sizeof(InsarSplitRegion) * ((int64_t)max_regions + 1);
  *ctrl_offset = L.off_ctrl;
  *ctrl_bytes = L.ctrl_words * 4;
  return INSAR_OK;
}

extern "C" int insar_split_basins(const int32_t* labels, const int32_t* height, int32_t H, int32_t W, int64_t max_pairs,
                                  int32_t max_rounds, void* scratch, void* stream) {
  const char* who = "insar_split_basins";
  if (int rc = scene_check_map(who, "labels", labels, 4)) return rc;
  if (int rc = scene_check_map(who, "height", height, 4)) return rc;
  SpLayout L;
  if (int rc = split_layout(who, H, W, max_pairs, max_rounds, &L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  int *basin = scratch_at<int>(scratch, 0), *ctrl = scratch_at<int>(scratch, L.off_ctrl);
  PairSlot* slots = scratch_at<PairSlot>(scratch, L.off_slots);
  pair_table_clear(s, slots, L.cap, ctrl, (int)(L.ctrl_words / 4));
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_ascent_kernel, scene_grid(L.npix, SP_THREADS), dim3(SP_THREADS), 0, s, (const int*)labels, (const int*)height, H, W,
                     basin, ctrl);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_resolve_kernel, scene_grid(L.npix, SP_THREADS), dim3(SP_THREADS), 0, s, basin, L.npix);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_saddles_kernel, scene_grid(L.npix, SP_THREADS), dim3(SP_THREADS), 0, s, (const int*)labels, (const int*)height,
                     (const int*)basin, H, W, scratch_at<int>(scratch, L.off_up), scratch_at<int>(scratch, L.off_nxt),
                     scratch_at<int>(scratch, L.off_bidx), scratch_at<unsigned long long>(scratch, L.off_best), ctrl, slots,
                     (unsigned int)(L.cap - 1));
  INSAR_CHECK_LAUNCH(who);
  pair_table_compact(s, slots, L.cap, max_pairs, ctrl + SP_NPAIRS, scratch_at<SpEdge>(scratch, L.off_edges));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_split_rounds(const int32_t* height, int32_t H, int32_t W, int32_t squared, int32_t threshold,
                                  int32_t first_round, int32_t n_rounds, int64_t max_pairs, int32_t max_rounds, void* scratch,
                                  void* stream) {
  const char* who = "insar_split_rounds";
  if (int rc = scene_check_map(who, "height", height, 4)) return rc;
  SpLayout L;
  if (int rc = split_layout(who, H, W, max_pairs, max_rounds, &L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (threshold < 0 || threshold > SP_MAX_T) INSAR_FAIL(INSAR_E_ARG, "%s: threshold %d outside 0..%d", who, threshold, SP_MAX_T);
  if (first_round < 0 || n_rounds < 1 || (int64_t)first_round + n_rounds > max_rounds)
    INSAR_FAIL(INSAR_E_ARG, "%s: rounds %d..%d outside 0..%d", who, first_round, first_round + n_rounds, max_rounds);
  hipStream_t s = (hipStream_t)stream;
  int *up = scratch_at<int>(scratch, L.off_up), *nxt = scratch_at<int>(scratch, L.off_nxt), *bidx = scratch_at<int>(scratch, L.off_bidx);
  int* ctrl = scratch_at<int>(scratch, L.off_ctrl);
  unsigned long long* best = scratch_at<unsigned long long>(scratch, L.off_best);
  const SpEdge* edges = scratch_at<SpEdge>(scratch, L.off_edges);
  const dim3 grid = scene_grid(max_pairs, SP_THREADS), block(SP_THREADS);
  for (int r = first_round; r < first_round + n_rounds; ++r) {
    hipLaunchKernelGGL(split_best1_kernel, grid, block, 0, s, edges, (const int*)ctrl, max_pairs, (const int*)up, (const int*)height, best);
    INSAR_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(split_best2_kernel, grid, block, 0, s, edges, (const int*)ctrl, max_pairs, (const int*)up, (const int*)height,
                       (const unsigned long long*)best, bidx);
    INSAR_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(split_decide_kernel, grid, block, 0, s, edges, ctrl, max_pairs, (const int*)up, (const int*)height,
                       (const unsigned long long*)best, (const int*)bidx, (int)(squared != 0), (long long)threshold, nxt, r);
    INSAR_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(split_compress_kernel, grid, block, 0, s, edges, (const int*)ctrl, max_pairs, up, (const int*)nxt, bidx, best);
    INSAR_CHECK_LAUNCH(who);
  }
  return INSAR_OK;
}

extern "C" int insar_split_finish(const int32_t* labels, const int32_t* height, const uint8_t* mask, const float* conf, int32_t H,
                                  int32_t W, int32_t max_regions, int64_t max_pairs, int32_t max_rounds, void* scratch, void* table,
                                  int32_t* labels_out, void* stream) {
  const char* who = "insar_split_finish";
  if (int rc = scene_check_map(who, "labels", labels, 4)) return rc;
  if (int rc = scene_check_map(who, "height", height, 4)) return rc;
  if (int rc = scene_check_map(who, "labels_out", labels_out, 4)) return rc;
  if (((uintptr_t)conf) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: conf not 4-byte aligned", who);
  SpLayout L;
  if (int rc = split_layout(who, H, W, max_pairs, max_rounds, &L)) return rc;
  if (max_regions < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d < 1", who, max_regions);
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  hipStream_t s = (hipStream_t)stream;
  int *piece = scratch_at<int>(scratch, 0), *up = scratch_at<int>(scratch, L.off_up), *ids = scratch_at<int>(scratch, L.off_nxt);
  int *bidx = scratch_at<int>(scratch, L.off_bidx), *counts = scratch_at<int>(scratch, L.off_counts), *ctrl = scratch_at<int>(scratch, L.off_ctrl);
  unsigned long long* best = scratch_at<unsigned long long>(scratch, L.off_best);
  InsarSplitRegion* t = (InsarSplitRegion*)table;
  const dim3 block(SP_THREADS);
  hipLaunchKernelGGL(split_best1_kernel, scene_grid(max_pairs, SP_THREADS), block, 0, s, (const SpEdge*)scratch_at<SpEdge>(scratch, L.off_edges),
                     (const int*)ctrl, max_pairs, (const int*)up, (const int*)height, best);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_piece_kernel, scene_grid(L.npix, SP_THREADS), block, 0, s, piece, (const int*)up, bidx, L.npix);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_count_kernel, dim3((unsigned)L.nblk), block, 0, s, (const int*)piece, (const int*)bidx, L.npix, counts, t,
                     max_regions);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(SP_SCAN_THREADS), 0, s, counts, (int)L.nblk, ctrl, t);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_number_kernel, dim3((unsigned)L.nblk), block, 0, s, (const int*)piece, (const int*)bidx,
                     (const unsigned long long*)best, (const int*)labels, (const int*)height, mask, L.npix, (const int*)counts, ids, t,
                     max_regions);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(split_relabel_kernel, scene_grid(L.npix, SP_THREADS), block, 0, s, (const int*)piece, (const int*)ids, conf, L.npix, W,
                     labels_out, t, max_regions);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
