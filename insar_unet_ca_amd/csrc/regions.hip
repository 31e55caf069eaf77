// Regions of a class map: connected-component labelling of a uint8 class map [H][W] (4- or 8-connectivity, pixels of the same
// non-zero class), per-region integer statistics, a minimum-area / minimum-confidence filter and ids 1..N in ascending order
// of each region's smallest row-major pixel index (its root). Seven launches per call, whatever the mask holds:
//
//   tiles    one work-group labels a 32 x 64 tile in LDS (horizontal runs by ballot, then a lock-free union-find with
//            atomicMin on LDS for the links between rows) and writes, per pixel, the GLOBAL index of the smallest pixel of
//            its tile-local component (-1: background); clears the area scratch
//   merge    one thread per pixel on a tile border unions it with its neighbours in the adjacent tile
//   flatten  every pixel's parent becomes its root; the root's area is counted (one atomic per wave and run of a root)
//   count    per block of 1024 pixels: how many roots are kept (area >= min_area); also clears the region table
//   scan     one work-group: exclusive prefix sum of the block counts; the total N goes to the table header
//   number   per block: kept roots get ids base + 1.., stored in place of their area; dropped roots get 0
//   relabel  labels / cleaned mask per pixel, statistics into the table (one set of atomics per wave and run of a label)
//
// No work-group ever waits on another: the phases are ordered by kernel boundaries on the caller's stream, and every loop
// walks a strictly decreasing parent index (parent[i] <= i always; links go from the larger root to the smaller).
// Visibility: in `merge` work-groups on different XCDs update one parent array, so every access to it there is an
// agent-scope atomic (relaxed load / fetch_min); everywhere else a kernel boundary lies between writer and reader.
// Reproducibility: integers only (int64 sums, min / max boxes, confidence as sum of llrint(clamp(conf, 0, 1) * 2^30));
// integer addition commutes, so the atomics' arrival order changes nothing.
#include "scene_common.h"
#include "block_scan.h"
#include <limits.h>

#define RG_THREADS 256
#define RG_TW 64                          // tile width: one row of a tile = 16 threads x 4 pixels
#define RG_TH 32
#define RG_TPIX (RG_TW * RG_TH)
#define RG_NB 1024                        // pixels per numbering block (256 threads x 4 pixels)
#define RG_SCAN_THREADS 1024

static_assert(sizeof(InsarRegion) == 64, "InsarRegion is four 16-byte stores");
static_assert(RG_TW == INSAR_WAVE && RG_THREADS % INSAR_WAVE == 0, "one tile row per wave in the run pass of `tiles`");

// ---------------------------------------------------------------------------------------------
// tiles: union-find in LDS. lab[i] <= i always; a union links the larger root to the smaller with atomicMin and, where
// another thread got there first, goes on with the value it displaced, so no link is lost (Komura's scheme).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int rg_lds_find(int* L, int a) {
  for (;;) {
    const int p = __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p >= a) return a;
    a = p;
  }
}
__device__ __forceinline__ void rg_lds_union(int* L, int a, int b) {
  for (;;) {                                                    // a + b strictly decreases from one round to the next
    a = rg_lds_find(L, a);
    b = rg_lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;
    a = old;
  }
}

__global__ void __launch_bounds__(RG_THREADS)
regions_tile_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ conf, float min_conf, int H, int W, int ntx,
                    int conn8, int vec, int* __restrict__ parent, int* __restrict__ area) {
  __shared__ int lab[RG_TPIX];
  __shared__ uint8_t cls[RG_TPIX];
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int y0 = ty * RG_TH, x0 = tx * RG_TW;
  const int64_t npix = (int64_t)H * W;
  for (int q = threadIdx.x; q < RG_TPIX / 4; q += RG_THREADS) {
    const int ly = q / (RG_TW / 4), lx = (q % (RG_TW / 4)) * 4;
    const int gy = y0 + ly, gx = x0 + lx;
    int c[4] = {0, 0, 0, 0};
    if (gy < H && gx < W) {
      const int64_t g = (int64_t)gy * W + gx;
      const int64_t row_end = (int64_t)(gy + 1) * W;            // the scalar path must not run into the next row
      quad_load_u8(mask, g, vec ? npix : row_end, vec, 0, c);
      if (conf) {
        float f[4];
        quad_load(conf, g, vec ? npix : row_end, vec, 0.f, f);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!(f[j] >= min_conf)) c[j] = 0;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cls[q * 4 + j] = (uint8_t)c[j];
  }
  __syncthreads();
  // horizontal links without atomics: i = tid + 256 k puts one tile row on one wave (RG_TW == INSAR_WAVE, lane == column),
  // so a ballot of "same class as my left neighbour" gives every pixel the first column of its run, its initial label
  for (int i = threadIdx.x; i < RG_TPIX; i += RG_THREADS) {
    const uint8_t c = cls[i];
    const int lx = i & (RG_TW - 1);
    const unsigned long long linked = __ballot(c && lx > 0 && cls[i - 1] == c);
    const unsigned long long starts = ~linked & ((2ull << lx) - 1ull);          // bit 0 is always set
    lab[i] = i - lx + (63 - __clzll((long long)starts));
  }
  __syncthreads();
  // vertical and diagonal links, only those that the runs do not already imply: `up` is implied where the left neighbours of
  // both pixels continue the two runs (the pair further left makes the link); with `up` in the class the diagonals hang on
  // its run; up-left is implied where the left neighbour is in the class (its `up`)
  for (int i = threadIdx.x; i < RG_TPIX; i += RG_THREADS) {
    const uint8_t c = cls[i];
    if (!c || i < RG_TW) continue;
    const int lx = i & (RG_TW - 1);
    const bool left = lx > 0 && cls[i - 1] == c;
    if (cls[i - RG_TW] == c) {
      if (!(left && cls[i - RG_TW - 1] == c)) rg_lds_union(lab, i, i - RG_TW);
    } else if (conn8) {
      if (lx > 0 && !left && cls[i - RG_TW - 1] == c) rg_lds_union(lab, i, i - RG_TW - 1);
      if (lx < RG_TW - 1 && cls[i - RG_TW + 1] == c) rg_lds_union(lab, i, i - RG_TW + 1);
    }
  }
  __syncthreads();
  const int zero[4] = {0, 0, 0, 0};
  for (int q = threadIdx.x; q < RG_TPIX / 4; q += RG_THREADS) {
    const int ly = q / (RG_TW / 4), lx = (q % (RG_TW / 4)) * 4;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    int out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = cls[q * 4 + j] ? rg_lds_find(lab, q * 4 + j) : -1;
      out[j] = r < 0 ? -1 : (y0 + r / RG_TW) * W + x0 + (r & (RG_TW - 1));       // < H * W < 2^31
    }
    const int64_t g = (int64_t)gy * W + gx;
    const int64_t lim = vec ? npix : (int64_t)(gy + 1) * W;
    quad_store(parent, g, lim, vec, out);
    quad_store(area, g, lim, vec, zero);
  }
}

// ---------------------------------------------------------------------------------------------
// merge: the same union on the global parent array, every access an agent-scope atomic. Work items: the pixels of the
// first row of every tile row but the top one (neighbours up, up-left, up-right), then the pixels either side of every
// vertical tile border (left; up-left and up-right where the row above belongs to the same tile row).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int rg_ag_find(int* P, int a) {
  for (;;) {
    const int p = agent_load(P + a);
    if (p >= a) return a;
    a = p;
  }
}
__device__ __forceinline__ void rg_ag_union(int* P, int a, int b) {
  for (;;) {
    a = rg_ag_find(P, a);
    b = rg_ag_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}
// pixels a and b (b inside the scene by construction): same class, both foreground (parent >= 0: the confidence threshold
// was applied by `tiles`)
__device__ __forceinline__ void rg_try_union(const uint8_t* __restrict__ mask, int* P, int a, int b) {
  if (mask[a] != mask[b]) return;
  if (agent_load(P + a) < 0 || agent_load(P + b) < 0) return;
  rg_ag_union(P, a, b);
}

__global__ void __launch_bounds__(RG_THREADS)
regions_merge_kernel(const uint8_t* __restrict__ mask, int H, int W, int nty, int ntx, int conn8, int* parent) {
  const int64_t nrow = (int64_t)(nty - 1) * W, ncol = (int64_t)(ntx - 1) * H;
  for (int64_t t = blockIdx.x * (int64_t)RG_THREADS + threadIdx.x; t < nrow + ncol; t += (int64_t)gridDim.x * RG_THREADS) {
    if (t < nrow) {                                                      // nrow + ncol < H * W < 2^31: 32-bit divisions
      const int y = (int)((uint32_t)t / (uint32_t)W + 1) * RG_TH, x = (int)((uint32_t)t % (uint32_t)W);
      const int a = y * W + x;
      if (mask[a] == 0) continue;
      rg_try_union(mask, parent, a, a - W);
      if (conn8) {
        if (x > 0) rg_try_union(mask, parent, a, a - W - 1);
        if (x + 1 < W) rg_try_union(mask, parent, a, a - W + 1);
      }
    } else {
      const uint32_t u = (uint32_t)(t - nrow);
      const int y = (int)(u % (uint32_t)H), x = (int)(u / (uint32_t)H + 1) * RG_TW;          // x: first column of a tile, x - 1: last of its neighbour
      const int a = y * W + x;
      rg_try_union(mask, parent, a, a - 1);
      if (conn8 && (y % RG_TH) != 0) {                                  // first rows of a tile row: done by the items above
        rg_try_union(mask, parent, a, a - W - 1);
        rg_try_union(mask, parent, a - 1, a - W);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// flatten: parent[i] <- root(i), area[root] += 1. Plain accesses: a concurrent flatten of another pixel can only replace a
// parent by its root, which is still an ancestor. Threads whose four pixels share a root count them once; lanes of a wave
// whose slots share a root combine over the run before one atomic.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RG_THREADS)
regions_flatten_kernel(int* parent, int* __restrict__ area, int64_t npix, int vec) {
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q0 = blockIdx.x * (int64_t)RG_THREADS; q0 < nquads; q0 += (int64_t)gridDim.x * RG_THREADS) {
    const int64_t q = q0 + threadIdx.x;                          // the loop bound is uniform over the block: shuffles below
    int r[4] = {-1, -1, -1, -1}, cnt[4];
    if (q < nquads) {
      quad_load(parent, q << 2, npix, vec, -1, r);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int a = r[j];
        if (a < 0) continue;
        for (;;) { const int p = parent[a]; if (p >= a) break; a = p; }
        r[j] = a;
      }
      quad_store(parent, q << 2, npix, vec, r);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[j] = r[j] >= 0;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (r[j] == r[j - 1]) { cnt[j] += cnt[j - 1]; cnt[j - 1] = 0; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = cnt[j] > 0 ? r[j] : -1;
      if (__ballot(key >= 0) == 0) continue;
      const WaveRuns runs = wave_runs(key);
      const int total = wave_run_reduce(runs, cnt[j], WaveAdd());
      if (runs.head && key >= 0) atomicAdd(area + key, total);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// count / scan / number: ids 1..N in ascending root order by a three-launch prefix sum over blocks of RG_NB pixels.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RG_THREADS)
regions_count_kernel(const int* __restrict__ parent, const int* __restrict__ area, int64_t npix, int64_t min_area, int vec,
                     int* __restrict__ counts, InsarRegion* __restrict__ table, int max_regions) {
  __shared__ int wsum[RG_THREADS / INSAR_WAVE];
  const int64_t i = (int64_t)blockIdx.x * RG_NB + threadIdx.x * 4;
  int p[4], a[4], c = 0;
  quad_load(parent, i, npix, vec && i < npix, -1, p);
  quad_load(area, i, npix, vec && i < npix, 0, a);
#pragma unroll
  for (int j = 0; j < 4; ++j) c += (i + j < npix && p[j] == i + j && (int64_t)a[j] >= min_area);
  int total;
  block_prefix_sum<RG_THREADS>(c, wsum, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
  // the table's records (the header is written by the scan): empty sums, an empty box
  int4* t4 = reinterpret_cast<int4*>(table + 1);
  for (int64_t r = blockIdx.x * (int64_t)RG_THREADS + threadIdx.x; r < max_regions; r += (int64_t)gridDim.x * RG_THREADS) {
    t4[4 * r + 0] = make_int4(0, 0, 0, 0);
    t4[4 * r + 1] = make_int4(0, 0, 0, 0);
    t4[4 * r + 2] = make_int4(INT_MAX, INT_MAX, 0, 0);
    t4[4 * r + 3] = make_int4(-1, 0, 0, 0);
  }
}

__global__ void __launch_bounds__(RG_SCAN_THREADS)
regions_scan_kernel(int* __restrict__ counts, int nblk, InsarRegion* __restrict__ table) {
  __shared__ int wsum[RG_SCAN_THREADS / INSAR_WAVE];
  const int carry = block_scan_array<RG_SCAN_THREADS>(counts, nblk, wsum);
  if (threadIdx.x < 4) {                                         // header record: {N, 0, ...}
    int4 h = make_int4(0, 0, 0, 0);
    if (threadIdx.x == 0) h.x = carry;
    reinterpret_cast<int4*>(table)[threadIdx.x] = h;
  }
}

__global__ void __launch_bounds__(RG_THREADS)
regions_number_kernel(const int* __restrict__ parent, int* __restrict__ area, const uint8_t* __restrict__ mask, int64_t npix,
                      int64_t min_area, int vec, const int* __restrict__ counts, InsarRegion* __restrict__ table,
                      int max_regions) {
  __shared__ int wsum[RG_THREADS / INSAR_WAVE];
  const int64_t i = (int64_t)blockIdx.x * RG_NB + threadIdx.x * 4;
  const bool v4 = vec && i < npix;
  int p[4], a[4], c = 0;
  bool root[4], keep[4];
  quad_load(parent, i, npix, v4, -1, p);
  quad_load(area, i, npix, v4, 0, a);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    root[j] = i + j < npix && p[j] == i + j;
    keep[j] = root[j] && (int64_t)a[j] >= min_area;
    c += keep[j];
  }
  int total;
  int id = counts[blockIdx.x] + block_prefix_sum<RG_THREADS>(c, wsum, &total);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!root[j]) continue;                                      // other pixels keep the 0 that `tiles` wrote
    a[j] = 0;
    if (keep[j]) {
      a[j] = ++id;
      if (id <= max_regions) *reinterpret_cast<int2*>(&table[id].root) = make_int2((int)(i + j), (int)mask[i + j]);
    }
  }
  if (i < npix) quad_store(area, i, npix, v4, a);
}

// ---------------------------------------------------------------------------------------------
// relabel: labels[i] = ids[root(i)], mask_out[i] = labels[i] ? mask[i] : 0, and the statistics of the kept regions.
// A thread merges those of its four pixels that share a label; lanes of a wave combine over runs of a label; the first
// lane of a run issues the atomics. Ids above max_regions write labels (scene-sized) but never the table.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RG_THREADS)
regions_relabel_kernel(const int* __restrict__ parent, const int* __restrict__ ids, const uint8_t* __restrict__ mask,
                       const float* __restrict__ conf, int64_t npix, int W, int vec, int* __restrict__ labels,
                       uint8_t* __restrict__ mask_out, InsarRegion* __restrict__ table, int max_regions) {
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q0 = blockIdx.x * (int64_t)RG_THREADS; q0 < nquads; q0 += (int64_t)gridDim.x * RG_THREADS) {
    const int64_t q = q0 + threadIdx.x;
    int id[4] = {0, 0, 0, 0}, cnt[4], y0[4], y1[4], x0[4], x1[4];
    long long sy[4], sx[4], sc[4];
    if (q < nquads) {
      const int64_t i = q << 2;
      int p[4], m[4];
      float f[4] = {0.f, 0.f, 0.f, 0.f};
      quad_load(parent, i, npix, vec, -1, p);
      quad_load_u8(mask, i, npix, vec, 0, m);
      if (conf) quad_load(conf, i, npix, vec, 0.f, f);
      int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W) - 1;      // i < 2^31
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        id[j] = p[j] >= 0 ? ids[p[j]] : 0;
        if (!id[j]) m[j] = 0;
        if (++x == W) { x = 0; ++y; }
        y0[j] = y; y1[j] = y + 1; x0[j] = x; x1[j] = x + 1;
        sy[j] = y; sx[j] = x;
        sc[j] = conf ? __float2ll_rn(fminf(fmaxf(f[j], 0.f), 1.f) * 1073741824.0f) : 0;
      }
      quad_store(labels, i, npix, vec, id);
      quad_store_u8(mask_out, i, npix, vec, m);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[j] = id[j] > 0;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (id[j] > 0 && id[j] == id[j - 1]) {
        cnt[j] += cnt[j - 1]; sy[j] += sy[j - 1]; sx[j] += sx[j - 1]; sc[j] += sc[j - 1];
        y0[j] = min(y0[j], y0[j - 1]); y1[j] = max(y1[j], y1[j - 1]);
        x0[j] = min(x0[j], x0[j - 1]); x1[j] = max(x1[j], x1[j - 1]);
        cnt[j - 1] = 0;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = cnt[j] > 0 ? id[j] : 0;
      if (__ballot(key > 0) == 0) continue;
      const WaveRuns runs = wave_runs(key);
      const long long n = wave_run_reduce(runs, (long long)cnt[j], WaveAdd());
      const long long ty = wave_run_reduce(runs, sy[j], WaveAdd());
      const long long tx = wave_run_reduce(runs, sx[j], WaveAdd());
      const long long tc = conf ? wave_run_reduce(runs, sc[j], WaveAdd()) : 0;
      const int by0 = wave_run_reduce(runs, y0[j], WaveMin()), by1 = wave_run_reduce(runs, y1[j], WaveMax());
      const int bx0 = wave_run_reduce(runs, x0[j], WaveMin()), bx1 = wave_run_reduce(runs, x1[j], WaveMax());
      if (runs.head && key > 0 && key <= max_regions) {
        InsarRegion* r = table + key;
        atomicAdd(reinterpret_cast<unsigned long long*>(&r->area), (unsigned long long)n);
        atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_y), (unsigned long long)ty);
        atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_x), (unsigned long long)tx);
        if (conf) atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_conf), (unsigned long long)tc);
        atomicMin(&r->y0, by0); atomicMin(&r->x0, bx0);
        atomicMax(&r->y1, by1); atomicMax(&r->x1, bx1);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side: scratch layout and the five entry points
// ---------------------------------------------------------------------------------------------
struct RgLayout { int64_t npix, seg, nblk, bytes; int nty, ntx; };

static int regions_layout(const char* who, int32_t H, int32_t W, RgLayout* L) {
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  const int64_t npix = (int64_t)H * W;
  if (npix >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^31 pixels or more", who, H, W);
  L->npix = npix;
  L->seg = insar_align16(npix * 4);
  L->nblk = (npix + RG_NB - 1) / RG_NB;
  L->bytes = 2 * L->seg + insar_align16(L->nblk * 4);
  L->nty = (H + RG_TH - 1) / RG_TH;
  L->ntx = (W + RG_TW - 1) / RG_TW;
  return INSAR_OK;
}
static int regions_check_scratch(const char* who, const void* scratch) {
  if (!scratch) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (!insar_aligned16(scratch)) INSAR_FAIL(INSAR_E_ALIGN, "%s: scratch not 16-byte aligned", who);
  return INSAR_OK;
}
static int regions_check_conn(const char* who, int32_t connectivity) {
  if (connectivity != 4 && connectivity != 8) INSAR_FAIL(INSAR_E_ARG, "%s: connectivity %d (4 or 8)", who, connectivity);
  return INSAR_OK;
}
static int regions_check_table(const char* who, const void* table, int32_t max_regions) {
  if (max_regions < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d < 1", who, max_regions);
  if (!table) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (!insar_aligned16(table)) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 16-byte aligned", who);
  return INSAR_OK;
}
static inline int* rg_parent(void* scratch) { return (int*)scratch; }
static inline int* rg_area(void* scratch, const RgLayout& L) { return (int*)((char*)scratch + L.seg); }
static inline int* rg_counts(void* scratch, const RgLayout& L) { return (int*)((char*)scratch + 2 * L.seg); }

extern "C" int insar_regions_scratch_bytes(int32_t H, int32_t W, int32_t max_regions, int64_t* scratch_bytes,
                                           int64_t* table_bytes) {
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "insar_regions_scratch_bytes: null pointer");
  RgLayout L;
  if (int rc = regions_layout("insar_regions_scratch_bytes", H, W, &L)) return rc;
  if (max_regions < 1) INSAR_FAIL(INSAR_E_SHAPE, "insar_regions_scratch_bytes: max_regions %d < 1", max_regions);
  *scratch_bytes = L.bytes;
  *table_bytes = (int64_t)sizeof(InsarRegion) * ((int64_t)max_regions + 1);
  return INSAR_OK;
}

extern "C" int insar_regions_tiles(const uint8_t* mask, const float* conf, float min_conf, int32_t H, int32_t W,
                                   int32_t connectivity, void* scratch, void* stream) {
  const char* who = "insar_regions_tiles";
  if (!mask) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  RgLayout L;
  if (int rc = regions_layout(who, H, W, &L)) return rc;
  if (int rc = regions_check_conn(who, connectivity)) return rc;
  if (int rc = regions_check_scratch(who, scratch)) return rc;
  if (((uintptr_t)conf) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: conf not 4-byte aligned", who);
  const int vec = (W % 4 == 0) && ((((uintptr_t)mask) & 3u) == 0) && insar_aligned16(conf);
  hipLaunchKernelGGL(regions_tile_kernel, dim3((unsigned)((int64_t)L.nty * L.ntx)), dim3(RG_THREADS), 0, (hipStream_t)stream, mask,
                     conf, min_conf, H, W, L.ntx, connectivity == 8, vec, rg_parent(scratch), rg_area(scratch, L));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_regions_merge(const uint8_t* mask, int32_t H, int32_t W, int32_t connectivity, void* scratch,
                                   void* stream) {
  const char* who = "insar_regions_merge";
  if (!mask) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  RgLayout L;
  if (int rc = regions_layout(who, H, W, &L)) return rc;
  if (int rc = regions_check_conn(who, connectivity)) return rc;
  if (int rc = regions_check_scratch(who, scratch)) return rc;
  const int64_t work = (int64_t)(L.nty - 1) * W + (int64_t)(L.ntx - 1) * H;
  hipLaunchKernelGGL(regions_merge_kernel, dim3(insar_grid_cap((work + RG_THREADS - 1) / RG_THREADS)), dim3(RG_THREADS), 0,
                     (hipStream_t)stream, mask, H, W, L.nty, L.ntx, connectivity == 8, rg_parent(scratch));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_regions_flatten(int32_t H, int32_t W, void* scratch, void* stream) {
  const char* who = "insar_regions_flatten";
  RgLayout L;
  if (int rc = regions_layout(who, H, W, &L)) return rc;
  if (int rc = regions_check_scratch(who, scratch)) return rc;
  const int vec = L.npix % 4 == 0;
  hipLaunchKernelGGL(regions_flatten_kernel, dim3(insar_grid_cap((L.npix / 4 + RG_THREADS) / RG_THREADS)), dim3(RG_THREADS), 0,
                     (hipStream_t)stream, rg_parent(scratch), rg_area(scratch, L), L.npix, vec);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_regions_number(const uint8_t* mask, int32_t H, int32_t W, int64_t min_area, int32_t max_regions,
                                    void* scratch, void* table, void* stream) {
  const char* who = "insar_regions_number";
  if (!mask) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  RgLayout L;
  if (int rc = regions_layout(who, H, W, &L)) return rc;
  if (min_area < 1) INSAR_FAIL(INSAR_E_ARG, "%s: min_area %lld < 1", who, (long long)min_area);
  if (int rc = regions_check_table(who, table, max_regions)) return rc;
  if (int rc = regions_check_scratch(who, scratch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int vec = L.npix % 4 == 0;
  int *parent = rg_parent(scratch), *area = rg_area(scratch, L), *counts = rg_counts(scratch, L);
  InsarRegion* t = (InsarRegion*)table;
  hipLaunchKernelGGL(regions_count_kernel, dim3((unsigned)L.nblk), dim3(RG_THREADS), 0, s, parent, area, L.npix, min_area, vec,
                     counts, t, max_regions);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(regions_scan_kernel, dim3(1), dim3(RG_SCAN_THREADS), 0, s, counts, (int)L.nblk, t);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(regions_number_kernel, dim3((unsigned)L.nblk), dim3(RG_THREADS), 0, s, parent, area, mask, L.npix, min_area,
                     vec, counts, t, max_regions);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_regions_relabel(const uint8_t* mask, const float* conf, int32_t H, int32_t W, int32_t max_regions,
                                     void* scratch, void* table, int32_t* labels, uint8_t* mask_out, void* stream) {
  const char* who = "insar_regions_relabel";
  if (!mask || !labels || !mask_out) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  RgLayout L;
  if (int rc = regions_layout(who, H, W, &L)) return rc;
  if (int rc = regions_check_table(who, table, max_regions)) return rc;
  if (int rc = regions_check_scratch(who, scratch)) return rc;
  if ((((uintptr_t)conf) | ((uintptr_t)labels)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: buffer not 4-byte aligned", who);
  const int vec = (L.npix % 4 == 0) && insar_aligned16(conf) && insar_aligned16(labels) &&
                  (((((uintptr_t)mask) | ((uintptr_t)mask_out)) & 3u) == 0);
  hipLaunchKernelGGL(regions_relabel_kernel, dim3(insar_grid_cap((L.npix / 4 + RG_THREADS) / RG_THREADS)), dim3(RG_THREADS), 0,
                     (hipStream_t)stream, rg_parent(scratch), rg_area(scratch, L), mask, conf, L.npix, W, vec, labels, mask_out,
                     (InsarRegion*)table, max_regions);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
