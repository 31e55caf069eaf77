// Sieving class maps: regions below a per-class area threshold are absorbed by their largest neighbour, whatever its class, so
// specks vanish and holes fill by one rule. Integers only; the rule is DESIGN.md's "Sieving class maps", tests/sieve_ref.py
// restates it in numpy. The regions themselves come from regions.hip (the insar_regions_* phases on a remapped copy of the
// class map in which every class is foreground); this file adds the region adjacency table and the sieve on top of it.
//
//   remap    every class -> a code in 1..255, the void value -> 0 (background for the labelling); the control words are zeroed
//   pairs    clear     zeroes the pair table and the header of the pair list
//            pairs     every pixel looks at its right and lower neighbour; where both labels are positive and differ,
//                      table[(min, max)] += 1: the number of pixel edges two regions share
//            compact   the table's slots as the pair list {a, b, edges} behind the header {n_pairs, overflow}
//   rounds   init      (first round only) up / nxt / area / cls / best of every region from the region table
//            per round, over the pair list and the region table only: best (atomic max of the neighbour's packed key into
//            every small piece), decide (nxt[u] = best(u) unless the pair is mutual and u has the greater key; one count per
//            merge), compress (up[r] <- the end of its nxt chain, areas added into the surviving roots, best words reset)
//   apply    out[p] = cls[up[label[p]]], void copied through; optionally the map of changed pixels; the counts
//
// No work-group ever waits on another: the phases are ordered by kernel boundaries on the caller's stream. The chase in
// `compress` follows nxt, along which the key (area, -id) strictly rises except inside a mutual pair, which `decide` has
// resolved: it ends. Visibility: the pair table, the overflow word, the best words, the round counters and (in compress) the
// areas are shared between work-groups of one launch, so every access to them in those launches is an agent-scope atomic.
// The pair table, its clear and compact launches and the aggregation of a thread's eight neighbour pairs before the atomics
// (pair_fold_insert: a wave that sees no border at all leaves after one ballot) are pair_table.h's.
// Reproducibility: integer sums and maxima commute; which slot a pair lands in, and the order of the pair list, depend on
// arrival order, but every result taken from them is a sum or a maximum under a total order.
#include "pair_table.h"
#include <limits.h>

#define SV_THREADS 256
#define SV_MAX_ROUNDS 4096
#define SV_MAX_REGIONS (1 << 30)
#define SV_CTRL_WORDS 8                   // n_pairs, overflow, regions, bad classes, changed pixels, absorbed, 2 spare; then one per round

struct SvPair { int a, b; long long edges; };
static_assert(sizeof(SvPair) == 16, "a pair is one record of pair_table_compact_kernel");
static_assert(sizeof(InsarRegion) == 64, "InsarRegion is four 16-byte stores");

enum { SV_NPAIRS = 0, SV_OVERFLOW = 1, SV_REGIONS = 2, SV_BADCLS = 3, SV_CHANGED = 4, SV_ABSORBED = 5 };

// ---------------------------------------------------------------------------------------------
// remap
// ---------------------------------------------------------------------------------------------
// class c -> a code in 1..255 that keeps classes apart: c + 1 below the void value (or without one), c above it; void -> 0
__global__ void __launch_bounds__(SV_THREADS)
sieve_remap_kernel(const uint8_t* __restrict__ mask, int64_t npix, int vec, int void_value, uint8_t* __restrict__ remap,
                   int4* __restrict__ ctrl, int ctrl_chunks) {
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < ctrl_chunks; i += SV_THREADS) ctrl[i] = make_int4(0, 0, 0, 0);
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q = blockIdx.x * (int64_t)SV_THREADS + threadIdx.x; q < nquads; q += (int64_t)gridDim.x * SV_THREADS) {
    const int64_t i = q << 2;
    int m[4];
    quad_load_u8(mask, i, npix, vec, 0, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (m[j] == void_value) m[j] = 0;
      else if (void_value < 0 || m[j] < void_value) m[j] = (m[j] + 1) & 255;      // class 255 without a void value: no code left
    }
    quad_store_u8(remap, i, npix, vec, m);
  }
}

// Without a void value 256 classes would need 257 codes: pixels of class 255 are then counted, and the host refuses the map.
// The remap launch zeroes the control words, so the count is a launch of its own; it runs only without a void value.
__global__ void __launch_bounds__(SV_THREADS)
sieve_badcls_kernel(const uint8_t* __restrict__ mask, int64_t npix, int* ctrl) {
  for (int64_t i0 = blockIdx.x * (int64_t)SV_THREADS; i0 < npix; i0 += (int64_t)gridDim.x * SV_THREADS) {
    const int64_t i = i0 + threadIdx.x;
    wave_count(ctrl + SV_BADCLS, i < npix && mask[i] == 255);
  }
}

// ---------------------------------------------------------------------------------------------
// pairs
// ---------------------------------------------------------------------------------------------
// (min, max) of two different region labels in 1..max_label, else 0 (the empty slot: max >= 2 keeps a key off it)
__device__ __forceinline__ unsigned long long sv_key(int a, int b, int max_label) {
  if (a == b || a <= 0 || b <= 0 || a > max_label || b > max_label) return 0ull;
  return ((unsigned long long)(uint32_t)min(a, b) << 32) | (unsigned long long)(uint32_t)max(a, b);
}

template <bool VEC>
__global__ void __launch_bounds__(SV_THREADS)
sieve_pairs_kernel(const int* __restrict__ labels, int H, int W, int max_label, int* hdr, PairSlot* slots, unsigned int mask) {
  const int64_t npix = (int64_t)H * W, nquads = (npix + 3) >> 2;
  for (int64_t q0 = blockIdx.x * (int64_t)SV_THREADS; q0 < nquads; q0 += (int64_t)gridDim.x * SV_THREADS) {
    const int64_t q = q0 + threadIdx.x;                            // the loop bound is uniform over the block: shuffles below
    unsigned long long k[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (q < nquads) {
      const int64_t i = q << 2;
      int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);      // i < 2^31
      if (VEC) {                                                   // W % 4 == 0: the quad lies in one row
        int v[4], d[4] = {0, 0, 0, 0};
        quad_load(labels, i, npix, true, 0, v);
        if (y + 1 < H) quad_load(labels, i + W, npix, true, 0, d);
        const int r = x + 4 < W ? labels[i + 4] : 0;
        k[0] = sv_key(v[0], v[1], max_label); k[1] = sv_key(v[1], v[2], max_label);
        k[2] = sv_key(v[2], v[3], max_label); k[3] = sv_key(v[3], r, max_label);
#pragma unroll
        for (int j = 0; j < 4; ++j) k[4 + j] = sv_key(v[j], d[j], max_label);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (i + j < npix) {
            const int l = labels[i + j];
            if (l > 0) {
              k[j] = sv_key(l, x + 1 < W ? labels[i + j + 1] : 0, max_label);
              k[4 + j] = sv_key(l, y + 1 < H ? labels[i + j + W] : 0, max_label);
            }
          }
          if (++x == W) { x = 0; ++y; }
        }
      }
    }
    int c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = k[j] != 0ull;
    pair_fold_insert<8, WaveAdd>(hdr + SV_OVERFLOW, slots, mask, k, c);
  }
}

// ---------------------------------------------------------------------------------------------
// rounds: over the pair list and the region table. up[a] is the root of region a's piece at the start of the round.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long sv_pack(int area, int id) {         // key (area, -id); never 0: area >= 1
  return ((unsigned long long)(uint32_t)area << 32) | (unsigned long long)(uint32_t)(0x7fffffff - id);
}
__device__ __forceinline__ int sv_id(unsigned long long packed) { return 0x7fffffff - (int)(uint32_t)packed; }
__device__ __forceinline__ int sv_pair_count(const int* hdr, int64_t max_pairs) {
  const int64_t n = hdr[SV_NPAIRS];                               // written by `compact`, a launch before
  return (int)(n < max_pairs ? n : max_pairs);
}

__global__ void __launch_bounds__(SV_THREADS)
sieve_init_kernel(const InsarRegion* __restrict__ table, const uint8_t* __restrict__ mask, const int* __restrict__ hdr, int max_regions,
                  int* __restrict__ ctrl, int* __restrict__ up, int* __restrict__ nxt, int* __restrict__ area, int* __restrict__ cls,
                  unsigned long long* __restrict__ best) {
  const int64_t N = table[0].area;                                // the TRUE count, which may exceed max_regions
  const int n = (int)(N < max_regions ? N : max_regions);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl[SV_NPAIRS] = hdr[SV_NPAIRS];
    ctrl[SV_OVERFLOW] = hdr[SV_OVERFLOW];
    ctrl[SV_REGIONS] = (int)(N < INT_MAX ? N : INT_MAX);
  }
  for (int r = blockIdx.x * SV_THREADS + threadIdx.x; r <= n; r += gridDim.x * SV_THREADS) {
    up[r] = r;
    nxt[r] = r;
    area[r] = r ? (int)table[r].area : 0;
    cls[r] = r ? (int)mask[table[r].root] : 0;
    best[r] = 0ull;
  }
}

__device__ __forceinline__ int sv_region_count(const int* ctrl, int max_regions) {
  const int n = ctrl[SV_REGIONS];                                 // written by `init`, a launch before
  return n < max_regions ? n : max_regions;
}

__global__ void __launch_bounds__(SV_THREADS)
sieve_best_kernel(const SvPair* __restrict__ pairs, const int* __restrict__ hdr, int64_t max_pairs, const int* __restrict__ up,
                  const int* __restrict__ area, const int* __restrict__ cls, const int* __restrict__ thr, unsigned long long* best) {
  const int n = sv_pair_count(hdr, max_pairs);
  for (int t = blockIdx.x * SV_THREADS + threadIdx.x; t < n; t += gridDim.x * SV_THREADS) {
    const int2 e = *reinterpret_cast<const int2*>(pairs + t);
    const int u = up[e.x], v = up[e.y];
    if (u == v) continue;
    const int au = area[u], av = area[v];
    if (au < thr[cls[u] & 255]) __hip_atomic_fetch_max(best + u, sv_pack(av, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (av < thr[cls[v] & 255]) __hip_atomic_fetch_max(best + v, sv_pack(au, u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// a small piece u with a neighbour merges into best(u), unless best(best(u)) == u and key(u) > key(best(u))
__global__ void __launch_bounds__(SV_THREADS)
sieve_decide_kernel(int* ctrl, int max_regions, const int* __restrict__ up, const int* __restrict__ area,
                    const unsigned long long* __restrict__ best, int* __restrict__ nxt, int round) {
  const int n = sv_region_count(ctrl, max_regions);
  for (int r0 = blockIdx.x * SV_THREADS; r0 <= n; r0 += gridDim.x * SV_THREADS) {
    const int r = r0 + threadIdx.x;
    bool merged = false;
    if (r >= 1 && r <= n && up[r] == r) {
      const unsigned long long b = best[r];
      if (b != 0ull) {
        const int v = sv_id(b);
        const unsigned long long bv = best[v];
        const bool stays = bv != 0ull && sv_id(bv) == r && sv_pack(area[r], r) > sv_pack(area[v], v);
        if (!stays) { nxt[r] = v; merged = true; }
      }
    }
    wave_count(ctrl + SV_CTRL_WORDS + round, merged);
  }
}

__global__ void __launch_bounds__(SV_THREADS)
sieve_compress_kernel(const int* __restrict__ ctrl, int max_regions, int* __restrict__ up, const int* __restrict__ nxt, int* area,
                      unsigned long long* __restrict__ best) {
  const int n = sv_region_count(ctrl, max_regions);
  for (int r = blockIdx.x * SV_THREADS + threadIdx.x; r <= n; r += gridDim.x * SV_THREADS) {
    if (r < 1) continue;
    const int x = up[r];                                           // up[r], best[r] and a merged root's area[r] are thread r's alone
    int y = x;
    for (;;) { const int m = nxt[y]; if (m == y) break; y = m; }
    up[r] = y;
    best[r] = 0ull;
    if (x == r && y != r)                                          // a root of this round that merged: only surviving roots receive
      __hip_atomic_fetch_add(area + y, area[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SV_THREADS)
sieve_apply_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ mask, int64_t npix, int vec, int max_regions, int* ctrl,
                   const int* __restrict__ up, const int* __restrict__ cls, uint8_t* __restrict__ out, uint8_t* __restrict__ changed) {
  const int n = sv_region_count(ctrl, max_regions);
  for (int r0 = blockIdx.x * SV_THREADS; r0 <= n; r0 += gridDim.x * SV_THREADS) {
    const int r = r0 + threadIdx.x;
    wave_count(ctrl + SV_ABSORBED, r >= 1 && r <= n && up[r] != r);
  }
  const int64_t nquads = (npix + 3) >> 2;
  for (int64_t q0 = blockIdx.x * (int64_t)SV_THREADS; q0 < nquads; q0 += (int64_t)gridDim.x * SV_THREADS) {
    const int64_t q = q0 + threadIdx.x;
    int diff = 0;
    if (q < nquads) {
      const int64_t i = q << 2;
      int l[4], m[4], o[4];
      quad_load(labels, i, npix, vec, 0, l);
      quad_load_u8(mask, i, npix, vec, 0, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j > 0 && l[j] == l[j - 1]) o[j] = l[j] > 0 && l[j] <= n ? o[j - 1] : m[j];
        else o[j] = l[j] > 0 && l[j] <= n ? cls[up[l[j]]] : m[j];
        diff += o[j] != m[j];                                      // past npix l, m and o are 0
      }
      // The two stores stay packed by hand. As two quad_store_u8 calls the `changed` map gets a branch of its own: the kernel
      // is 23 instructions longer and was measured at 30 us instead of 26 us on a 4096 x 4096 map of large regions
      // (profiles/pair_table_refactor_ab.txt, part 3).
      if (vec) {
        *reinterpret_cast<uint32_t*>(out + i) = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
        if (changed)
          *reinterpret_cast<uint32_t*>(changed + i) = (uint32_t)(o[0] != m[0]) | ((uint32_t)(o[1] != m[1]) << 8) |
                                                       ((uint32_t)(o[2] != m[2]) << 16) | ((uint32_t)(o[3] != m[3]) << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i + j < npix) {
            out[i + j] = (uint8_t)o[j];
            if (changed) changed[i + j] = (uint8_t)(o[j] != m[j]);
          }
      }
    }
    wave_tally(ctrl + SV_CHANGED, diff);
  }
}

// ---------------------------------------------------------------------------------------------
// host side: scratch layout and the entry points
// ---------------------------------------------------------------------------------------------
struct SvLayout {
  int64_t npix, cap, ctrl_words, regions;
  int64_t off_ctrl, off_up, off_nxt, off_area, off_cls, off_best, off_hdr, off_pairs, off_slots, bytes;
};

static int sieve_layout(const char* who, int32_t H, int32_t W, int32_t max_regions, int64_t max_pairs, int32_t max_rounds, SvLayout* L) {
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  const int64_t npix = (int64_t)H * W;
  if (npix >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^31 pixels or more", who, H, W);
  if (max_regions < 1 || max_regions > SV_MAX_REGIONS) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d outside 1..%d", who, max_regions, SV_MAX_REGIONS);
  if (int rc = pair_table_capacity(who, max_pairs, &L->cap)) return rc;
  if (max_rounds < 1 || max_rounds > SV_MAX_ROUNDS)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_rounds %d outside 1..%d", who, max_rounds, SV_MAX_ROUNDS);
  L->npix = npix;
  L->ctrl_words = insar_align16((SV_CTRL_WORDS + (int64_t)max_rounds) * 4) / 4;
  L->regions = (int64_t)max_regions + 1;
  const int64_t seg = insar_align16(L->regions * 4);
  L->off_ctrl = insar_align16(npix);                                 // the remapped class map comes first
  L->off_up = L->off_ctrl + L->ctrl_words * 4;                    // directly behind the control words: one read-back takes both
  L->off_nxt = L->off_up + seg;
  L->off_area = L->off_nxt + seg;
  L->off_cls = L->off_area + seg;
  L->off_best = L->off_cls + seg;
  L->off_hdr = L->off_best + 2 * seg;
  L->off_pairs = L->off_hdr + 16;
  L->off_slots = L->off_pairs + max_pairs * (int64_t)sizeof(SvPair);
  L->bytes = L->off_slots + L->cap * (int64_t)sizeof(PairSlot);
  return INSAR_OK;
}

extern "C" int insar_sieve_scratch_bytes(int32_t H, int32_t W, int32_t max_regions, int64_t max_pairs, int32_t max_rounds,
                                         int64_t* scratch_bytes, int64_t* ctrl_offset, int64_t* ctrl_bytes, int64_t* pairs_offset) {
  const char* who = "insar_sieve_scratch_bytes";
  if (!scratch_bytes || !ctrl_offset || !ctrl_bytes || !pairs_offset) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  SvLayout L;
  if (int rc = sieve_layout(who, H, W, max_regions, max_pairs, max_rounds, &L)) return rc;
  *scratch_bytes = L.bytes;
  *ctrl_offset = L.off_ctrl;
  *ctrl_bytes = L.ctrl_words * 4;
  *pairs_offset = L.off_hdr;
  return INSAR_OK;
}

extern "C" int insar_sieve_remap(const uint8_t* mask, int32_t H, int32_t W, int32_t void_value, int32_t max_regions, int64_t max_pairs,
                                 int32_t max_rounds, void* scratch, void* stream) {
  const char* who = "insar_sieve_remap";
  if (int rc = scene_check_map(who, "mask", mask, 1)) return rc;
  SvLayout L;
  if (int rc = sieve_layout(who, H, W, max_regions, max_pairs, max_rounds, &L)) return rc;
  if (void_value < -1 || void_value > 255) INSAR_FAIL(INSAR_E_ARG, "%s: void_value %d outside -1..255", who, void_value);
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  int* ctrl = scratch_at<int>(scratch, L.off_ctrl);
  const int vec = (L.npix % 4 == 0) && ((((uintptr_t)mask) & 3u) == 0);
  hipLaunchKernelGGL(sieve_remap_kernel, scene_grid((L.npix + 3) / 4, SV_THREADS), dim3(SV_THREADS), 0, s, mask, L.npix, vec, (int)void_value,
                     scratch_at<uint8_t>(scratch, 0), (int4*)ctrl, (int)(L.ctrl_words / 4));
  INSAR_CHECK_LAUNCH(who);
  if (void_value < 0) {
    hipLaunchKernelGGL(sieve_badcls_kernel, scene_grid(L.npix, SV_THREADS), dim3(SV_THREADS), 0, s, mask, L.npix, ctrl);
    INSAR_CHECK_LAUNCH(who);
  }
  return INSAR_OK;
}

extern "C" int insar_sieve_pairs(const int32_t* labels, int32_t H, int32_t W, int32_t max_label, int32_t max_regions,
                                 int64_t max_pairs, int32_t max_rounds, void* scratch, void* stream) {
  const char* who = "insar_sieve_pairs";
  if (int rc = scene_check_map(who, "labels", labels, 4)) return rc;
  SvLayout L;
  if (int rc = sieve_layout(who, H, W, max_regions, max_pairs, max_rounds, &L)) return rc;
  if (max_label < 1) INSAR_FAIL(INSAR_E_ARG, "%s: max_label %d < 1", who, max_label);
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  int* hdr = scratch_at<int>(scratch, L.off_hdr);
  PairSlot* slots = scratch_at<PairSlot>(scratch, L.off_slots);
  const dim3 block(SV_THREADS), grid = scene_grid((L.npix + 3) / 4, SV_THREADS);
  const unsigned int mask = (unsigned int)(L.cap - 1);
  pair_table_clear(s, slots, L.cap, hdr, 1);
  INSAR_CHECK_LAUNCH(who);
  if (W % 4 == 0 && insar_aligned16(labels))
    hipLaunchKernelGGL(sieve_pairs_kernel<true>, grid, block, 0, s, (const int*)labels, H, W, max_label, hdr, slots, mask);
  else
    hipLaunchKernelGGL(sieve_pairs_kernel<false>, grid, block, 0, s, (const int*)labels, H, W, max_label, hdr, slots, mask);
  INSAR_CHECK_LAUNCH(who);
  pair_table_compact(s, slots, L.cap, max_pairs, hdr + SV_NPAIRS, scratch_at<SvPair>(scratch, L.off_pairs));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_sieve_rounds(const void* table, const uint8_t* mask, const int32_t* thresholds, int32_t H, int32_t W,
                                  int32_t first_round, int32_t n_rounds, int32_t max_regions, int64_t max_pairs, int32_t max_rounds,
                                  void* scratch, void* stream) {
  const char* who = "insar_sieve_rounds";
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  if (int rc = scene_check_map(who, "mask", mask, 1)) return rc;
  if (int rc = scene_check_map(who, "thresholds", thresholds, 4)) return rc;
  SvLayout L;
  if (int rc = sieve_layout(who, H, W, max_regions, max_pairs, max_rounds, &L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (first_round < 0 || n_rounds < 1 || (int64_t)first_round + n_rounds > max_rounds)
    INSAR_FAIL(INSAR_E_ARG, "%s: rounds %d..%d outside 0..%d", who, first_round, first_round + n_rounds, max_rounds);
  hipStream_t s = (hipStream_t)stream;
  int *ctrl = scratch_at<int>(scratch, L.off_ctrl), *up = scratch_at<int>(scratch, L.off_up), *nxt = scratch_at<int>(scratch, L.off_nxt);
  int *area = scratch_at<int>(scratch, L.off_area), *cls = scratch_at<int>(scratch, L.off_cls);
  const int* hdr = scratch_at<int>(scratch, L.off_hdr);
  unsigned long long* best = scratch_at<unsigned long long>(scratch, L.off_best);
  const SvPair* pairs = scratch_at<SvPair>(scratch, L.off_pairs);
  const dim3 block(SV_THREADS), pgrid = scene_grid(max_pairs, SV_THREADS), rgrid = scene_grid(L.regions, SV_THREADS);
  if (first_round == 0) {
    hipLaunchKernelGGL(sieve_init_kernel, rgrid, block, 0, s, (const InsarRegion*)table, mask, hdr, max_regions, ctrl, up, nxt, area,
                       cls, best);
    INSAR_CHECK_LAUNCH(who);
  }
  for (int r = first_round; r < first_round + n_rounds; ++r) {
    hipLaunchKernelGGL(sieve_best_kernel, pgrid, block, 0, s, pairs, hdr, max_pairs, (const int*)up, (const int*)area, (const int*)cls,
                       (const int*)thresholds, best);
    INSAR_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(sieve_decide_kernel, rgrid, block, 0, s, ctrl, max_regions, (const int*)up, (const int*)area,
                       (const unsigned long long*)best, nxt, r);
    INSAR_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(sieve_compress_kernel, rgrid, block, 0, s, (const int*)ctrl, max_regions, up, (const int*)nxt, area, best);
    INSAR_CHECK_LAUNCH(who);
  }
  return INSAR_OK;
}

extern "C" int insar_sieve_apply(const int32_t* labels, const uint8_t* mask, int32_t H, int32_t W, int32_t max_regions,
                                 int64_t max_pairs, int32_t max_rounds, void* scratch, uint8_t* out, uint8_t* changed, void* stream) {
  const char* who = "insar_sieve_apply";
  if (int rc = scene_check_map(who, "labels", labels, 4)) return rc;
  if (int rc = scene_check_map(who, "mask", mask, 1)) return rc;
  if (int rc = scene_check_map(who, "out", out, 1)) return rc;
  SvLayout L;
  if (int rc = sieve_layout(who, H, W, max_regions, max_pairs, max_rounds, &L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  const int vec = (L.npix % 4 == 0) && insar_aligned16(labels) &&
                  (((((uintptr_t)mask) | ((uintptr_t)out) | ((uintptr_t)changed)) & 3u) == 0);
  hipLaunchKernelGGL(sieve_apply_kernel, scene_grid((L.npix + 3) / 4, SV_THREADS), dim3(SV_THREADS), 0, (hipStream_t)stream, (const int*)labels, mask,
                     L.npix, vec, max_regions, scratch_at<int>(scratch, L.off_ctrl), (const int*)scratch_at<int>(scratch, L.off_up),
                     (const int*)scratch_at<int>(scratch, L.off_cls), out, changed);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
