// Region outlines: the exact pixel-edge ("crack") boundary of every region of an int32 label map [H][W], as ordered, closed
// rings of lattice vertices (exteriors with positive, holes with negative doubled area). Semantics: include/insar_hip.h.
// A boundary edge is a side (0 top, 1 right, 2 bottom, 3 left) of a labelled pixel whose neighbour across it differs; its id
// is 4 * pixel + side, its COMPACT index k the number of boundary edges with a smaller id, so "smallest id" and "smallest
// index" are the same thing and every array below is indexed by k. With E edges and L = ceil(log2 E):
//
//   edges   mark     per pixel: the 4-bit side mask; boundary edges per block of 1024 pixels
//           scan     trace_common.h: the prefix sum of the block counts; E goes to the table header, the rest of it is cleared
//           offsets  per pixel: the compact index of its first edge
//           link     per edge: successor (the turn rule), id, "the successor turns" flag; pair (succ, k) for `lead`
//   lead    trace_common.h: after L rounds of pointer doubling every edge knows the smallest edge of its ring, its leader
//   rank    cut      every ring is cut in front of its leader: pair (next, d) = (succ, 1), or (-1, 0) for the last edge
//           trace_common.h: after L rounds of list ranking d[k] is the distance from k to the last edge of its ring
//   rings   trace_common.h (count / scan / number) with OlTool: a leader is lead[k] == k; R goes to the header
//   write   scatter  per edge: position = ring start + rank; tail vertex, ring number and side go there, the corner flag of
//                    the SUCCESSOR goes to the successor's position
//           reduce   over the ordered array, where a ring is one contiguous run: area2 and box by trace_common.h's
//                    trace_reduce, the kept-vertex count with them; kept vertices per block of 256 positions
//           scan     trace_common.h: prefix sum of the kept counts; V goes to the header
//           compact  kept vertices to their final place; every ring's `start`
//
// 12 + 2 L launches, a function of E alone; how the steps are ordered and why the atomics' arrival order changes nothing:
// trace_common.h. Integers only. A round moves 24 bytes per edge: 8 read in index order, 8 gathered, 8 written; the pair
// packing makes the gather one 8-byte access instead of two 4-byte ones.
// Capacity: no kernel writes an edge slot >= max_edges, a record > max_rings or a vertex >= max_vertices; lead / rank / rings /
// write take the edge count read back from the header and refuse one above max_edges.
#include "trace_common.h"

#define OL_MAX_PIX ((int64_t)1 << 29)
// int32 slots of the header record (InsarRing: area2 0-1, label 2, leader 3, start 4, count 5, edges 6, ...)
#define OL_HDR_RINGS 2
#define OL_HDR_VERTS 5
#define OL_HDR_EDGES 6

__device__ __forceinline__ int ol_below(int mask, int s) { return __popc(mask & ((1 << s) - 1)); }

// what trace_common.h asks of its tool
struct OlTool {
  const int *lead, *eid, *labels;
  InsarRing* rings;
  __device__ __forceinline__ bool is_leader(int k) const { return lead[k] == k; }
  __device__ __forceinline__ void init_record(int r, int k, int, int len) const {      // area2 0, start / count by `write`, an empty box
    const int e = eid[k];
    int4* t4 = reinterpret_cast<int4*>(rings + 1 + r);
    t4[0] = make_int4(0, 0, labels[e >> 2], e);
    t4[1] = make_int4(0, 0, len, INT_MAX);
    t4[2] = make_int4(INT_MAX, 0, 0, 0);
  }
  // behind the first scan of a call E stands in its slot and the rest of the header record is cleared
  __device__ __forceinline__ static void first_header(int* hdr, int t, int slot, int carry, const int*, int, int) {
    if (t < (int)(sizeof(InsarRing) / 4)) hdr[t] = t == slot ? carry : 0;
  }
};

// ---------------------------------------------------------------------------------------------
// edges: mark / scan / offsets / link
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TR_THREADS)
outline_mark_kernel(const int* __restrict__ labels, int H, int W, int npix, int vec, uint8_t* __restrict__ mask,
                    int* __restrict__ counts) {
  __shared__ int wsum[TR_THREADS / INSAR_WAVE];
  const int i = blockIdx.x * TR_NB + threadIdx.x * 4;
  int v[4];
  quad_load(labels, i, npix, vec && i < npix, 0, v);
  uint32_t m4 = 0;
  if (i < npix) {
    int y = (int)((uint32_t)i / (uint32_t)W), x = i - y * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = v[j];
      if (i + j < npix && c != 0) {                              // x + 1 < W implies i + j + 1 < npix
        const int up = y > 0 ? labels[i + j - W] : 0, dn = y + 1 < H ? labels[i + j + W] : 0;
        const int lf = x > 0 ? (j > 0 ? v[j > 0 ? j - 1 : 0] : labels[i + j - 1]) : 0;
        const int rt = x + 1 < W ? (j < 3 ? v[j < 3 ? j + 1 : 3] : labels[i + j + 1]) : 0;
        const uint32_t m = (uint32_t)(up != c) | ((uint32_t)(rt != c) << 1) | ((uint32_t)(dn != c) << 2) | ((uint32_t)(lf != c) << 3);
        m4 |= m << (8 * j);
      }
      if (++x == W) { x = 0; ++y; }
    }
    if (vec) {
      *reinterpret_cast<uint32_t*>(mask + i) = m4;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < npix) mask[i + j] = (uint8_t)((m4 >> (8 * j)) & 0xffu);
    }
  }
  int total;
  block_prefix_sum<TR_THREADS>(__popc(m4), wsum, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TR_THREADS)
outline_offsets_kernel(const uint8_t* __restrict__ mask, int npix, int vec, const int* __restrict__ counts, int* __restrict__ off) {
  __shared__ int wsum[TR_THREADS / INSAR_WAVE];
  const int i = blockIdx.x * TR_NB + threadIdx.x * 4;
  int m[4];
  quad_load_u8(mask, i, npix, vec && i < npix, 0, m);
  const int c = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
  int total;
  int o = counts[blockIdx.x] + block_prefix_sum<TR_THREADS>(c, wsum, &total);
  int out[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { out[j] = o; o += __popc(m[j]); }
  if (i < npix) quad_store(off, i, npix, vec, out);
}

__device__ __forceinline__ int ol_label_at(const int* __restrict__ labels, int y, int x, int H, int W) {
  return ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? labels[y * W + x] : 0;
}

__global__ void __launch_bounds__(TR_THREADS)
outline_link_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ mask, const int* __restrict__ off, int H, int W,
                    int npix, int conn8, int cap, int* __restrict__ succ0, int* __restrict__ eid, uint8_t* __restrict__ turn,
                    int2* __restrict__ pair) {
  const int p = blockIdx.x * TR_THREADS + threadIdx.x;           // one pixel per thread: neighbouring lanes, neighbouring edges
  if (p >= npix) return;
  const int m = mask[p];
  if (!m) return;
  const int c = labels[p], base = off[p];
  const int y = (int)((uint32_t)p / (uint32_t)W), x = p - y * W;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!((m >> s) & 1)) continue;
    const int k = base + ol_below(m, s);
    if (k >= cap) continue;
    // travel direction d(s): east, south, west, north; the outer side lies towards d((s + 3) % 4)
    const int dy = (s == 1) - (s == 3), dx = (s == 0) - (s == 2);
    const int n = (s + 3) & 3;
    const int ny = (n == 1) - (n == 3), nx = (n == 0) - (n == 2);
    const int ay = y + dy, ax = x + dx, by = ay + ny, bx = ax + nx;
    const bool a = ol_label_at(labels, ay, ax, H, W) == c, b = ol_label_at(labels, by, bx, H, W) == c;
    int q, s2, t = 1;
    if (b && (a || conn8)) { q = by * W + bx; s2 = n; }          // left
    else if (a) { q = ay * W + ax; s2 = s; t = 0; }              // straight
    else { q = p; s2 = (s + 1) & 3; }                            // right
    int k2 = off[q] + ol_below(mask[q], s2);
    if (k2 >= cap) k2 = k;                                       // more edges than slots: the caller reads E and stops
    succ0[k] = k2;
    eid[k] = 4 * p + s;
    turn[k] = (uint8_t)t;
    pair[k] = make_int2(k2, k);
  }
}

// ---------------------------------------------------------------------------------------------
// lead / rank: the rounds are list_rank.h's; `cut` between them
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TR_THREADS)
outline_cut_kernel(const int2* __restrict__ in, const int* __restrict__ succ0, int* __restrict__ lead, int2* __restrict__ out, int n) {
  const int k = blockIdx.x * TR_THREADS + threadIdx.x;
  if (k >= n) return;
  const int m = in[k].y, s = succ0[k];
  lead[k] = m;
  out[k] = s == m ? make_int2(-1, 0) : make_int2(s, 1);          // the successor of a ring's last edge is its leader
}

// ---------------------------------------------------------------------------------------------
// write: scatter / reduce / scan / compact
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TR_THREADS)
outline_scatter_kernel(const int* __restrict__ lead, const int2* __restrict__ dist, const int2* __restrict__ info,
                       const int* __restrict__ succ0, const int* __restrict__ eid, const uint8_t* __restrict__ turn, int n, int W,
                       int corners_only, int2* __restrict__ overt, int* __restrict__ ometa, uint8_t* __restrict__ ocorner) {
  const int k = blockIdx.x * TR_THREADS + threadIdx.x;
  if (k >= n) return;
  const int m = lead[k];
  const int2 ri = info[m];
  const int pos = ri.y + dist[m].y - dist[k].y;
  if ((unsigned)pos >= (unsigned)n) return;                      // cannot happen on a permutation; never leave the arrays
  const int e = eid[k], s = e & 3, p = e >> 2;
  const int y = (int)((uint32_t)p / (uint32_t)W), x = p - y * W;
  overt[pos] = make_int2(y + (s >= 2), x + (s == 1 || s == 2));  // the tail: (y, x), (y, x+1), (y+1, x+1), (y+1, x)
  ometa[pos] = ri.x * 4 + s;                                     // a ring has four edges or more: ring * 4 < E
  const int ps = succ0[k] == m ? ri.y : pos + 1;
  if ((unsigned)ps < (unsigned)n) ocorner[ps] = corners_only ? turn[k] : (uint8_t)1;
}

__global__ void __launch_bounds__(TR_THREADS)
outline_reduce_kernel(const int2* __restrict__ overt, const int* __restrict__ ometa, const uint8_t* __restrict__ ocorner, int n,
                      InsarRing* __restrict__ rings, int max_rings, int* __restrict__ ccnt) {
  __shared__ int wsum[TR_THREADS / INSAR_WAVE];
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  int key = -1, vy = 0, vx = 0, flag = 0;
  long long a2 = 0;
  if (i < n) {
    const int meta = ometa[i], s = meta & 3;
    const int2 v = overt[i];
    key = meta >> 2; vy = v.x; vx = v.y; flag = ocorner[i];
    a2 = s == 0 ? -vy : s == 1 ? vx : s == 2 ? vy : -vx;         // x_i * y_{i+1} - x_{i+1} * y_i with the head one step along d(s)
  }
  const WaveRuns runs = wave_runs(key);
  const int tc = wave_run_reduce(runs, flag, WaveAdd());
  if (trace_reduce(runs, reinterpret_cast<TraceRecord*>(rings + 1), key, max_rings, a2, vy, vx)) atomicAdd(&rings[1 + key].count, tc);
  int total;
  block_prefix_sum<TR_THREADS>(flag, wsum, &total);
  if (threadIdx.x == 0) ccnt[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TR_THREADS)
outline_compact_kernel(const int2* __restrict__ overt, const int* __restrict__ ometa, const uint8_t* __restrict__ ocorner, int n,
                       const int* __restrict__ ccnt, InsarRing* __restrict__ rings, int max_rings, int2* __restrict__ vertices,
                       int max_vertices) {
  __shared__ int wsum[TR_THREADS / INSAR_WAVE];
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  const int flag = i < n ? ocorner[i] : 0;
  int total;
  const int o = ccnt[blockIdx.x] + block_prefix_sum<TR_THREADS>(flag, wsum, &total);
  if (i >= n) return;
  const int key = ometa[i] >> 2;
  if ((i == 0 || (ometa[i - 1] >> 2) != key) && key < max_rings) rings[1 + key].start = o;
  if (flag && o < max_vertices) vertices[o] = overt[i];
}

// ---------------------------------------------------------------------------------------------
// host side: scratch layout and the entry points
// ---------------------------------------------------------------------------------------------
struct OlLayout {
  int npix, nblk, cap, eblk, cblk;
  int64_t mask, off, counts, succ0, eid, turn, lead, p0, p1, overt, ometa, ocorner, rcnt, rlen, ccnt, bytes;
};

static int outline_layout(const char* who, int32_t H, int32_t W, int32_t max_edges, OlLayout* L) {
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  const int64_t npix = (int64_t)H * W;
  if (npix >= OL_MAX_PIX) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^29 pixels or more", who, H, W);
  if (int rc = trace_check_capacity(who, "max_edges", max_edges)) return rc;
  L->npix = (int)npix;
  L->nblk = (int)((npix + TR_NB - 1) / TR_NB);
  L->cap = max_edges;
  L->eblk = (max_edges + TR_NB - 1) / TR_NB;
  L->cblk = (max_edges + TR_THREADS - 1) / TR_THREADS;
  ScratchTake take;
  const int64_t cap = max_edges;
  L->mask = take(npix);        L->off = take(npix * 4);    L->counts = take((int64_t)L->nblk * 4);
  L->succ0 = take(cap * 4);    L->eid = take(cap * 4);     L->turn = take(cap);
  L->lead = take(cap * 4);     L->p0 = take(cap * 8);      L->p1 = take(cap * 8);
  L->overt = take(cap * 8);    L->ometa = take(cap * 4);   L->ocorner = take(cap);
  L->rcnt = take((int64_t)L->eblk * 4);  L->rlen = take((int64_t)L->eblk * 4);  L->ccnt = take((int64_t)L->cblk * 4);
  L->bytes = take.at;
  return INSAR_OK;
}
static int outline_check_count(const char* who, int32_t n_edges, const OlLayout& L) {
  return trace_check_count(who, "n_edges", n_edges, "max_edges", L.cap);
}

extern "C" int insar_outline_scratch_bytes(int32_t H, int32_t W, int32_t max_rings, int32_t max_edges, int64_t* scratch_bytes,
                                           int64_t* table_bytes) {
  const char* who = "insar_outline_scratch_bytes";
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  OlLayout L;
  if (int rc = outline_layout(who, H, W, max_edges, &L)) return rc;
  if (int rc = trace_check_capacity(who, "max_rings", max_rings)) return rc;
  *scratch_bytes = L.bytes;
  *table_bytes = (int64_t)sizeof(InsarRing) * ((int64_t)max_rings + 1);
  return INSAR_OK;
}

extern "C" int insar_outline_launches(int32_t n_edges) {
  return n_edges < 1 ? 6 : 12 + 2 * list_rounds(n_edges);
}

extern "C" int insar_outline_edges(const int32_t* labels, int32_t H, int32_t W, int32_t connectivity, int32_t max_edges,
                                   void* scratch, void* table, void* stream) {
  const char* who = "insar_outline_edges";
  if (!labels) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  OlLayout L;
  if (int rc = outline_layout(who, H, W, max_edges, &L)) return rc;
  if (connectivity != 4 && connectivity != 8) INSAR_FAIL(INSAR_E_ARG, "%s: connectivity %d (4 or 8)", who, connectivity);
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  if (((uintptr_t)labels) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: labels not 4-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int vec = L.npix % 4 == 0;
  const int lvec = vec && insar_aligned16(labels);
  uint8_t* mask = scratch_at<uint8_t>(scratch, L.mask);
  int *off = scratch_at<int>(scratch, L.off), *counts = scratch_at<int>(scratch, L.counts);
  hipLaunchKernelGGL(outline_mark_kernel, dim3((unsigned)L.nblk), dim3(TR_THREADS), 0, s, labels, H, W, L.npix, lvec, mask, counts);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(trace_scan_kernel<OlTool>, dim3(1), dim3(TR_SCAN_THREADS), 0, s, counts, (int*)nullptr, L.nblk, (int*)table,
                     OL_HDR_EDGES, 1);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(outline_offsets_kernel, dim3((unsigned)L.nblk), dim3(TR_THREADS), 0, s, mask, L.npix, vec, counts, off);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(outline_link_kernel, dim3(scene_blocks(L.npix, TR_THREADS)), dim3(TR_THREADS), 0, s, labels, mask, off, H, W,
                     L.npix, connectivity == 8, L.cap, scratch_at<int>(scratch, L.succ0), scratch_at<int>(scratch, L.eid),
                     scratch_at<uint8_t>(scratch, L.turn), scratch_at<int2>(scratch, L.p0));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_outline_lead(int32_t H, int32_t W, int32_t n_edges, int32_t max_edges, void* scratch, void* stream) {
  const char* who = "insar_outline_lead";
  OlLayout L;
  if (int rc = outline_layout(who, H, W, max_edges, &L)) return rc;
  if (int rc = outline_check_count(who, n_edges, L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (n_edges == 0) return INSAR_OK;
  return trace_lead(scratch_at<int2>(scratch, L.p0), scratch_at<int2>(scratch, L.p1), n_edges, (hipStream_t)stream, who);
}

extern "C" int insar_outline_rank(int32_t H, int32_t W, int32_t n_edges, int32_t max_edges, void* scratch, void* stream) {
  const char* who = "insar_outline_rank";
  OlLayout L;
  if (int rc = outline_layout(who, H, W, max_edges, &L)) return rc;
  if (int rc = outline_check_count(who, n_edges, L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (n_edges == 0) return INSAR_OK;
  hipStream_t s = (hipStream_t)stream;
  auto cut = [&](const int2* in, int2* out) {
    hipLaunchKernelGGL(outline_cut_kernel, dim3(scene_blocks(n_edges, TR_THREADS)), dim3(TR_THREADS), 0, s, in,
                       (const int*)scratch_at<int>(scratch, L.succ0), scratch_at<int>(scratch, L.lead), out, n_edges);
  };
  return trace_cut_and_rank(cut, scratch_at<int2>(scratch, L.p0), scratch_at<int2>(scratch, L.p1), n_edges, s, who);
}

extern "C" int insar_outline_rings(const int32_t* labels, int32_t H, int32_t W, int32_t n_edges, int32_t max_rings,
                                   int32_t max_edges, void* scratch, void* table, void* stream) {
  const char* who = "insar_outline_rings";
  if (!labels) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  OlLayout L;
  if (int rc = outline_layout(who, H, W, max_edges, &L)) return rc;
  if (int rc = outline_check_count(who, n_edges, L)) return rc;
  if (int rc = trace_check_table(who, "max_rings", max_rings, table)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (((uintptr_t)labels) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: labels not 4-byte aligned", who);
  const OlTool tool = {scratch_at<int>(scratch, L.lead), scratch_at<int>(scratch, L.eid), labels, (InsarRing*)table};
  return trace_number(tool, scratch_at<int2>(scratch, L.p1), n_edges, scratch_at<int>(scratch, L.rcnt), scratch_at<int>(scratch, L.rlen),
                      scratch_at<int2>(scratch, L.p0), table, OL_HDR_RINGS, max_rings, (hipStream_t)stream, who);
}

extern "C" int insar_outline_write(int32_t H, int32_t W, int32_t n_edges, int32_t corners_only, int32_t max_rings,
                                   int32_t max_vertices, int32_t max_edges, void* scratch, void* table, int32_t* vertices,
                                   void* stream) {
  const char* who = "insar_outline_write";
  OlLayout L;
  if (int rc = outline_layout(who, H, W, max_edges, &L)) return rc;
  if (int rc = outline_check_count(who, n_edges, L)) return rc;
  if (int rc = trace_check_table(who, "max_rings", max_rings, table)) return rc;
  if (max_vertices < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_vertices %d < 1", who, max_vertices);
  if (!vertices) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (((uintptr_t)vertices) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: vertices not 8-byte aligned", who);
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = (int)scene_blocks(n_edges, TR_THREADS);
  int2* overt = scratch_at<int2>(scratch, L.overt);
  int *ometa = scratch_at<int>(scratch, L.ometa), *ccnt = scratch_at<int>(scratch, L.ccnt);
  uint8_t* ocorner = scratch_at<uint8_t>(scratch, L.ocorner);
  if (nblk > 0) {
    hipLaunchKernelGGL(outline_scatter_kernel, dim3((unsigned)nblk), dim3(TR_THREADS), 0, s, (const int*)scratch_at<int>(scratch, L.lead),
                       (const int2*)scratch_at<int2>(scratch, L.p1), (const int2*)scratch_at<int2>(scratch, L.p0),
                       (const int*)scratch_at<int>(scratch, L.succ0), (const int*)scratch_at<int>(scratch, L.eid),
                       (const uint8_t*)scratch_at<uint8_t>(scratch, L.turn), n_edges, W, corners_only != 0, overt, ometa, ocorner);
    INSAR_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(outline_reduce_kernel, dim3((unsigned)nblk), dim3(TR_THREADS), 0, s, (const int2*)overt, (const int*)ometa,
                       (const uint8_t*)ocorner, n_edges, (InsarRing*)table, max_rings, ccnt);
    INSAR_CHECK_LAUNCH(who);
  }
  hipLaunchKernelGGL(trace_scan_kernel<OlTool>, dim3(1), dim3(TR_SCAN_THREADS), 0, s, ccnt, (int*)nullptr, nblk, (int*)table,
                     OL_HDR_VERTS, 0);
  INSAR_CHECK_LAUNCH(who);
  if (nblk > 0) {
    hipLaunchKernelGGL(outline_compact_kernel, dim3((unsigned)nblk), dim3(TR_THREADS), 0, s, (const int2*)overt, (const int*)ometa,
                       (const uint8_t*)ocorner, n_edges, (const int*)ccnt, (InsarRing*)table, max_rings,
                       reinterpret_cast<int2*>(vertices), max_vertices);
    INSAR_CHECK_LAUNCH(who);
  }
  return INSAR_OK;
}
