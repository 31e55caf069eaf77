// Contour lines: the iso-lines of a raster [H][W] (float32, uint8 or int32) at up to 32 levels as ordered polylines of sub-pixel
// vertices in 1/256 pixel, closed rings and open lines, by marching squares in exact integers. Semantics: include/insar_hip.h.
// A node is a pixel centre, a lattice edge joins a node p to its right (o = 0) or lower (o = 1) neighbour, and a crossing is a
// lattice edge whose two valid ends lie on different sides of level l and that bounds a cell of four valid nodes; its id is
// (l * H * W + p) * 2 + o, its COMPACT index k the number of crossings with a smaller id. Every array below is indexed by k;
// per level the raster has one 2-bit mask per pixel, four pixels to a 32-bit word (the plane padded to whole words), and one
// compact index per WORD: index(l, p, o) = off4[word] + popcount(mask bits of the word below bit 8 (p & 3) + o).
// With E crossings and R = ceil(log2 E):
//
//   edges   quantise  per pixel: q (zonal.hip's rule) and the valid flag; the only kernel that sees a float
//           mark      per word of four pixels: which of its eight lattice edges are crossings, level by level (q is loaded once
//                     for all levels); crossings per level and block of 1024 pixels
//           scan      trace_common.h: the prefix sum of the counts in (level, block) order; E goes to the table header, and
//                     CtTool's first_header writes the rest of it: no line yet, V = E, the crossings per level
//           offsets   per level and word: the compact index of its first crossing
//           link      per crossing: vertex, id, successor (the turn rule below) or none, "no predecessor" flag; pair (succ, k),
//                     a crossing without successor (a tail) pointing at itself
//   lead    trace_common.h: after R rounds of pointer doubling an element of a ring knows the ring's smallest crossing, an
//           element of an open line has jumped to its tail (the fixed point), and "my jump target has no successor" tells the
//           two apart
//   rank    cut       rings are cut in front of their leader, open lines end at their tail anyway: pair (next, 1) or (-1, 0);
//                     lead[k] = the ring's leader, or -1 - tail for an open line, whose head writes itself at its tail's slot
//           trace_common.h: after R rounds of list ranking d[k] is the distance from k to the last crossing of its line
//   lines   trace_common.h (count / scan / number) with CtTool: a leader is a ring's minimum or the head of an open line; the
//           number of lines goes to the header
//   write   scatter   per crossing: position = line start + rank; the vertex goes there (every crossing is kept: V = E)
//           reduce    over the ordered array, where a line is one contiguous run: area2 of the rings and the box by
//                     trace_common.h's trace_reduce
//
// 11 + 2 R launches, a function of E alone (5 when E = 0); how the steps are ordered and why the atomics' arrival order changes
// nothing: trace_common.h. Integers only behind `quantise`. A round moves 24 bytes per crossing (8 read in index order,
// 8 gathered, 8 written). Capacity: no kernel writes a crossing slot or a vertex >= max_vertices or a record > max_lines.
//
// The turn rule of `link`. The line runs with the above side on its right. Through a crossing it travels in direction d with the
// above end A of the lattice edge on the right and the below end B on the left; the cell ahead has A' = A + d and B' = B + d. A'
// below: turn right (leave through A - A'), unless B' is above and the saddle is joined (the four q sum to >= 4 q_l), then turn left
// (leave through B - B'); A' above: left if B' is above too, else straight on (leave through A' - B').
#include "trace_common.h"

#define CT_MAX_LEVELS 32
#define CT_MAX_SIDE (1 << 22)             // 256 * side + 128 fits an int32
#define CT_LIMIT 2147483647.0
#define CT_HDR 4                          // records of the table header: 48 int32 slots
// int32 slots of the header (InsarContourLine: area2 0-1, level 2, leader 3, start 4, count 5, ...)
#define CT_HDR_LINES 2
#define CT_HDR_CROSSINGS 3
#define CT_HDR_VERTS 5
#define CT_HDR_LEVELS 16                  // .. 47: crossings per level

static_assert(CT_HDR_LEVELS + CT_MAX_LEVELS == CT_HDR * (int)sizeof(InsarContourLine) / 4, "the level counts end the header");

struct CtLevels { int q[CT_MAX_LEVELS]; };

// what trace_common.h asks of its tool
struct CtTool {
  const int *lead, *eid;
  const uint8_t* head;
  InsarContourLine* lines;
  int npix2;
  __device__ __forceinline__ bool is_leader(int k) const {       // a ring's smallest crossing, or the head of an open line
    return lead[k] == k || head[k];
  }
  __device__ __forceinline__ void init_record(int r, int k, int start, int len) const {     // area2 0, an empty box
    const int e = eid[k];
    int4* t4 = reinterpret_cast<int4*>(lines + CT_HDR + r);
    t4[0] = make_int4(0, 0, (int)((uint32_t)e / (uint32_t)npix2), e);
    t4[1] = make_int4(start, len, lead[k] >= 0, INT_MAX);
    t4[2] = make_int4(INT_MAX, 0, 0, 0);
  }
  // behind the first scan of a call (a[] is L levels of nblk / L counts each; E in its slot): no line yet, V = E, the crossings
  // per level, zero for the levels that are not there
  __device__ __forceinline__ static void first_header(int* hdr, int t, int slot, int carry, const int* a, int nblk, int L) {
    if (t < CT_HDR_LEVELS) {
      hdr[t] = (t == slot || t == CT_HDR_VERTS) ? carry : 0;
    } else if (t < CT_HDR_LEVELS + CT_MAX_LEVELS) {
      const int l = t - CT_HDR_LEVELS, per = nblk / L;
      hdr[t] = l < L ? (l + 1 < L ? a[(l + 1) * per] : carry) - a[l * per] : 0;
    }
  }
};

// ---------------------------------------------------------------------------------------------
// edges: quantise / mark / scan / offsets / link
// ---------------------------------------------------------------------------------------------
// four raster elements as values the quantiser takes (zonal.hip's ZnRaster, without the clipped count)
template <typename T> struct CtRaster;
template <> struct CtRaster<float> {
  typedef float V;
  __device__ __forceinline__ static void load(const float* p, int64_t i, int64_t n, bool vec, V* v) { quad_load(p, i, n, vec, 0.0f, v); }
  __device__ __forceinline__ static bool quantise(V v, double scale, bool has_nodata, double nodata, int* q) {
    if (!(fabsf(v) <= 3.402823466e38f) || (has_nodata && v == (float)nodata)) return false;
    double d = (double)v * scale;
    d = d > CT_LIMIT ? CT_LIMIT : d < -CT_LIMIT ? -CT_LIMIT : d;
    *q = (int)rint(d);                                           // nearest even; |d| <= 2^31 - 1 fits
    return true;
  }
};
template <> struct CtRaster<int> {
  typedef int V;
  __device__ __forceinline__ static void load(const int* p, int64_t i, int64_t n, bool vec, V* v) { quad_load(p, i, n, vec, 0, v); }
  __device__ __forceinline__ static bool quantise(V v, double, bool has_nodata, double nodata, int* q) {
    if (has_nodata && v == (int)nodata) return false;
    *q = v;
    return true;
  }
};
template <> struct CtRaster<uint8_t> {
  typedef int V;
  __device__ __forceinline__ static void load(const uint8_t* p, int64_t i, int64_t n, bool vec, V* v) { quad_load_u8(p, i, n, vec, 0, v); }
  __device__ __forceinline__ static bool quantise(V v, double s, bool has_nodata, double nodata, int* q) {
    return CtRaster<int>::quantise(v, s, has_nodata, nodata, q);
  }
};

template <typename T>
__global__ void __launch_bounds__(TR_THREADS)
contour_quantise_kernel(const T* __restrict__ raster, const uint8_t* __restrict__ valid, int npix, int rvec, int vvec, int vec,
                        double scale, int has_nodata, double nodata, int* __restrict__ q, uint8_t* __restrict__ ok) {
  const int i = (blockIdx.x * TR_THREADS + threadIdx.x) * 4;
  if (i >= npix) return;
  typename CtRaster<T>::V v[4];
  CtRaster<T>::load(raster, i, npix, rvec, v);
  int use[4] = {1, 1, 1, 1};
  if (valid) quad_load_u8(valid, i, npix, vvec, 0, use);
  int out[4];
  uint32_t ok4 = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int qq = 0;
    const bool good = i + j < npix && use[j] != 0 && CtRaster<T>::quantise(v[j], scale, has_nodata != 0, nodata, &qq);
    out[j] = good ? qq : 0;
    ok4 |= (uint32_t)good << (8 * j);
  }
  quad_store(q, i, npix, vec, out);
  if (vec) {
    *reinterpret_cast<uint32_t*>(ok + i) = ok4;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < npix) ok[i + j] = (uint8_t)((ok4 >> (8 * j)) & 1u);
  }
}

__global__ void __launch_bounds__(TR_THREADS)
contour_mark_kernel(const int* __restrict__ q, const uint8_t* __restrict__ ok, int H, int W, int npix, int nq, int nblk, int L,
                    CtLevels lv, uint32_t* __restrict__ mask, int* __restrict__ counts) {
  __shared__ int cnt[CT_MAX_LEVELS];
  if (threadIdx.x < CT_MAX_LEVELS) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int t = blockIdx.x * TR_THREADS + threadIdx.x;
  if (t < nq) {
    const int i = 4 * t;
    int qp[4], qr[4], qb[4];
    uint32_t e = 0;                                              // bit 2 j + o: lattice edge o of pixel i + j can be a crossing
    int y = (int)((uint32_t)i / (uint32_t)W), x = i - y * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = i + j;
      qp[j] = qr[j] = qb[j] = 0;
      if (p < npix && ok[p]) {
        const bool r = x + 1 < W && ok[p + 1], b = y + 1 < H && ok[p + W];
        qp[j] = q[p];
        if (r) {                                                 // the cell above or the cell below emits
          qr[j] = q[p + 1];
          const bool up = y > 0 && ok[p - W] && ok[p - W + 1], dn = b && ok[p + W + 1];
          if (up || dn) e |= 1u << (2 * j);
        }
        if (b) {                                                 // the cell to the left or the cell to the right emits
          qb[j] = q[p + W];
          const bool lf = x > 0 && ok[p - 1] && ok[p + W - 1], rt = r && ok[p + W + 1];
          if (lf || rt) e |= 2u << (2 * j);
        }
      }
      if (++x == W) { x = 0; ++y; }
    }
    for (int l = 0; l < L; ++l) {
      const int lq = lv.q[l];
      uint32_t m4 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool a = qp[j] >= lq;
        const uint32_t m = (uint32_t)(a != (qr[j] >= lq)) | ((uint32_t)(a != (qb[j] >= lq)) << 1);
        m4 |= (m & (e >> (2 * j)) & 3u) << (8 * j);
      }
      mask[l * nq + t] = m4;
      if (m4) atomicAdd(&cnt[l], __popc(m4));                    // LDS; an integer sum, whatever the order
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < L) counts[threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
}

__global__ void __launch_bounds__(TR_THREADS)
contour_offsets_kernel(const uint32_t* __restrict__ mask, int nq, int nblk, const int* __restrict__ counts, int* __restrict__ off4) {
  __shared__ int wsum[TR_THREADS / INSAR_WAVE];
  const int l = blockIdx.y, t = blockIdx.x * TR_THREADS + threadIdx.x;
  const uint32_t w = t < nq ? mask[l * nq + t] : 0u;
  int total;
  const int o = counts[l * nblk + blockIdx.x] + block_prefix_sum<TR_THREADS>(__popc(w), wsum, &total);
  if (t < nq) off4[l * nq + t] = o;
}

// the compact index of crossing (p, o) of the level whose planes start at word `base`
__device__ __forceinline__ int ct_index(const uint32_t* __restrict__ mask, const int* __restrict__ off4, int base, int p, int o) {
  const int w = base + (p >> 2);
  return off4[w] + __popc(mask[w] & ((1u << (8 * (p & 3) + o)) - 1u));
}

__global__ void __launch_bounds__(TR_THREADS)
contour_link_kernel(const int* __restrict__ q, const uint8_t* __restrict__ ok, const uint32_t* __restrict__ mask,
                    const int* __restrict__ off4, int H, int W, int npix, int nq, CtLevels lv, int cap, int* __restrict__ succ0,
                    int* __restrict__ eid, int2* __restrict__ vert, uint8_t* __restrict__ head, int2* __restrict__ pair) {
  const int l = blockIdx.y, t = blockIdx.x * TR_THREADS + threadIdx.x;
  if (t >= nq) return;
  const int base = l * nq;
  const uint32_t m4 = mask[base + t];
  if (!m4) return;
  const int lq = lv.q[l];
  int k = off4[base + t];
  for (int bit = 0; bit < 32; bit += (bit & 1) ? 7 : 1) {        // bits 8 j and 8 j + 1
    if (!((m4 >> bit) & 1u)) continue;
    const int kk = k++;
    if (kk >= cap) continue;
    const int p = 4 * t + (bit >> 3), o = bit & 1;
    const int y = (int)((uint32_t)p / (uint32_t)W), x = p - y * W;
    const int qp = q[p], qn = q[p + (o ? W : 1)];
    const bool ap = qp >= lq;
    // the position, measured from the below end: s = floor(((q_l - q_below) * 512 + d) / (2 d)), 1 .. 255
    const long long qa = ap ? qp : qn, qb = ap ? qn : qp, d = qa - qb;
    long long s = (((long long)lq - qb) * 512 + d) / (2 * d);
    s = s < 1 ? 1 : s > 255 ? 255 : s;
    const int offp = ap ? 256 - (int)s : (int)s;
    // travel direction d, the above end A on its right, the below end B on its left
    int dy = 0, dx = 0, Ay = y, Ax = x, By = y, Bx = x;
    if (o == 0) {
      if (ap) { dy = 1; Bx = x + 1; } else { dy = -1; Ax = x + 1; }
    } else {
      if (ap) { dx = -1; By = y + 1; } else { dx = 1; Ay = y + 1; }
    }
    const int nAy = Ay + dy, nAx = Ax + dx, nBy = By + dy, nBx = Bx + dx;      // the cell ahead
    const int pAy = Ay - dy, pAx = Ax - dx, pBy = By - dy, pBx = Bx - dx;      // the cell behind
    const bool ahead = (unsigned)nAy < (unsigned)H && (unsigned)nAx < (unsigned)W && ok[nAy * W + nAx] && ok[nBy * W + nBx];
    const bool behind = (unsigned)pAy < (unsigned)H && (unsigned)pAx < (unsigned)W && ok[pAy * W + pAx] && ok[pBy * W + pBx];
    int k2 = -1;
    if (ahead) {
      const int qA2 = q[nAy * W + nAx], qB2 = q[nBy * W + nBx];
      const bool aA = qA2 >= lq, aB = qB2 >= lq;
      int uy, ux, vy, vx;
      bool left;
      if (!aA) left = aB && (long long)qa + qb + qA2 + qB2 >= 4 * (long long)lq;   // a saddle is joined through its centre
      else left = aB;
      if (!aA && !left) { uy = Ay; ux = Ax; vy = nAy; vx = nAx; }              // right
      else if (left) { uy = By; ux = Bx; vy = nBy; vx = nBx; }                 // left
      else { uy = nAy; ux = nAx; vy = nBy; vx = nBx; }                         // straight on
      const int o2 = uy == vy ? 0 : 1;
      const int p2 = min(uy, vy) * W + min(ux, vx);
      k2 = ct_index(mask, off4, base, p2, o2);
      if (k2 >= cap) k2 = -1;                                    // more crossings than slots: the caller reads E and stops
    }
    succ0[kk] = k2;
    eid[kk] = (l * npix + p) * 2 + o;
    vert[kk] = make_int2(256 * y + 128 + (o ? offp : 0), 256 * x + 128 + (o ? 0 : offp));
    head[kk] = (uint8_t)!behind;
    pair[kk] = make_int2(k2 < 0 ? kk : k2, kk);
  }
}

// ---------------------------------------------------------------------------------------------
// lead / rank: the rounds are list_rank.h's; `cut` between them
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TR_THREADS)
contour_cut_kernel(const int2* __restrict__ in, const int* __restrict__ succ0, const uint8_t* __restrict__ head,
                   int* __restrict__ lead, int* __restrict__ headof, int2* __restrict__ out, int n) {
  const int k = blockIdx.x * TR_THREADS + threadIdx.x;
  if (k >= n) return;
  const int2 a = in[k];
  const int s = succ0[k];
  if (succ0[a.x] < 0) {                                          // the jump target is a tail: an open line
    lead[k] = -1 - a.x;
    if (head[k]) headof[a.x] = k;                                // one head per line: the only writer of this slot
    out[k] = s < 0 ? make_int2(-1, 0) : make_int2(s, 1);
  } else {
    lead[k] = a.y;
    out[k] = s == a.y ? make_int2(-1, 0) : make_int2(s, 1);      // the successor of a ring's last crossing is its leader
  }
}

// ---------------------------------------------------------------------------------------------
// write: scatter / reduce
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TR_THREADS)
contour_scatter_kernel(const int* __restrict__ lead, const int* __restrict__ headof, const int2* __restrict__ dist,
                       const int2* __restrict__ info, const int2* __restrict__ vert, int n, int* __restrict__ ometa,
                       int2* __restrict__ vertices) {
  const int k = blockIdx.x * TR_THREADS + threadIdx.x;
  if (k >= n) return;
  const int l = lead[k];
  const int m = l >= 0 ? l : headof[-1 - l];
  if ((unsigned)m >= (unsigned)n) return;                        // cannot happen; never leave the arrays
  const int2 li = info[m];
  const int pos = li.y + dist[m].y - dist[k].y;
  if ((unsigned)pos >= (unsigned)n) return;
  ometa[pos] = li.x;
  vertices[pos] = vert[k];
}

__global__ void __launch_bounds__(TR_THREADS)
contour_reduce_kernel(const int2* __restrict__ vertices, const int* __restrict__ ometa, int n,
                      InsarContourLine* __restrict__ lines, int max_lines) {
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  int key = -1, vy = 0, vx = 0;
  long long a2 = 0;
  if (i < n) {
    const int r = ometa[i];
    if (r < max_lines) {
      const int2 v = vertices[i];
      key = r; vy = v.x; vx = v.y;
      const InsarContourLine* ln = lines + CT_HDR + r;           // closed and start were written by `number` and stay
      if (ln->closed) {
        const int nxt = (i + 1 < n && ometa[i + 1] == r) ? i + 1 : ln->start;
        const int2 w = vertices[(unsigned)nxt < (unsigned)n ? nxt : i];
        a2 = (long long)vx * w.x - (long long)w.y * vy;          // x_i * y_{i+1} - x_{i+1} * y_i
      }
    }
  }
  trace_reduce(wave_runs(key), reinterpret_cast<TraceRecord*>(lines + CT_HDR), key, max_lines, a2, vy, vx);
}

// ---------------------------------------------------------------------------------------------
// host side: scratch layout and the entry points
// ---------------------------------------------------------------------------------------------
struct CtLayout {
  int npix, nq, nblk, L, cap, eblk;
  int64_t q, ok, mask, off4, counts, succ0, eid, vert, head, lead, headof, p0, p1, ometa, lcnt, llen, bytes;
};

static int contour_layout(const char* who, int32_t H, int32_t W, int32_t n_levels, int32_t max_vertices, CtLayout* L) {
  if (H < 1 || W < 1 || H > CT_MAX_SIDE || W > CT_MAX_SIDE) INSAR_FAIL(INSAR_E_SHAPE, "%s: raster %d x %d: H, W in 1 .. 2^22", who, H, W);
  if (n_levels < 1 || n_levels > CT_MAX_LEVELS) INSAR_FAIL(INSAR_E_SHAPE, "%s: n_levels %d outside 1 .. %d", who, n_levels, CT_MAX_LEVELS);
  const int64_t npix = (int64_t)H * W;
  if (npix * n_levels >= ((int64_t)1 << 30))
    INSAR_FAIL(INSAR_E_SHAPE, "%s: n_levels * H * W = %d * %d * %d is 2^30 or more", who, n_levels, H, W);
  if (int rc = trace_check_capacity(who, "max_vertices", max_vertices)) return rc;
  L->npix = (int)npix;
  L->nq = (int)((npix + 3) / 4);
  L->nblk = (L->nq + TR_THREADS - 1) / TR_THREADS;
  L->L = n_levels;
  L->cap = max_vertices;
  L->eblk = (max_vertices + TR_NB - 1) / TR_NB;
  ScratchTake take;
  const int64_t cap = max_vertices, words = (int64_t)n_levels * L->nq;
  L->q = take(npix * 4);       L->ok = take(npix);         L->mask = take(words * 4);   L->off4 = take(words * 4);
  L->counts = take((int64_t)n_levels * L->nblk * 4);
  L->succ0 = take(cap * 4);    L->eid = take(cap * 4);     L->vert = take(cap * 8);     L->head = take(cap);
  L->lead = take(cap * 4);     L->headof = take(cap * 4);  L->p0 = take(cap * 8);       L->p1 = take(cap * 8);
  L->ometa = take(cap * 4);
  L->lcnt = take((int64_t)L->eblk * 4);  L->llen = take((int64_t)L->eblk * 4);
  L->bytes = take.at;
  return INSAR_OK;
}
static int contour_check_count(const char* who, int32_t n, const CtLayout& L) {
  return trace_check_count(who, "n_crossings", n, "max_vertices", L.cap);
}

extern "C" int insar_contour_scratch_bytes(int32_t H, int32_t W, int32_t n_levels, int32_t max_lines, int32_t max_vertices,
                                           int64_t* scratch_bytes, int64_t* table_bytes) {
  const char* who = "insar_contour_scratch_bytes";
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  CtLayout L;
  if (int rc = contour_layout(who, H, W, n_levels, max_vertices, &L)) return rc;
  if (int rc = trace_check_capacity(who, "max_lines", max_lines)) return rc;
  *scratch_bytes = L.bytes;
  *table_bytes = (int64_t)sizeof(InsarContourLine) * ((int64_t)max_lines + CT_HDR);
  return INSAR_OK;
}

extern "C" int insar_contour_launches(int32_t n_crossings) {
  return n_crossings < 1 ? 5 : 11 + 2 * list_rounds(n_crossings);
}

template <typename T>
static void contour_launch_quantise(const void* raster, const uint8_t* valid, const CtLayout& L, double scale, int32_t has_nodata,
                                    double nodata, void* scratch, hipStream_t s) {
  const int vec = L.npix % 4 == 0;
  const int rvec = vec && insar_aligned16(raster), vvec = vec && valid && ((((uintptr_t)valid) & 3u) == 0);
  hipLaunchKernelGGL(contour_quantise_kernel<T>, dim3(scene_blocks(L.nq, TR_THREADS)), dim3(TR_THREADS), 0, s, (const T*)raster, valid,
                     L.npix, rvec, vvec, vec, scale, has_nodata, nodata, scratch_at<int>(scratch, L.q), scratch_at<uint8_t>(scratch, L.ok));
}

extern "C" int insar_contour_edges(const void* raster, int32_t elem_type, int32_t H, int32_t W, double scale, int32_t has_nodata,
                                   double nodata, const uint8_t* valid, const int32_t* levels_q, int32_t n_levels,
                                   int32_t max_vertices, void* scratch, void* table, void* stream) {
  const char* who = "insar_contour_edges";
  if (!raster || !levels_q) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  CtLayout L;
  if (int rc = contour_layout(who, H, W, n_levels, max_vertices, &L)) return rc;
  if (elem_type != INSAR_ZONAL_F32 && elem_type != INSAR_ZONAL_U8 && elem_type != INSAR_ZONAL_I32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: elem_type %d (INSAR_ZONAL_F32, _U8 or _I32)", who, elem_type);
  if (!(scale > 0.0) || !(scale <= 1.7976931348623157e308)) INSAR_FAIL(INSAR_E_ARG, "%s: scale must be positive and finite", who);
  if (has_nodata && nodata != nodata) INSAR_FAIL(INSAR_E_ARG, "%s: nodata is NaN", who);
  CtLevels lv;
  for (int l = 0; l < CT_MAX_LEVELS; ++l) lv.q[l] = l < n_levels ? levels_q[l] : INT_MAX;
  for (int l = 1; l < n_levels; ++l)
    if (lv.q[l] <= lv.q[l - 1]) INSAR_FAIL(INSAR_E_ARG, "%s: levels_q[%d] = %d is not above levels_q[%d] = %d", who, l, lv.q[l], l - 1, lv.q[l - 1]);
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (int rc = scene_check_buffer(who, "table", table)) return rc;
  if (elem_type != INSAR_ZONAL_U8 && (((uintptr_t)raster) & 3u)) INSAR_FAIL(INSAR_E_ALIGN, "%s: raster not 4-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  if (elem_type == INSAR_ZONAL_F32) contour_launch_quantise<float>(raster, valid, L, scale, has_nodata, nodata, scratch, s);
  else if (elem_type == INSAR_ZONAL_I32) contour_launch_quantise<int>(raster, valid, L, scale, has_nodata, nodata, scratch, s);
  else contour_launch_quantise<uint8_t>(raster, valid, L, scale, has_nodata, nodata, scratch, s);
  INSAR_CHECK_LAUNCH(who);
  const int* q = scratch_at<int>(scratch, L.q);
  const uint8_t* ok = scratch_at<uint8_t>(scratch, L.ok);
  uint32_t* mask = scratch_at<uint32_t>(scratch, L.mask);
  int *off4 = scratch_at<int>(scratch, L.off4), *counts = scratch_at<int>(scratch, L.counts);
  hipLaunchKernelGGL(contour_mark_kernel, dim3((unsigned)L.nblk), dim3(TR_THREADS), 0, s, q, ok, H, W, L.npix, L.nq, L.nblk, L.L, lv,
                     mask, counts);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(trace_scan_kernel<CtTool>, dim3(1), dim3(TR_SCAN_THREADS), 0, s, counts, (int*)nullptr, L.L * L.nblk, (int*)table,
                     CT_HDR_CROSSINGS, L.L);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(contour_offsets_kernel, dim3((unsigned)L.nblk, (unsigned)L.L), dim3(TR_THREADS), 0, s, (const uint32_t*)mask,
                     L.nq, L.nblk, (const int*)counts, off4);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(contour_link_kernel, dim3((unsigned)L.nblk, (unsigned)L.L), dim3(TR_THREADS), 0, s, q, ok, (const uint32_t*)mask,
                     (const int*)off4, H, W, L.npix, L.nq, lv, L.cap, scratch_at<int>(scratch, L.succ0), scratch_at<int>(scratch, L.eid),
                     scratch_at<int2>(scratch, L.vert), scratch_at<uint8_t>(scratch, L.head), scratch_at<int2>(scratch, L.p0));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_contour_lead(int32_t H, int32_t W, int32_t n_levels, int32_t n_crossings, int32_t max_vertices, void* scratch,
                                  void* stream) {
  const char* who = "insar_contour_lead";
  CtLayout L;
  if (int rc = contour_layout(who, H, W, n_levels, max_vertices, &L)) return rc;
  if (int rc = contour_check_count(who, n_crossings, L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (n_crossings == 0) return INSAR_OK;
  return trace_lead(scratch_at<int2>(scratch, L.p0), scratch_at<int2>(scratch, L.p1), n_crossings, (hipStream_t)stream, who);
}

extern "C" int insar_contour_rank(int32_t H, int32_t W, int32_t n_levels, int32_t n_crossings, int32_t max_vertices, void* scratch,
                                  void* stream) {
  const char* who = "insar_contour_rank";
  CtLayout L;
  if (int rc = contour_layout(who, H, W, n_levels, max_vertices, &L)) return rc;
  if (int rc = contour_check_count(who, n_crossings, L)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (n_crossings == 0) return INSAR_OK;
  hipStream_t s = (hipStream_t)stream;
  auto cut = [&](const int2* in, int2* out) {
    hipLaunchKernelGGL(contour_cut_kernel, dim3(scene_blocks(n_crossings, TR_THREADS)), dim3(TR_THREADS), 0, s, in,
                       (const int*)scratch_at<int>(scratch, L.succ0), (const uint8_t*)scratch_at<uint8_t>(scratch, L.head),
                       scratch_at<int>(scratch, L.lead), scratch_at<int>(scratch, L.headof), out, n_crossings);
  };
  return trace_cut_and_rank(cut, scratch_at<int2>(scratch, L.p0), scratch_at<int2>(scratch, L.p1), n_crossings, s, who);
}

extern "C" int insar_contour_lines(int32_t H, int32_t W, int32_t n_levels, int32_t n_crossings, int32_t max_lines,
                                   int32_t max_vertices, void* scratch, void* table, void* stream) {
  const char* who = "insar_contour_lines";
  CtLayout L;
  if (int rc = contour_layout(who, H, W, n_levels, max_vertices, &L)) return rc;
  if (int rc = contour_check_count(who, n_crossings, L)) return rc;
  if (int rc = trace_check_table(who, "max_lines", max_lines, table)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  const CtTool tool = {scratch_at<int>(scratch, L.lead), scratch_at<int>(scratch, L.eid), scratch_at<uint8_t>(scratch, L.head),
                       (InsarContourLine*)table, 2 * L.npix};
  return trace_number(tool, scratch_at<int2>(scratch, L.p1), n_crossings, scratch_at<int>(scratch, L.lcnt), scratch_at<int>(scratch, L.llen),
                      scratch_at<int2>(scratch, L.p0), table, CT_HDR_LINES, max_lines, (hipStream_t)stream, who);
}

extern "C" int insar_contour_write(int32_t H, int32_t W, int32_t n_levels, int32_t n_crossings, int32_t max_lines,
                                   int32_t max_vertices, void* scratch, void* table, int32_t* vertices, void* stream) {
  const char* who = "insar_contour_write";
  CtLayout L;
  if (int rc = contour_layout(who, H, W, n_levels, max_vertices, &L)) return rc;
  if (int rc = contour_check_count(who, n_crossings, L)) return rc;
  if (int rc = trace_check_table(who, "max_lines", max_lines, table)) return rc;
  if (!vertices) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (vertices)", who);
  if (((uintptr_t)vertices) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: vertices not 8-byte aligned", who);
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (n_crossings == 0) return INSAR_OK;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = scene_blocks(n_crossings, TR_THREADS);
  int* ometa = scratch_at<int>(scratch, L.ometa);
  hipLaunchKernelGGL(contour_scatter_kernel, dim3(grid), dim3(TR_THREADS), 0, s, (const int*)scratch_at<int>(scratch, L.lead),
                     (const int*)scratch_at<int>(scratch, L.headof), (const int2*)scratch_at<int2>(scratch, L.p1),
                     (const int2*)scratch_at<int2>(scratch, L.p0), (const int2*)scratch_at<int2>(scratch, L.vert), n_crossings, ometa,
                     reinterpret_cast<int2*>(vertices));
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(contour_reduce_kernel, dim3(grid), dim3(TR_THREADS), 0, s, (const int2*)reinterpret_cast<int2*>(vertices),
                     (const int*)ometa, n_crossings, (InsarContourLine*)table, max_lines);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
