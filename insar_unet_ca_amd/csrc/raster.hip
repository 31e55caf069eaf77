// Polygon rasterisation: an edge table (X0, Y0, X1, Y1, value) in 1/256 pixel becomes a label map [H][W], uint8 or int32, by
// the top-left rule in exact integers. Semantics: include/insar_hip.h, "polygon rasterisation". A CROSSING is a pair (edge,
// row) with min(Y0, Y1) <= 256 row + 128 < max(Y0, Y1); it adds w (+1 for an edge that runs up, -1 down) to `cover` and
// w * value to `vsum` of every pixel of the row from column c0 on, c0 = ceil((Xi - 128) / 256) with Xi the edge's intercept on
// the row's centre line, clamped to 0 .. W. A BAND is R consecutive rows, R = rs_band_rows(W) a power of two.
//
//   clear   the band counters and the overlap counter
//   count   per edge: its crossings per band, added to the band counters
//   scan    one work-group: exclusive prefix sum of the band counters: every band's slice of the record array
//   emit    per edge and crossed row: the record (row in band, c0, w, value) at the band's cursor
//   fill    one work-group per band: two int32 LDS planes [R][P] (cover, vsum) cleared, the band's records added with LDS
//           atomics, an inclusive prefix sum along every row, the pixel decided and stored four at a time
//
// Five launches whatever the table holds, no work-group waits on another, no read-back. The order of the records inside a
// band is arbitrary; they are only ever summed, in integers, so the map is bitwise reproducible. Memory safety does not rest
// on the caller's crossing count: no record is written at or past `cap`, fill reads none there and ignores a record whose
// row or column lies outside its planes.
#include "scene_common.h"
#include "block_scan.h"

#define RS_THREADS 256
#define RS_FILL_THREADS 1024
#define RS_FILL_WAVES (RS_FILL_THREADS / INSAR_WAVE)
#define RS_MAX_W 16384
#define RS_MAX_R 32
#define RS_LDS_BYTES (136 * 1024)          // both planes of a band; 8 * (16384 + 4) bytes at the widest scene
#define RS_LONG 64                         // an edge with more rows (emit) or bands (count) than this is shared by its wave
#define RS_MAX_CROSS ((int64_t)1 << 30)
#define RS_MAX_EDGES (1 << 28)

static_assert(RS_FILL_WAVES == 16, "teams of 16 / min(R, 16) waves per row in rs_fill_kernel");
static_assert(8 * ((RS_MAX_W + 1 + 3) & ~3) <= RS_LDS_BYTES, "one row of the widest scene fits");

// record: x = c0 (15 bits) | row in band << 15 (5 bits) | (w > 0) << 20, y = value
__device__ __forceinline__ int2 rs_record(int c0, int rin, int up, int value) { return make_int2(c0 | (rin << 15) | (up << 20), value); }

__host__ __device__ __forceinline__ int rs_pitch(int W) { return (W + 1 + 3) & ~3; }
static inline int rs_band_rows(int W) {
  int R = RS_MAX_R;
  while (R > 1 && (int64_t)R * rs_pitch(W) * 8 > RS_LDS_BYTES) R >>= 1;
  return R;
}

// rows r0 <= r < r1 of [0, H) whose centre line the edge crosses (half-open in Y); returns r1 - r0, 0 for none
__device__ __forceinline__ int rs_rows(int ya, int yb, int H, int* r0, int* r1) {
  const int lo = min(ya, yb), hi = max(ya, yb);
  const int64_t a = ((int64_t)lo + 127) >> 8, b = ((int64_t)hi + 127) >> 8;       // ceil((Y - 128) / 256)
  const int s = (int)max(a, (int64_t)0), e = (int)min(b, (int64_t)H);
  *r0 = s; *r1 = e;
  return e > s ? e - s : 0;
}
// first column the crossing of (xa, ya) - (xb, yb), ya < yb, with row r affects, clamped to 0 .. W
__device__ __forceinline__ int rs_c0(int xa, int ya, int xb, int yb, int r, int W) {
  int64_t q;
  if (xa == xb) {
    q = ((int64_t)xa + 127) >> 8;
  } else {
    const int64_t dy = (int64_t)yb - ya, D = dy * 256;
    const int64_t num = ((int64_t)xa - 128) * dy + ((int64_t)xb - xa) * ((int64_t)r * 256 + 128 - ya);
    q = num / D;
    if (q * D < num) ++q;                                                            // the ceiling, D > 0
  }
  return (int)min(max(q, (int64_t)0), (int64_t)W);
}

struct RsEdge { int xa, ya, xb, yb, value, up, r0, r1, n; };
// edge e of the table in canonical order (ya < yb); n = 0 for e >= n_edges, a horizontal edge or one that crosses no row
__device__ __forceinline__ RsEdge rs_load(const int* __restrict__ edges, int e, int n_edges, int H) {
  RsEdge g = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (e >= n_edges) return g;
  const int* p = edges + (int64_t)e * 5;
  const int x0 = p[0], y0 = p[1], x1 = p[2], y1 = p[3];
  g.value = p[4];
  if (y0 == y1) return g;
  g.up = y1 < y0;
  if (g.up) { g.xa = x1; g.ya = y1; g.xb = x0; g.yb = y0; }
  else { g.xa = x0; g.ya = y0; g.xb = x1; g.yb = y1; }
  g.n = rs_rows(y0, y1, H, &g.r0, &g.r1);
  return g;
}

__global__ void __launch_bounds__(RS_THREADS)
raster_clear_kernel(int* __restrict__ cnt, int nb, unsigned long long* __restrict__ overlap) {
  const int64_t i0 = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (i0 == 0) *overlap = 0ull;
  for (int64_t i = i0; i <= nb; i += (int64_t)gridDim.x * RS_THREADS) cnt[i] = 0;
}

__global__ void __launch_bounds__(RS_THREADS)
raster_count_kernel(const int* __restrict__ edges, int n_edges, int H, int lgR, int* __restrict__ cnt) {
  const int e = blockIdx.x * RS_THREADS + threadIdx.x, lane = (int)__lane_id(), R = 1 << lgR;
  const RsEdge g = rs_load(edges, e, n_edges, H);
  const int b0 = g.r0 >> lgR, b1 = g.n ? (g.r1 - 1) >> lgR : b0 - 1;               // bands b0 .. b1
  const bool wide = b1 - b0 >= RS_LONG;
  if (!wide)
    for (int b = b0; b <= b1; ++b) atomicAdd(&cnt[b], (int)(min((int64_t)g.r1, ((int64_t)b + 1) * R) - max((int64_t)g.r0, (int64_t)b * R)));
  unsigned long long m = __ballot(wide);
  while (m) {                                                                         // wave-uniform
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int r0 = __shfl(g.r0, src, INSAR_WAVE), r1 = __shfl(g.r1, src, INSAR_WAVE);
    const int last = (r1 - 1) >> lgR;
    for (int b = (r0 >> lgR) + lane; b <= last; b += INSAR_WAVE)
      atomicAdd(&cnt[b], (int)(min((int64_t)r1, ((int64_t)b + 1) * R) - max((int64_t)r0, (int64_t)b * R)));
  }
}

// One work-group: cnt[0 .. nb) becomes its exclusive prefix sum, cnt[nb] the total; cur[] a copy for the cursors.
__global__ void __launch_bounds__(RS_FILL_THREADS)
raster_scan_kernel(int* __restrict__ cnt, int* __restrict__ cur, int nb) {
  __shared__ int ws[RS_FILL_WAVES];
  const int carry = block_scan_array<RS_FILL_THREADS>(cnt, nb, ws);                  // base + threadIdx.x < 2^31: nb <= 2^31 - 1024
  for (int i = threadIdx.x; i < nb; i += RS_FILL_THREADS) cur[i] = cnt[i];           // every thread copies what it wrote itself
  if (threadIdx.x == 0) cnt[nb] = carry;
}

__global__ void __launch_bounds__(RS_THREADS)
raster_emit_kernel(const int* __restrict__ edges, int n_edges, int H, int W, int lgR, int* __restrict__ cur, int2* __restrict__ rec,
                   int cap) {
  const int e = blockIdx.x * RS_THREADS + threadIdx.x, lane = (int)__lane_id(), R = 1 << lgR;
  const RsEdge g = rs_load(edges, e, n_edges, H);
  const bool tall = g.n > RS_LONG;
  if (!tall) {
    for (int r = g.r0; r < g.r1;) {                                                   // one atomic per band the edge touches
      const int b = r >> lgR, end = (int)min((int64_t)g.r1, ((int64_t)b + 1) * R);
      int pos = atomicAdd(&cur[b], end - r);
      for (; r < end; ++r, ++pos)
        if ((unsigned)pos < (unsigned)cap) rec[pos] = rs_record(rs_c0(g.xa, g.ya, g.xb, g.yb, r, W), r & (R - 1), g.up, g.value);
    }
  }
  unsigned long long m = __ballot(tall);
  while (m) {                                                                         // wave-uniform: the wave shares a tall edge
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int xa = __shfl(g.xa, src, INSAR_WAVE), ya = __shfl(g.ya, src, INSAR_WAVE), xb = __shfl(g.xb, src, INSAR_WAVE),
              yb = __shfl(g.yb, src, INSAR_WAVE), value = __shfl(g.value, src, INSAR_WAVE), up = __shfl(g.up, src, INSAR_WAVE),
              r0 = __shfl(g.r0, src, INSAR_WAVE), r1 = __shfl(g.r1, src, INSAR_WAVE);
    for (int64_t rbase = r0; rbase < r1; rbase += INSAR_WAVE) {
      const int64_t r64 = rbase + lane;
      const bool act = r64 < r1;
      const int r = act ? (int)r64 : 0;
      const int band = act ? r >> lgR : -1;
      const WaveRuns runs = wave_runs(band);                                          // a run: the lanes of one band
      const unsigned long long heads = __ballot(runs.head);
      const unsigned long long upto = (2ull << lane) - 1ull;                          // lane 63: 2 << 63 wraps to 0, all ones
      const int first = 63 - __clzll((long long)(heads & upto));
      const unsigned long long above = heads & ~upto;
      const int end = above ? __ffsll((long long)above) - 1 : INSAR_WAVE;
      int pos = 0;
      if (runs.head && act) pos = atomicAdd(&cur[band], end - first);
      pos = __shfl(pos, first, INSAR_WAVE) + (lane - first);
      if (act && (unsigned)pos < (unsigned)cap) rec[pos] = rs_record(rs_c0(xa, ya, xb, yb, r, W), r & (R - 1), up, value);
    }
  }
}

template <typename T> struct RsOut;
template <> struct RsOut<uint8_t> {
  __device__ __forceinline__ static bool fits(int v) { return (unsigned)v <= 255u; }
  __device__ __forceinline__ static void load4(const uint8_t* p, bool vec, int n, int* v) { quad_load_u8(p, 0, n, vec, 0, v); }
  __device__ __forceinline__ static void store4(uint8_t* p, bool vec, int n, const int* v) {
    if (vec) {
      *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) p[j] = (uint8_t)v[j];
    }
  }
};
template <> struct RsOut<int> {
  __device__ __forceinline__ static bool fits(int) { return true; }
  __device__ __forceinline__ static void load4(const int* p, bool vec, int n, int* v) { quad_load(p, 0, n, vec, 0, v); }
  __device__ __forceinline__ static void store4(int* p, bool vec, int n, const int* v) { quad_store(p, 0, n, vec, v); }
};

// One work-group per band. Rows are shared out to TEAMS of `tw` = 16 / min(R, 16) waves: a team walks its row in chunks of
// tw * 256 columns, four per lane; a chunk's prefix is lane-local, then a wave scan, then the sums of the team's earlier waves
// (through `ws`, double-buffered by chunk parity: one barrier per chunk) and the carry of the chunks before. Every loop count
// is uniform over the work-group.
template <typename T>
__global__ void __launch_bounds__(RS_FILL_THREADS)
raster_fill_kernel(const int2* __restrict__ rec, const int* __restrict__ start, int cap, int H, int W, int lgR, int fill, int ov,
                   const T* __restrict__ base, T* __restrict__ out, int vec, int bvec, unsigned long long* __restrict__ overlap) {
  extern __shared__ int4 rs_lds[];
  __shared__ int2 ws[2][RS_FILL_WAVES];
  const int R = 1 << lgR, P = rs_pitch(W), plane = R * P;
  int* cover = reinterpret_cast<int*>(rs_lds);
  int* vsum = cover + plane;
  const int tid = threadIdx.x, lane = tid & (INSAR_WAVE - 1), wave = tid / INSAR_WAVE;
  const int band = blockIdx.x;

  for (int i = tid; i < plane / 2; i += RS_FILL_THREADS) rs_lds[i] = make_int4(0, 0, 0, 0);    // 2 * plane ints, plane % 4 == 0
  __syncthreads();
  const int n0 = max(min(start[band], cap), 0), n1 = min(start[band + 1], cap);      // never outside rec[0 .. cap)
  for (int i = n0 + tid; i < n1; i += RS_FILL_THREADS) {
    const int2 q = rec[i];
    const int c0 = q.x & 0x7fff, rin = (q.x >> 15) & 31, w = ((q.x >> 20) & 1) ? 1 : -1;
    if (c0 <= W && rin < R) {
      atomicAdd(&cover[rin * P + c0], w);
      atomicAdd(&vsum[rin * P + c0], w > 0 ? q.y : (int)(0u - (uint32_t)q.y));
    }
  }
  __syncthreads();

  const int teams = R < RS_FILL_WAVES ? R : RS_FILL_WAVES, tw = RS_FILL_WAVES / teams;
  const int team = wave / tw, wt = wave - team * tw;
  const int span = tw * INSAR_WAVE * 4, chunks = (W + span - 1) / span;
  int voided = 0, par = 0;
  for (int rb = 0; rb < R; rb += teams) {
    const int rin = rb + team;                                                        // < R: R is a multiple of `teams`
    const int64_t row = (int64_t)band * R + rin;
    const bool live = row < H;
    int carry_c = 0, carry_v = 0;
    for (int ch = 0; ch < chunks; ++ch, par ^= 1) {
      const int c = ch * span + (wt * INSAR_WAVE + lane) * 4;
      int4 a = make_int4(0, 0, 0, 0), s = a;
      if (c < P) {                                                                    // P % 4 == 0: the whole quad lies in the row
        a = *reinterpret_cast<const int4*>(cover + rin * P + c);
        s = *reinterpret_cast<const int4*>(vsum + rin * P + c);
      }
      a.y += a.x; a.z += a.y; a.w += a.z;
      s.y += s.x; s.z += s.y; s.w += s.z;
      const int ic = wave_incl_scan(a.w, lane), iv = wave_incl_scan(s.w, lane);
      if (lane == INSAR_WAVE - 1) ws[par][wave] = make_int2(ic, iv);
      __syncthreads();
      int oc = carry_c, ovs = carry_v;
      for (int j = 0; j < tw; ++j) {
        const int2 t = ws[par][team * tw + j];
        if (j < wt) { oc += t.x; ovs += t.y; }
        carry_c += t.x; carry_v += t.y;
      }
      oc += ic - a.w; ovs += iv - s.w;                                                // exclusive over the lanes before this one
      if (live && c < W) {
        const int n = min(4, W - c);
        const int64_t gi = row * W + c;
        const int cv[4] = {oc + a.x, oc + a.y, oc + a.z, oc + a.w}, sv[4] = {ovs + s.x, ovs + s.y, ovs + s.z, ovs + s.w};
        int px[4] = {fill, fill, fill, fill};
        if (base) RsOut<T>::load4(base + gi, bvec && n == 4, n, px);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (cv[j] == 0 && sv[j] == 0) continue;                                     // background: fill, or the base pixel
          if (cv[j] == 1 && RsOut<T>::fits(sv[j]) && sv[j] != ov) px[j] = sv[j];
          else { px[j] = ov; voided += j < n; }
        }
        RsOut<T>::store4(out + gi, vec && n == 4, n, px);
      }
    }
  }
#pragma unroll
  for (int d = INSAR_WAVE / 2; d > 0; d >>= 1) voided += __shfl_xor(voided, d, INSAR_WAVE);
  if (lane == 0 && voided) atomicAdd(overlap, (unsigned long long)voided);
}

// ---------------------------------------------------------------------------------------------
// host side: scratch layout and the entry points
// ---------------------------------------------------------------------------------------------
struct RsLayout {
  int R, lgR, nb, cap;
  int64_t cnt, cur, rec, bytes;
};

static int raster_layout(const char* who, int32_t H, int32_t W, int64_t max_crossings, RsLayout* L) {
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  if (W > RS_MAX_W) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene width %d above %d", who, W, RS_MAX_W);
  if ((int64_t)H * W >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^31 pixels or more", who, H, W);
  if (max_crossings < 0 || max_crossings > RS_MAX_CROSS)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_crossings %lld outside 0 .. 2^30", who, (long long)max_crossings);
  L->R = rs_band_rows(W);
  L->lgR = 0;
  while ((1 << L->lgR) < L->R) ++L->lgR;
  L->nb = (int)(((int64_t)H + L->R - 1) / L->R);
  L->cap = (int)max_crossings;
  ScratchTake take;
  L->cnt = take(((int64_t)L->nb + 1) * 4);
  L->cur = take((int64_t)L->nb * 4);
  L->rec = take((max_crossings > 0 ? max_crossings : 1) * 8);
  L->bytes = take.at;
  return INSAR_OK;
}

extern "C" int insar_raster_band_rows(int32_t W) {
  if (W < 1 || W > RS_MAX_W) INSAR_FAIL(INSAR_E_SHAPE, "insar_raster_band_rows: scene width %d outside 1 .. %d", W, RS_MAX_W);
  return rs_band_rows(W);
}

extern "C" int insar_raster_launches(void) { return 5; }

extern "C" int insar_raster_scratch_bytes(int32_t H, int32_t W, int64_t max_crossings, int64_t* scratch_bytes) {
  const char* who = "insar_raster_scratch_bytes";
  if (!scratch_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  RsLayout L;
  if (int rc = raster_layout(who, H, W, max_crossings, &L)) return rc;
  *scratch_bytes = L.bytes;
  return INSAR_OK;
}

template <typename T>
static int raster_fill(const char* who, const RsLayout& L, void* scratch, int32_t H, int32_t W, int32_t fill, int32_t ov,
                       const void* base, void* out, int64_t* overlap, hipStream_t s) {
  static std::atomic<uint64_t> attr_mask{0};     // per-device, see common.h
  const int lds = 8 * L.R * rs_pitch(W);
  hipError_t e = insar_set_lds_once(attr_mask, (const void*)raster_fill_kernel<T>, RS_LDS_BYTES);
  if (e != hipSuccess) INSAR_FAIL(-(int)e, "%s: hipFuncSetAttribute(%d bytes LDS): %s", who, RS_LDS_BYTES, hipGetErrorString(e));
  const uintptr_t amask = sizeof(T) * 4 - 1;     // four pixels: a dword of uint8, 16 bytes of int32
  const int vec = W % 4 == 0 && (((uintptr_t)out) & amask) == 0, bvec = W % 4 == 0 && base && (((uintptr_t)base) & amask) == 0;
  hipLaunchKernelGGL(raster_fill_kernel<T>, dim3((unsigned)L.nb), dim3(RS_FILL_THREADS), (size_t)lds, s,
                     (const int2*)((char*)scratch + L.rec), (const int*)((char*)scratch + L.cnt), L.cap, H, W, L.lgR, fill, ov,
                     (const T*)base, (T*)out, vec, bvec, reinterpret_cast<unsigned long long*>(overlap));
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_raster_polygons(const int32_t* edges, int32_t n_edges, int32_t H, int32_t W, int64_t max_crossings,
                                     int32_t elem_type, int32_t fill, int32_t overlap_value, const void* base, void* out,
                                     void* scratch, int64_t* overlap_pixels, void* stream) {
  const char* who = "insar_raster_polygons";
  RsLayout L;
  if (int rc = raster_layout(who, H, W, max_crossings, &L)) return rc;
  if (n_edges < 0 || n_edges > RS_MAX_EDGES) INSAR_FAIL(INSAR_E_SHAPE, "%s: n_edges %d outside 0 .. 2^28", who, n_edges);
  if (elem_type != INSAR_RASTER_U8 && elem_type != INSAR_RASTER_I32) INSAR_FAIL(INSAR_E_DTYPE, "%s: element type %d", who, elem_type);
  if (elem_type == INSAR_RASTER_U8 && (fill < 0 || fill > 255 || overlap_value < 0 || overlap_value > 255))
    INSAR_FAIL(INSAR_E_ARG, "%s: fill %d / overlap_value %d outside 0 .. 255 of a uint8 map", who, fill, overlap_value);
  if (!out || !scratch || !overlap_pixels || (!edges && n_edges > 0)) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (!insar_aligned16(scratch)) INSAR_FAIL(INSAR_E_ALIGN, "%s: scratch not 16-byte aligned", who);
  if (((uintptr_t)overlap_pixels) & 7u) INSAR_FAIL(INSAR_E_ALIGN, "%s: overlap_pixels not 8-byte aligned", who);
  if (((uintptr_t)edges) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: edges not 4-byte aligned", who);
  if (elem_type == INSAR_RASTER_I32 && ((((uintptr_t)out) | ((uintptr_t)base)) & 3u))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: int32 map not 4-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  int *cnt = (int*)((char*)scratch + L.cnt), *cur = (int*)((char*)scratch + L.cur);
  int2* rec = (int2*)((char*)scratch + L.rec);
  const unsigned egrid = (unsigned)((n_edges + RS_THREADS - 1) / RS_THREADS);
  hipLaunchKernelGGL(raster_clear_kernel, dim3((unsigned)insar_grid_cap(((int64_t)L.nb + RS_THREADS) / RS_THREADS)), dim3(RS_THREADS), 0,
                     s, cnt, L.nb, reinterpret_cast<unsigned long long*>(overlap_pixels));
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(raster_count_kernel, dim3(egrid ? egrid : 1u), dim3(RS_THREADS), 0, s, edges, n_edges, H, L.lgR, cnt);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(raster_scan_kernel, dim3(1), dim3(RS_FILL_THREADS), 0, s, cnt, cur, L.nb);
  INSAR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(raster_emit_kernel, dim3(egrid ? egrid : 1u), dim3(RS_THREADS), 0, s, edges, n_edges, H, W, L.lgR, cur, rec, L.cap);
  INSAR_CHECK_LAUNCH(who);
  if (elem_type == INSAR_RASTER_U8) return raster_fill<uint8_t>(who, L, scratch, H, W, fill, overlap_value, base, out, overlap_pixels, s);
  return raster_fill<int>(who, L, scratch, H, W, fill, overlap_value, base, out, overlap_pixels, s);
}
