// Training from whole scenes: class-balanced crops drawn on the device. A label map uint8 [H][W] is reduced once per scene
// to a table int32 [K + 1][Hc + 1][Wc + 1] of per-class pixel counts of g x g cells (cells), turned in place into its
// exclusive 2-D prefix sums (sat); after that the count of any cell-aligned rectangle costs four lookups per plane. Every
// batch then takes two launches: draw (one wave per sample, lane t evaluates try t against the table) and gather (the
// image tiles, normalised as insar_scene_gather does, and the label tiles at the drawn origins).
//
// All arithmetic that decides anything is integer, nothing is read back, there are no atomics: every output is bitwise
// defined (tests/crops_ref.py restates it). Plane p < K counts label p; plane K counts the void pixels: label 255 and
// every other label >= K.
#include "scene_common.h"

// nothing below is meant to fuse (the image path of gather, image_quad of scene_common.h, turns contraction off by itself)
#pragma clang fp contract(off)

#define CR_THREADS 256
#define CR_MAX_K 8
#define CR_MAX_TRIES 64
#define CR_SCAN_WAVES 16

// ---------------------------------------------------------------------------------------------
// cells
// ---------------------------------------------------------------------------------------------
struct CropTable {
  int32_t* t;
  int K, Hc, Wc;
  __device__ __forceinline__ int64_t pitch() const { return (int64_t)Wc + 1; }
  __device__ __forceinline__ int64_t plane() const { return ((int64_t)Hc + 1) * pitch(); }
};

// cnt[p] = pixels of the cell with label p (p < 8, whatever K is) -> planes 0..K-1, and the rest of the cell to plane K
__device__ __forceinline__ void crops_store_cell(const CropTable& tb, int i, int j, const int* cnt, int area) {
  const int64_t at = ((int64_t)i + 1) * tb.pitch() + 1 + j;
  int known = 0;
#pragma unroll
  for (int p = 0; p < CR_MAX_K; ++p) {
    if (p < tb.K) {
      tb.t[p * tb.plane() + at] = cnt[p];
      known += cnt[p];
    }
  }
  tb.t[tb.K * tb.plane() + at] = area - known;
}

// row 0 and column 0 of every plane
__device__ __forceinline__ void crops_zero_borders(const CropTable& tb) {
  const int64_t rim = (int64_t)tb.Hc + 1 + tb.Wc + 1;
  const int64_t nwork = (tb.K + 1) * rim;
  for (int64_t w = blockIdx.x * (int64_t)CR_THREADS + threadIdx.x; w < nwork; w += (int64_t)gridDim.x * CR_THREADS) {
    const int p = (int)(w / rim);
    const int64_t e = w % rim;
    const int64_t at = e <= tb.Wc ? e : (e - (tb.Wc + 1)) * tb.pitch();
    tb.t[p * tb.plane() + at] = 0;
  }
}

// G in {1, 2, 4, 8, 16}, W % 16 == 0 and a 16-byte aligned map: a thread owns the 16 / G cells of one cell row that share
// a 16-byte run of pixels and reads each of their G pixel rows with one 16-byte load
template <int G>
__global__ void __launch_bounds__(CR_THREADS) crops_cells_vec_kernel(const uint8_t* __restrict__ lab, int W, CropTable tb) {
  constexpr int CPT = 16 / G;
  const int tpr = (tb.Wc + CPT - 1) / CPT;                   // threads per cell row; 16 * tpr <= W (W % 16 == 0)
  const int64_t nwork = (int64_t)tb.Hc * tpr;
  for (int64_t w = blockIdx.x * (int64_t)CR_THREADS + threadIdx.x; w < nwork; w += (int64_t)gridDim.x * CR_THREADS) {
    const int i = (int)(w / tpr), t = (int)(w % tpr);
    uint32_t px[G][4];
#pragma unroll
    for (int r = 0; r < G; ++r) {
      const uint4 v = *reinterpret_cast<const uint4*>(lab + ((int64_t)i * G + r) * W + 16 * (int64_t)t);
      px[r][0] = v.x; px[r][1] = v.y; px[r][2] = v.z; px[r][3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int j = t * CPT + c;
      if (j >= tb.Wc) continue;
      int cnt[CR_MAX_K] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < G; ++r) {
#pragma unroll
        for (int b = 0; b < G; ++b) {
          const int at = c * G + b;
          const uint32_t v = (px[r][at >> 2] >> (8 * (at & 3))) & 0xffu;
#pragma unroll
          for (int p = 0; p < CR_MAX_K; ++p) cnt[p] += (v == (uint32_t)p);
        }
      }
      crops_store_cell(tb, i, j, cnt, G * G);
    }
  }
  crops_zero_borders(tb);
}

// any g, any pitch, any alignment: one thread per cell, byte loads (adjacent lanes read adjacent cells)
__global__ void __launch_bounds__(CR_THREADS) crops_cells_kernel(const uint8_t* __restrict__ lab, int W, int g, CropTable tb) {
  const int64_t nwork = (int64_t)tb.Hc * tb.Wc;
  for (int64_t w = blockIdx.x * (int64_t)CR_THREADS + threadIdx.x; w < nwork; w += (int64_t)gridDim.x * CR_THREADS) {
    const int i = (int)(w / tb.Wc), j = (int)(w % tb.Wc);
    int cnt[CR_MAX_K] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < g; ++r) {
      const uint8_t* row = lab + ((int64_t)i * g + r) * W + (int64_t)j * g;
      for (int b = 0; b < g; ++b) {
        const uint32_t v = row[b];
#pragma unroll
        for (int p = 0; p < CR_MAX_K; ++p) cnt[p] += (v == (uint32_t)p);
      }
    }
    crops_store_cell(tb, i, j, cnt, g * g);
  }
  crops_zero_borders(tb);
}

static int crops_check_scene(const char* who, int32_t K, int32_t g, int32_t H, int32_t W) {
  if (K < 2 || K > CR_MAX_K) INSAR_FAIL(INSAR_E_SHAPE, "%s: num_classes %d outside 2..%d", who, K, CR_MAX_K);
  if (g < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: cell size %d below 1", who, g);
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  if ((int64_t)H * W >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^31 pixels or more", who, H, W);
  if (g > H || g > W) INSAR_FAIL(INSAR_E_SHAPE, "%s: cell size %d above the scene %d x %d", who, g, H, W);
  return INSAR_OK;
}

static int crops_check_tile(const char* who, int32_t T, int32_t g, int32_t H, int32_t W) {
  if (T < 1 || T % g != 0) INSAR_FAIL(INSAR_E_SHAPE, "%s: tile %d is not a positive multiple of the cell size %d", who, T, g);
  if (T > H || T > W) INSAR_FAIL(INSAR_E_SHAPE, "%s: tile %d above the scene %d x %d", who, T, H, W);
  return INSAR_OK;
}

extern "C" int insar_crops_cells(const uint8_t* labels, int32_t H, int32_t W, int32_t K, int32_t g, int32_t* table, void* stream) {
  const char* who = "insar_crops_cells";
  if (!labels || !table) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !labels ? "labels" : "table");
  if (int rc = crops_check_scene(who, K, g, H, W)) return rc;
  if (((uintptr_t)table) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 4-byte aligned", who);
  CropTable tb;
  tb.t = table; tb.K = K; tb.Hc = H / g; tb.Wc = W / g;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = (g == 1 || g == 2 || g == 4 || g == 8 || g == 16) && W % 16 == 0 && insar_aligned16(labels);
  if (vec) {
    const int cpt = 16 / g;
    const int64_t nwork = (int64_t)tb.Hc * ((tb.Wc + cpt - 1) / cpt);
    const dim3 grid(insar_grid_cap((nwork + CR_THREADS - 1) / CR_THREADS, 1 << 16)), block(CR_THREADS);
    switch (g) {
      case 1: hipLaunchKernelGGL(crops_cells_vec_kernel<1>, grid, block, 0, s, labels, W, tb); break;
      case 2: hipLaunchKernelGGL(crops_cells_vec_kernel<2>, grid, block, 0, s, labels, W, tb); break;
      case 4: hipLaunchKernelGGL(crops_cells_vec_kernel<4>, grid, block, 0, s, labels, W, tb); break;
      case 8: hipLaunchKernelGGL(crops_cells_vec_kernel<8>, grid, block, 0, s, labels, W, tb); break;
      default: hipLaunchKernelGGL(crops_cells_vec_kernel<16>, grid, block, 0, s, labels, W, tb); break;
    }
  } else {
    const int64_t nwork = (int64_t)tb.Hc * tb.Wc;
    hipLaunchKernelGGL(crops_cells_kernel, dim3(insar_grid_cap((nwork + CR_THREADS - 1) / CR_THREADS, 1 << 16)), dim3(CR_THREADS), 0, s,
                       labels, W, g, tb);
  }
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// sat: the inclusive 2-D scan of the table WITH its zero row 0 and column 0 is the exclusive scan of the cells. Two
// launches: along the rows (a wave per row, 64 entries at a time, the carry in a register), then down the columns (a
// work-group per 64 adjacent columns of a plane, lane = column so that every access is a 256-byte run of a row; its 16 waves
// own consecutive row segments, sum them, exchange the 16 segment totals through LDS and scan their segment with the
// totals of the segments above as the carry). int32 adds in any order give one result: exact for any Hc, Wc.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CR_THREADS) crops_scan_rows_kernel(int32_t* __restrict__ table, int64_t nrows, int64_t pitch) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)CR_THREADS + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * CR_THREADS) >> 6;
  for (int64_t row = wave; row < nrows; row += nwaves) {              // wave-uniform: every shuffle below has 64 lanes
    int32_t* p = table + row * pitch;
    int32_t carry = 0;
    for (int64_t c0 = 0; c0 < pitch; c0 += 64) {
      const int64_t c = c0 + lane;
      const int32_t v = wave_incl_scan(c < pitch ? p[c] : 0, lane) + carry;
      if (c < pitch) p[c] = v;
      carry = __shfl(v, 63, 64);
    }
  }
}

__global__ void __launch_bounds__(CR_SCAN_WAVES * 64)
crops_scan_cols_kernel(int32_t* __restrict__ table, int64_t rows, int64_t pitch, int colgroups) {
  __shared__ int32_t tot[CR_SCAN_WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.x / colgroups, cg = blockIdx.x % colgroups;
  const int64_t col = (int64_t)cg * 64 + lane;
  const bool in = col < pitch;
  int32_t* base = table + p * rows * pitch + col;
  const int64_t seg = (rows + CR_SCAN_WAVES - 1) / CR_SCAN_WAVES;
  const int64_t r0 = wv * seg, r1 = r0 + seg < rows ? r0 + seg : rows;
  int32_t s = 0;
  if (in)
    for (int64_t r = r0; r < r1; ++r) s += base[r * pitch];
  tot[wv][lane] = s;
  __syncthreads();
  int32_t carry = 0;
  for (int k = 0; k < wv; ++k) carry += tot[k][lane];
  if (in) {
    for (int64_t r = r0; r < r1; ++r) {
      carry += base[r * pitch];
      base[r * pitch] = carry;
    }
  }
}

extern "C" int insar_crops_sat(int32_t* table, int32_t K, int32_t Hc, int32_t Wc, void* stream) {
  const char* who = "insar_crops_sat";
  if (!table) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (table)", who);
  if (K < 2 || K > CR_MAX_K) INSAR_FAIL(INSAR_E_SHAPE, "%s: num_classes %d outside 2..%d", who, K, CR_MAX_K);
  if (Hc < 1 || Wc < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty table %d x %d cells", who, Hc, Wc);
  if (((int64_t)Hc + 1) * ((int64_t)Wc + 1) >= ((int64_t)1 << 31))
    INSAR_FAIL(INSAR_E_SHAPE, "%s: a plane of %d x %d cells has 2^31 entries or more", who, Hc, Wc);
  if (((uintptr_t)table) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 4-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)Hc + 1, pitch = (int64_t)Wc + 1, nrows = (K + 1) * rows;
  hipLaunchKernelGGL(crops_scan_rows_kernel, dim3(insar_grid_cap((nrows + 3) / 4, 1 << 16)), dim3(CR_THREADS), 0, s, table, nrows, pitch);
  INSAR_CHECK_LAUNCH(who);
  const int colgroups = (int)((pitch + 63) / 64);
  hipLaunchKernelGGL(crops_scan_cols_kernel, dim3((K + 1) * colgroups), dim3(CR_SCAN_WAVES * 64), 0, s, table, rows, pitch, colgroups);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// draw: one wave per sample, lane t evaluates try t. The rule is stated in include/insar_hip.h; its aug_hash64 is insar_hash64
// of scene_common.h.
// ---------------------------------------------------------------------------------------------
struct CropCum { float c[CR_MAX_K]; };

__global__ void __launch_bounds__(CR_THREADS)
crops_draw_kernel(uint64_t key, int n, int K, int tries, CropCum cum, int min_count, int max_void, int tg, int g, int Hc, int Wc,
                  const int32_t* __restrict__ sat, int32_t* __restrict__ origins, int32_t* __restrict__ info) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (CR_THREADS / 64) + (threadIdx.x >> 6);
  if (s >= n) return;                                                // wave-uniform
  const uint64_t b = (uint64_t)s * 65ull;
  const float u = (float)(insar_hash64(key, b) >> 40) * 0x1p-24f;
  int cls = K - 1;
#pragma unroll
  for (int c = CR_MAX_K - 2; c >= 0; --c)
    if (c < K - 1 && u < cum.c[c]) cls = c;                          // descending: the first such c stays
  const bool act = lane < tries;
  const uint64_t r = insar_hash64(key, b + 1ull + (uint64_t)lane);
  const uint64_t ny = (uint64_t)(Hc - tg + 1), nx = (uint64_t)(Wc - tg + 1);
  const int cy = (int)(((r >> 32) * ny) >> 32), cx = (int)(((r & 0xffffffffull) * nx) >> 32);
  const int64_t pitch = (int64_t)Wc + 1, plane = ((int64_t)Hc + 1) * pitch;
  int cnt = 0, vd = 0;
  if (act) {
    const int64_t a00 = cy * pitch + cx, a01 = a00 + tg, a10 = a00 + tg * pitch, a11 = a10 + tg;      // cy + tg <= Hc, cx + tg <= Wc
    const int32_t* sc = sat + cls * plane;
    const int32_t* sv = sat + K * plane;
    cnt = sc[a11] - sc[a01] - sc[a10] + sc[a00];
    vd = sv[a11] - sv[a01] - sv[a10] + sv[a00];
  }
  const bool capped = act && vd <= max_void;
  const unsigned long long accepted = __ballot(capped && cnt >= min_count);
  int win, acc;
  if (accepted) {
    win = __ffsll(accepted) - 1;
    acc = win;
  } else {
    // most target pixels among the tries within the void cap, else fewest void pixels; 63 - lane in the low byte: ties to
    // the lowest try. Lane 0 is always a try, so the second key is never all zero.
    unsigned long long best = wave_max(capped ? (((unsigned long long)cnt + 1ull) << 8) | (unsigned)(63 - lane) : 0ull);
    if (best == 0ull)
      best = wave_max(act ? ((0x80000000ull - (unsigned long long)vd) << 8) | (unsigned)(63 - lane) : 0ull);
    win = 63 - (int)(best & 0xffull);
    acc = -1;
  }
  const int oy = __shfl(cy * g, win, 64), ox = __shfl(cx * g, win, 64);
  const int wc = __shfl(cnt, win, 64), wvd = __shfl(vd, win, 64);
  if (lane == 0) {
    origins[2 * (int64_t)s] = oy;
    origins[2 * (int64_t)s + 1] = ox;
    int32_t* o = info + 4 * (int64_t)s;
    o[0] = cls; o[1] = acc; o[2] = wc; o[3] = wvd;
  }
}

extern "C" int insar_crops_draw(uint64_t key, int32_t n, int32_t K, int32_t tries, const float* cum, int32_t min_count,
                                int32_t max_void, int32_t T, int32_t g, int32_t H, int32_t W, const int32_t* sat, int32_t* origins,
                                int32_t* info, void* stream) {
  const char* who = "insar_crops_draw";
  if (!cum || !sat || !origins || !info)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !cum ? "cum" : !sat ? "sat" : !origins ? "origins" : "info");
  if (int rc = crops_check_scene(who, K, g, H, W)) return rc;
  if (int rc = crops_check_tile(who, T, g, H, W)) return rc;
  if (tries < 1 || tries > CR_MAX_TRIES) INSAR_FAIL(INSAR_E_ARG, "%s: tries %d outside 1..%d", who, tries, CR_MAX_TRIES);
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: n = %d samples", who, n);
  if ((((uintptr_t)sat) | ((uintptr_t)origins) | ((uintptr_t)info)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: sat, origins or info not 4-byte aligned", who);
  CropCum c;
  for (int k = 0; k < CR_MAX_K; ++k) c.c[k] = k < K ? cum[k] : 0.f;
  const int wpb = CR_THREADS / 64;
  hipLaunchKernelGGL(crops_draw_kernel, dim3((n + wpb - 1) / wpb), dim3(CR_THREADS), 0, (hipStream_t)stream, key, n, K, tries, c,
                     min_count, max_void, T / g, g, H / g, W / g, sat, origins, info);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

// ---------------------------------------------------------------------------------------------
// gather: one launch for the image tiles and the label tiles of a batch. One thread per four adjacent output pixels
// (T % 4 == 0: a quad never leaves its tile row); the first n * T * T / 4 work items are image quads, the rest label quads,
// so a wave is of one kind except at the one boundary. The image arithmetic is image_quad of scene_common.h, the one that
// insar_scene_gather runs. A tile whose origin leaves the scene (no table insar_crops_draw writes holds one) is zero-filled,
// its labels are 255.
// ---------------------------------------------------------------------------------------------
template <typename S, int MD>
__global__ void __launch_bounds__(CR_THREADS)
crops_gather_kernel(const S* __restrict__ scene, const uint8_t* __restrict__ labels, int H, int W, const int32_t* __restrict__ origins,
                    int n, int T, float* __restrict__ images, void* __restrict__ masks) {
  const int qrow = T >> 2;
  const int64_t nquads = (int64_t)n * T * qrow;
  const int64_t nimg = images ? nquads : 0;
  const int64_t nwork = nimg + (MD != INSAR_AUG_MASK_NONE ? nquads : 0);
  for (int64_t w = blockIdx.x * (int64_t)CR_THREADS + threadIdx.x; w < nwork; w += (int64_t)gridDim.x * CR_THREADS) {
    const bool is_img = w < nimg;
    const int64_t q = is_img ? w : w - nimg;
    const int tx = (int)(q % qrow) << 2;
    const int64_t r = q / qrow;
    const int ty = (int)(r % T);
    const int t = (int)(r / T);
    const int y0 = origins[2 * t], x0 = origins[2 * t + 1];
    const bool inside = y0 >= 0 && x0 >= 0 && y0 + T <= H && x0 + T <= W;
    const int64_t at = (int64_t)(y0 + ty) * W + x0 + tx;
    if (is_img) {
      float f[4] = {0.f, 0.f, 0.f, 0.f};
      if (inside) image_quad<S>(scene + at, f);
      *reinterpret_cast<float4*>(images + (q << 2)) = make_float4(f[0], f[1], f[2], f[3]);
    } else if constexpr (MD != INSAR_AUG_MASK_NONE) {
      const uint32_t u = inside ? load4_u8_any(labels + at) : 0xffffffffu;
      if constexpr (MD == INSAR_AUG_MASK_U8) {
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(masks) + (q << 2)) = u;
      } else {
        labels4_store_i64(reinterpret_cast<int64_t*>(masks) + (q << 2), u);
      }
    }
  }
}

template <typename S>
static void crops_gather_launch(int md, dim3 grid, hipStream_t s, const void* scene, const uint8_t* labels, int H, int W,
                                const int32_t* origins, int n, int T, float* images, void* masks) {
  const dim3 block(CR_THREADS);
  const S* sc = (const S*)scene;
  if (md == INSAR_AUG_MASK_U8)
    hipLaunchKernelGGL((crops_gather_kernel<S, INSAR_AUG_MASK_U8>), grid, block, 0, s, sc, labels, H, W, origins, n, T, images, masks);
  else if (md == INSAR_AUG_MASK_I64)
    hipLaunchKernelGGL((crops_gather_kernel<S, INSAR_AUG_MASK_I64>), grid, block, 0, s, sc, labels, H, W, origins, n, T, images, masks);
  else
    hipLaunchKernelGGL((crops_gather_kernel<S, INSAR_AUG_MASK_NONE>), grid, block, 0, s, sc, labels, H, W, origins, n, T, images, masks);
}

extern "C" int insar_crops_gather(const void* scene, int32_t scene_dtype, const uint8_t* labels, int32_t H, int32_t W,
                                  const int32_t* origins, int32_t n, int32_t T, float* images, void* masks, int32_t mask_dtype,
                                  void* stream) {
  const char* who = "insar_crops_gather";
  if (!origins) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (origins)", who);
  if (!images && !masks) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (neither images nor masks)", who);
  if (images && !scene) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (scene, with images asked for)", who);
  if (masks && !labels) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (labels, with masks asked for)", who);
  if (images && scene_dtype != INSAR_SCENE_U8 && scene_dtype != INSAR_SCENE_F32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: scene dtype %d (uint8 or float32)", who, scene_dtype);
  if (masks && mask_dtype != INSAR_AUG_MASK_U8 && mask_dtype != INSAR_AUG_MASK_I64)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: mask dtype %d (uint8 or int64)", who, mask_dtype);
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty scene %d x %d", who, H, W);
  if ((int64_t)H * W >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: scene %d x %d has 2^31 pixels or more", who, H, W);
  if (T < 4 || T % 4) INSAR_FAIL(INSAR_E_SHAPE, "%s: tile %d is not a positive multiple of 4", who, T);
  if (T > H || T > W) INSAR_FAIL(INSAR_E_SHAPE, "%s: tile %d above the scene %d x %d", who, T, H, W);
  if (n < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: n = %d tiles", who, n);
  if (((uintptr_t)origins) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: origins not 4-byte aligned", who);
  if (images && !insar_aligned16(images)) INSAR_FAIL(INSAR_E_ALIGN, "%s: images not 16-byte aligned", who);
  if (images && scene_dtype == INSAR_SCENE_F32 && (((uintptr_t)scene) & 3u)) INSAR_FAIL(INSAR_E_ALIGN, "%s: float32 scene not 4-byte aligned", who);
  if (masks && (mask_dtype == INSAR_AUG_MASK_I64 ? !insar_aligned16(masks) : (((uintptr_t)masks) & 3u) != 0))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: masks not aligned (int64: 16 bytes, uint8: 4 bytes)", who);
  const int md = masks ? mask_dtype : INSAR_AUG_MASK_NONE;
  const int64_t nquads = (int64_t)n * T * (T / 4) * ((images ? 1 : 0) + (masks ? 1 : 0));
  const dim3 grid(insar_grid_cap((nquads + CR_THREADS - 1) / CR_THREADS));
  hipStream_t s = (hipStream_t)stream;
  if (images && scene_dtype == INSAR_SCENE_F32) crops_gather_launch<float>(md, grid, s, scene, labels, H, W, origins, n, T, images, masks);
  else crops_gather_launch<uint8_t>(md, grid, s, scene, labels, H, W, origins, n, T, images, masks);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
