// Grey-scale morphological reconstruction of a raster [planes][H][W] with the no-data rules of the scene tools: the pointwise
// limit of J <- min(G, max of J over the pixel and its 4 or 8 neighbours) from J = min(F, G), on order-preserving 32-bit keys of
// the raw values. fill_sinks, h_dome and regional_extrema are this one operation with a marker derived in the prepare kernel.
//
// Keys: float32 hysteresis.ordered_u32 (-0.0 directly below 0.0), int32 with the sign bit flipped, uint8 as it is. Reconstruction
// by erosion is reconstruction by dilation of the complemented keys (`flip`). An invalid pixel (and a pixel outside the raster)
// has the mask key 0, the minimum: it never rises and never raises a neighbour, so the propagation has no special case for it.
//
//   prepare   rc_prepare_kernel: one thread per pixel. Writes the mask keys G and the start J = min(F, G) (the derived markers:
//             outlets, raster -/+ h, key - 1), sets every tile active and clears the counters of the call's rounds.
//   round     rc_round_kernel: one work-group of 256 threads per RC_T x RC_T tile of one plane (planes on grid z). It stages its J
//             tile with a one-pixel halo and its G tile in LDS (pitches 67 and 65 words: neither a row walk nor a column walk has
//             a bank conflict), solves the tile to its LOCAL fixed point with the halo held fixed, writes the interior to the
//             other J buffer and records whether anything changed. The solver is four directional sweeps by the first wave: a
//             lane owns a row (left to right, right to left) or a column (down, up; at connectivity 8 the three pixels of the row
//             behind join, the two outer ones by a wave shuffle); the four sweeps repeat until one pass changes nothing. J only
//             rises and is bounded by G, so the loop ends; it is capped at the tile's pixel count anyway.
//             The J plane ping-pongs between two buffers: no work-group reads what another writes in the same launch; no atomics
//             on pixel data; no work-group waits on another. A tile is active in round r + 1 iff it or one of its 8 neighbours
//             changed in round r (the activity map ping-pongs too). An inactive tile is skipped: it did not change in the round
//             before, so its tile is the same in both J buffers.
//   finish    rc_finish_kernel: keys back to values, the residue, the extrema map, `fill` / NaN at invalid pixels, the valid plane.
//
// The fixed point is unique, so nothing here depends on the schedule: the outputs are bitwise defined, and so is the number of
// rounds (tests/reconstruct_ref.py restates both).
#include "scene_common.h"

#define RC_THREADS 256
#define RC_T 64                          // tile edge
#define RC_PJ 67                         // pitch of the staged J tile with its halo (RC_T + 2 columns), odd
#define RC_PG 65                         // pitch of the staged G tile, odd
#define RC_MAX_ROUNDS INSAR_RECONSTRUCT_MAX_ROUNDS
#define RC_MAX_PLANES 65535
#define RC_QNAN 0x7fc00000u
#define RC_COUNTER_BYTES (8 * ((int64_t)RC_MAX_ROUNDS + 1))

static_assert(RC_COUNTER_BYTES % 16 == 0, "the counter pairs end the scratch without padding");
static_assert(RC_T == INSAR_WAVE, "one lane of the first wave per tile row / column");
static_assert(RC_PJ >= RC_T + 2 && (RC_PJ & 1) && (RC_PG & 1) && RC_PG >= RC_T, "odd pitches: conflict-free row walks");

enum { RC_PLAIN = INSAR_RECONSTRUCT_PLAIN, RC_FILL = INSAR_RECONSTRUCT_FILL, RC_HDOME = INSAR_RECONSTRUCT_HDOME,
       RC_EXTREMA = INSAR_RECONSTRUCT_EXTREMA };

// ---- per element type: validity, the order key and its inverse, the marker raster -/+ h, the residue ---------------------------
template <typename T> struct RcElem;
template <> struct RcElem<float> {
  typedef float Residue;
  __device__ __forceinline__ static bool mask_ok(float v, bool has_nodata, double nodata) {
    return fabsf(v) <= 3.402823466e38f && !(has_nodata && v == (float)nodata);
  }
  __device__ __forceinline__ static bool marker_ok(float v, bool has_nodata, double nodata) {      // +-inf is a marker
    return v == v && !(has_nodata && v == (float)nodata);
  }
  __device__ __forceinline__ static uint32_t key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
  }
  __device__ __forceinline__ static float from_key(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
  __device__ __forceinline__ static float shifted(float v, double h, bool up) {
#pragma clang fp contract(off)
    return up ? v + (float)h : v - (float)h;
  }
  __device__ __forceinline__ static float residue(float hi, float lo) {
#pragma clang fp contract(off)
    return hi - lo;
  }
  __device__ __forceinline__ static float invalid(int) { return __uint_as_float(RC_QNAN); }
  __device__ __forceinline__ static float invalid_residue() { return __uint_as_float(RC_QNAN); }
};
template <> struct RcElem<int> {
  typedef int Residue;
  __device__ __forceinline__ static bool mask_ok(int v, bool has_nodata, double nodata) { return !(has_nodata && v == (int)nodata); }
  __device__ __forceinline__ static bool marker_ok(int v, bool has_nodata, double nodata) { return mask_ok(v, has_nodata, nodata); }
  __device__ __forceinline__ static uint32_t key(int v) { return (uint32_t)v ^ 0x80000000u; }
  __device__ __forceinline__ static int from_key(uint32_t k) { return (int)(k ^ 0x80000000u); }
  __device__ __forceinline__ static int shifted(int v, double h, bool up) {
    const long long s = (long long)v + (up ? (long long)h : -(long long)h);
    return (int)(s > 2147483647ll ? 2147483647ll : s < -2147483648ll ? -2147483648ll : s);
  }
  __device__ __forceinline__ static int residue(int hi, int lo) {
    const long long d = (long long)hi - (long long)lo;
    return (int)(d > 2147483647ll ? 2147483647ll : d);
  }
  __device__ __forceinline__ static int invalid(int fill) { return fill; }
  __device__ __forceinline__ static int invalid_residue() { return 0; }
};
template <> struct RcElem<uint8_t> {
  typedef int Residue;
  __device__ __forceinline__ static bool mask_ok(uint8_t v, bool has_nodata, double nodata) { return !(has_nodata && (int)v == (int)nodata); }
  __device__ __forceinline__ static bool marker_ok(uint8_t v, bool has_nodata, double nodata) { return mask_ok(v, has_nodata, nodata); }
  __device__ __forceinline__ static uint32_t key(uint8_t v) { return (uint32_t)v; }
  __device__ __forceinline__ static uint8_t from_key(uint32_t k) { return (uint8_t)k; }
  __device__ __forceinline__ static uint8_t shifted(uint8_t v, double h, bool up) {
    const long long s = (long long)v + (up ? (long long)h : -(long long)h);
    return (uint8_t)(s > 255 ? 255 : s < 0 ? 0 : s);
  }
  __device__ __forceinline__ static int residue(uint8_t hi, uint8_t lo) { return (int)hi - (int)lo; }
  __device__ __forceinline__ static uint8_t invalid(int fill) { return (uint8_t)fill; }
  __device__ __forceinline__ static int invalid_residue() { return 0; }
};

struct RcArgs {
  const void* marker;                    // RC_PLAIN only
  const void* mask;
  const uint8_t* valid;
  uint32_t* J;                           // prepare: the start plane; finish: the plane of the last round
  uint32_t* G;
  void* out;
  void* residue;
  uint8_t* extrema;
  uint8_t* out_valid;
  uint8_t* act;                          // prepare: the activity map round 0 reads
  int* counters;
  int64_t n_act;
  int n_counters;                        // prepare: the int32 words of the counter pairs of rounds 0 .. max_rounds
  int H, W, conn, mode, flip, has_nodata, fill;
  double nodata, h;
};

// validity of pixel (y, x) of the plane whose mask is `mask` and whose marker (nullable) is `marker`; outside is invalid
template <typename T>
__device__ __forceinline__ bool rc_valid_at(const RcArgs& a, const T* mask, const T* marker, int y, int x) {
  if (y < 0 || y >= a.H || x < 0 || x >= a.W) return false;
  const int64_t p = (int64_t)y * a.W + x;
  if (a.valid && a.valid[p] == 0) return false;
  if (!RcElem<T>::mask_ok(mask[p], a.has_nodata != 0, a.nodata)) return false;
  return !marker || RcElem<T>::marker_ok(marker[p], a.has_nodata != 0, a.nodata);
}

template <typename T>
__global__ void __launch_bounds__(RC_THREADS)
rc_prepare_kernel(RcArgs a) {
  const int64_t npix = (int64_t)a.H * a.W;
  const int64_t gid = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (blockIdx.z == 0) {                 // every tile active in round 0; the (changed, active) counters of the call's rounds at 0
    const int64_t step = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t i = gid; i < a.n_act; i += step) a.act[i] = 1;
    for (int64_t i = gid; i < a.n_counters; i += step) a.counters[i] = 0;
  }
  if (gid >= npix) return;
  const int y = (int)(gid / a.W), x = (int)(gid - (int64_t)y * a.W);
  const int64_t plane = (int64_t)blockIdx.z * npix;
  const T* mask = reinterpret_cast<const T*>(a.mask) + plane;
  const T* marker = a.mode == RC_PLAIN ? reinterpret_cast<const T*>(a.marker) + plane : nullptr;
  const uint32_t flip = a.flip ? 0xffffffffu : 0u;
  uint32_t g = 0u, j = 0u;
  if (rc_valid_at<T>(a, mask, marker, y, x)) {
    const T v = mask[gid];
    g = RcElem<T>::key(v) ^ flip;
    if (a.mode == RC_PLAIN) {
      j = RcElem<T>::key(marker[gid]) ^ flip;
    } else if (a.mode == RC_FILL) {      // the raster at outlets, the lowest key elsewhere
      bool outlet = false;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
          if ((dy || dx) && (a.conn == 8 || !(dy && dx))) outlet = outlet || !rc_valid_at<T>(a, mask, nullptr, y + dy, x + dx);
      j = outlet ? g : 0u;
    } else if (a.mode == RC_HDOME) {
      j = RcElem<T>::key(RcElem<T>::shifted(v, a.h, a.flip != 0)) ^ flip;
    } else {
      j = g ? g - 1u : 0u;
    }
    j = j < g ? j : g;
  }
  a.G[plane + gid] = g;
  a.J[plane + gid] = j;
}

// ---- the local solver's sweeps: wave 0 only, all 64 lanes; true if a pixel rose ----------------------------------------------------
__device__ __forceinline__ bool rc_sweep_row(uint32_t* sj, const uint32_t* sg, int lane, bool forward) {
  uint32_t* row = sj + (lane + 1) * RC_PJ;
  const uint32_t* g = sg + lane * RC_PG;
  bool ch = false;
  uint32_t v = row[forward ? 0 : RC_T + 1];
  for (int i = 0; i < RC_T; ++i) {
    const int x = forward ? i : RC_T - 1 - i;
    const uint32_t j = row[x + 1];
    const uint32_t m = j > v ? j : v;
    const uint32_t n = m < g[x] ? m : g[x];
    if (n != j) { row[x + 1] = n; ch = true; }
    v = n;
  }
  return ch;
}
template <int CONN>
__device__ __forceinline__ bool rc_sweep_col(uint32_t* sj, const uint32_t* sg, int lane, bool down) {
  bool ch = false;
  uint32_t v = sj[(down ? 0 : RC_T + 1) * RC_PJ + lane + 1];
  for (int i = 0; i < RC_T; ++i) {
    const int y = down ? i : RC_T - 1 - i;             // interior row; the row behind is staged row y (down) or y + 2 (up)
    uint32_t m = v;
    if (CONN == 8) {
      const int behind = (down ? y : y + 2) * RC_PJ;
      uint32_t l = __shfl_up(v, 1, INSAR_WAVE), r = __shfl_down(v, 1, INSAR_WAVE);
      if (lane == 0) l = sj[behind];
      if (lane == RC_T - 1) r = sj[behind + RC_T + 1];
      l = l > r ? l : r;
      m = m > l ? m : l;
    }
    const uint32_t j = sj[(y + 1) * RC_PJ + lane + 1];
    const uint32_t g = sg[y * RC_PG + lane];
    m = j > m ? j : m;
    const uint32_t n = m < g ? m : g;
    if (n != j) { sj[(y + 1) * RC_PJ + lane + 1] = n; ch = true; }
    v = n;
  }
  return ch;
}

struct RcRound {
  const uint32_t* Jin;
  uint32_t* Jout;
  const uint32_t* G;
  const uint8_t* act_in;
  uint8_t* act_out;
  int* counter;                          // [0] tiles that changed in this round, [1] tiles that were active
  int H, W, tiles_x, tiles_y;
};

template <int CONN>
__global__ void __launch_bounds__(RC_THREADS)
rc_round_kernel(RcRound a) {
  __shared__ uint32_t sj[(RC_T + 2) * RC_PJ];
  __shared__ uint32_t sg[RC_T * RC_PG];
  __shared__ int s_flag, s_any;
  const int tid = threadIdx.x;
  const int tile = (int)blockIdx.x;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int64_t tbase = (int64_t)blockIdx.z * a.tiles_x * a.tiles_y;

  bool active = false;                   // uniform over the work-group
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = ty + dy, xx = tx + dx;
      if (yy >= 0 && yy < a.tiles_y && xx >= 0 && xx < a.tiles_x) active = active || a.act_in[tbase + (int64_t)yy * a.tiles_x + xx] != 0;
    }
  if (!active) {
    if (tid == 0) a.act_out[tbase + tile] = 0;
    return;
  }

  const int y0 = ty * RC_T, x0 = tx * RC_T;
  const int64_t plane = (int64_t)blockIdx.z * a.H * a.W;
  const uint32_t* Jin = a.Jin + plane;
  const uint32_t* G = a.G + plane;
  for (int idx = tid; idx < (RC_T + 2) * (RC_T + 2); idx += RC_THREADS) {
    const int sy = idx / (RC_T + 2), sx = idx - sy * (RC_T + 2);
    const int gy = y0 - 1 + sy, gx = x0 - 1 + sx;
    const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    sj[sy * RC_PJ + sx] = in ? Jin[(int64_t)gy * a.W + gx] : 0u;
  }
  for (int idx = tid; idx < RC_T * RC_T; idx += RC_THREADS) {
    const int sy = idx / RC_T, sx = idx - sy * RC_T;
    const int gy = y0 + sy, gx = x0 + sx;
    sg[sy * RC_PG + sx] = (gy < a.H && gx < a.W) ? G[(int64_t)gy * a.W + gx] : 0u;
  }
  if (tid == 0) s_any = 0;

  for (int it = 0; it < RC_T * RC_T; ++it) {
    __syncthreads();                     // the staging (first pass) or the last pass's read of s_flag is behind every thread
    if (tid == 0) s_flag = 0;
    bool ch = false;
    if (tid < INSAR_WAVE) ch = rc_sweep_row(sj, sg, tid, true);
    __syncthreads();
    if (tid < INSAR_WAVE) ch = rc_sweep_row(sj, sg, tid, false) || ch;
    __syncthreads();
    if (tid < INSAR_WAVE) ch = rc_sweep_col<CONN>(sj, sg, tid, true) || ch;
    __syncthreads();
    if (tid < INSAR_WAVE) ch = rc_sweep_col<CONN>(sj, sg, tid, false) || ch;
    if (ch) s_flag = 1;
    __syncthreads();
    if (!s_flag) break;
    if (tid == 0) s_any = 1;
  }
  __syncthreads();

  uint32_t* Jout = a.Jout + plane;
  for (int idx = tid; idx < RC_T * RC_T; idx += RC_THREADS) {
    const int sy = idx / RC_T, sx = idx - sy * RC_T;
    const int gy = y0 + sy, gx = x0 + sx;
    if (gy < a.H && gx < a.W) Jout[(int64_t)gy * a.W + gx] = sj[(sy + 1) * RC_PJ + sx + 1];
  }
  if (tid == 0) {
    const int any = s_any;
    a.act_out[tbase + tile] = (uint8_t)any;
    atomicAdd(&a.counter[1], 1);
    if (any) atomicAdd(&a.counter[0], 1);
  }
}

template <typename T>
__global__ void __launch_bounds__(RC_THREADS)
rc_finish_kernel(RcArgs a) {
  typedef typename RcElem<T>::Residue R;
  const int64_t npix = (int64_t)a.H * a.W;
  const int64_t gid = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (gid >= npix) return;
  const int y = (int)(gid / a.W), x = (int)(gid - (int64_t)y * a.W);
  const int64_t plane = (int64_t)blockIdx.z * npix;
  const T* mask = reinterpret_cast<const T*>(a.mask) + plane;
  const T* marker = a.mode == RC_PLAIN ? reinterpret_cast<const T*>(a.marker) + plane : nullptr;
  const uint32_t flip = a.flip ? 0xffffffffu : 0u;
  const bool ok = rc_valid_at<T>(a, mask, marker, y, x);
  const uint32_t j = a.J[plane + gid];
  const T rec = RcElem<T>::from_key(j ^ flip);
  if (a.out) reinterpret_cast<T*>(a.out)[plane + gid] = ok ? rec : RcElem<T>::invalid(a.fill);
  if (a.residue) {
    const T v = mask[gid];
    reinterpret_cast<R*>(a.residue)[plane + gid] =
        !ok ? RcElem<T>::invalid_residue() : a.flip ? RcElem<T>::residue(rec, v) : RcElem<T>::residue(v, rec);
  }
  if (a.extrema) a.extrema[plane + gid] = (ok && a.G[plane + gid] > j) ? 1 : 0;
  if (a.out_valid) a.out_valid[plane + gid] = ok ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct RcLayout {
  int64_t j0, j1, g, act0, act1, counters, bytes;
  int tiles_x, tiles_y;
  int64_t n_act;
  RcLayout(int32_t planes, int32_t H, int32_t W) {
    ScratchTake take;
    const int64_t plane_bytes = (int64_t)planes * H * W * 4;
    tiles_x = (W + RC_T - 1) / RC_T;
    tiles_y = (H + RC_T - 1) / RC_T;
    n_act = (int64_t)planes * tiles_x * tiles_y;
    j0 = take(plane_bytes);
    j1 = take(plane_bytes);
    g = take(plane_bytes);
    act0 = take(n_act);
    act1 = take(n_act);
    counters = take(RC_COUNTER_BYTES);                     // the LAST piece: the host reads it at bytes - RC_COUNTER_BYTES
    bytes = take.at;
  }
};

static int rc_check_shape(const char* who, int32_t planes, int32_t H, int32_t W) {
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty raster %d x %d", who, H, W);
  if ((int64_t)H * W >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: raster %d x %d has 2^31 pixels or more", who, H, W);
  if (planes < 1 || planes > RC_MAX_PLANES) INSAR_FAIL(INSAR_E_SHAPE, "%s: planes %d outside 1..%d", who, planes, RC_MAX_PLANES);
  return INSAR_OK;
}
static int rc_check_maps(const char* who, const void* marker, const void* mask, int32_t elem_type, int32_t mode, int32_t flip,
                         int32_t has_nodata, double nodata, const void* scratch) {
  if (elem_type != INSAR_ZONAL_F32 && elem_type != INSAR_ZONAL_U8 && elem_type != INSAR_ZONAL_I32)
    INSAR_FAIL(INSAR_E_DTYPE, "%s: element type %d", who, elem_type);
  if (mode < RC_PLAIN || mode > RC_EXTREMA) INSAR_FAIL(INSAR_E_ARG, "%s: mode %d", who, mode);
  if (flip != 0 && flip != 1) INSAR_FAIL(INSAR_E_ARG, "%s: flip %d: 0 or 1", who, flip);
  const unsigned align = elem_type == INSAR_ZONAL_U8 ? 1u : 4u;
  if (int rc = scene_check_map(who, "mask", mask, align)) return rc;
  if (mode == RC_PLAIN) {
    if (int rc = scene_check_map(who, "marker", marker, align)) return rc;
  } else if (marker) {
    INSAR_FAIL(INSAR_E_ARG, "%s: a marker with mode %d (the marker is derived from the mask)", who, mode);
  }
  if (has_nodata && nodata != nodata) INSAR_FAIL(INSAR_E_ARG, "%s: nodata is NaN", who);
  if (has_nodata && elem_type != INSAR_ZONAL_F32 && (nodata != (double)(int64_t)nodata || nodata < -2147483648.0 || nodata > 2147483647.0))
    INSAR_FAIL(INSAR_E_ARG, "%s: nodata %g is no value of an integer raster", who, nodata);
  return scene_check_buffer(who, "scratch", scratch);
}
static inline dim3 rc_pixel_grid(int32_t planes, int32_t H, int32_t W) {
  return dim3((unsigned)(((int64_t)H * W + RC_THREADS - 1) / RC_THREADS), 1, (unsigned)planes);      // < 2^23 blocks
}

extern "C" int insar_reconstruct_tile(int32_t* edge) {
  if (!edge) INSAR_FAIL(INSAR_E_ARG, "insar_reconstruct_tile: null pointer");
  *edge = RC_T;
  return INSAR_OK;
}

extern "C" int insar_reconstruct_bytes(int32_t planes, int32_t H, int32_t W, int64_t* scratch_bytes) {
  const char* who = "insar_reconstruct_bytes";
  if (!scratch_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  if (int rc = rc_check_shape(who, planes, H, W)) return rc;
  *scratch_bytes = RcLayout(planes, H, W).bytes;
  return INSAR_OK;
}

extern "C" int insar_reconstruct_prepare(const void* marker, const void* mask, int32_t elem_type, int32_t planes, int32_t H, int32_t W,
                                         int32_t mode, int32_t flip, int32_t connectivity, double h, int32_t max_rounds, int32_t has_nodata,
                                         double nodata, const uint8_t* valid, void* scratch, void* stream) {
  const char* who = "insar_reconstruct_prepare";
  if (int rc = rc_check_shape(who, planes, H, W)) return rc;
  if (int rc = rc_check_maps(who, marker, mask, elem_type, mode, flip, has_nodata, nodata, scratch)) return rc;
  if (connectivity != 4 && connectivity != 8) INSAR_FAIL(INSAR_E_ARG, "%s: connectivity %d: 4 or 8", who, connectivity);
  if (max_rounds < 1 || max_rounds > RC_MAX_ROUNDS) INSAR_FAIL(INSAR_E_ARG, "%s: max_rounds %d outside 1..%d", who, max_rounds, RC_MAX_ROUNDS);
  if (mode == RC_HDOME) {
    if (!(h > 0.0) || !(h <= 1.7976931348623157e308)) INSAR_FAIL(INSAR_E_ARG, "%s: h %g: positive and finite", who, h);
    if (elem_type == INSAR_ZONAL_F32 && (!((float)h > 0.0f) || !((float)h <= 3.402823466e38f)))
      INSAR_FAIL(INSAR_E_ARG, "%s: h %g is not positive and finite in float32", who, h);
    if (elem_type != INSAR_ZONAL_F32 && (h != (double)(int64_t)h || h > 2147483647.0))
      INSAR_FAIL(INSAR_E_ARG, "%s: h %g: an integer in 1..2^31 - 1 for an integer raster", who, h);
  }
  const RcLayout L(planes, H, W);
  RcArgs a = {};
  a.marker = marker; a.mask = mask; a.valid = valid;
  a.J = scratch_at<uint32_t>(scratch, L.j0); a.G = scratch_at<uint32_t>(scratch, L.g);
  a.act = scratch_at<uint8_t>(scratch, L.act0); a.counters = scratch_at<int>(scratch, L.counters); a.n_act = L.n_act;
  a.n_counters = 2 * (max_rounds + 1);
  a.H = H; a.W = W; a.conn = connectivity; a.mode = mode; a.flip = flip; a.has_nodata = has_nodata;
  a.nodata = nodata; a.h = h;
  const dim3 grid = rc_pixel_grid(planes, H, W), block(RC_THREADS);
  if (elem_type == INSAR_ZONAL_F32) hipLaunchKernelGGL(rc_prepare_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
  else if (elem_type == INSAR_ZONAL_U8) hipLaunchKernelGGL(rc_prepare_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rc_prepare_kernel<int>, grid, block, 0, (hipStream_t)stream, a);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_reconstruct_rounds(int32_t planes, int32_t H, int32_t W, int32_t connectivity, int32_t first_round, int32_t n_rounds,
                                        void* scratch, void* stream) {
  const char* who = "insar_reconstruct_rounds";
  if (int rc = rc_check_shape(who, planes, H, W)) return rc;
  if (int rc = scene_check_buffer(who, "scratch", scratch)) return rc;
  if (connectivity != 4 && connectivity != 8) INSAR_FAIL(INSAR_E_ARG, "%s: connectivity %d: 4 or 8", who, connectivity);
  if (first_round < 0 || n_rounds < 1 || (int64_t)first_round + n_rounds > RC_MAX_ROUNDS)
    INSAR_FAIL(INSAR_E_ARG, "%s: rounds %d .. %d + %d outside 0..%d", who, first_round, first_round, n_rounds, RC_MAX_ROUNDS);
  const RcLayout L(planes, H, W);
  uint32_t* J[2] = {scratch_at<uint32_t>(scratch, L.j0), scratch_at<uint32_t>(scratch, L.j1)};
  uint8_t* act[2] = {scratch_at<uint8_t>(scratch, L.act0), scratch_at<uint8_t>(scratch, L.act1)};
  const dim3 grid((unsigned)(L.tiles_x * L.tiles_y), 1, (unsigned)planes), block(RC_THREADS);
  for (int r = first_round; r < first_round + n_rounds; ++r) {     // round r reads buffer r & 1 and writes the other
    RcRound a;
    a.Jin = J[r & 1]; a.Jout = J[(r + 1) & 1]; a.G = scratch_at<uint32_t>(scratch, L.g);
    a.act_in = act[r & 1]; a.act_out = act[(r + 1) & 1];
    a.counter = scratch_at<int>(scratch, L.counters) + 2 * r;
    a.H = H; a.W = W; a.tiles_x = L.tiles_x; a.tiles_y = L.tiles_y;
    if (connectivity == 8) hipLaunchKernelGGL(rc_round_kernel<8>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(rc_round_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
    INSAR_CHECK_LAUNCH(who);
  }
  return INSAR_OK;
}

extern "C" int insar_reconstruct_finish(const void* marker, const void* mask, int32_t elem_type, int32_t planes, int32_t H, int32_t W,
                                        int32_t mode, int32_t flip, int32_t has_nodata, double nodata, const uint8_t* valid,
                                        int32_t rounds_run, int32_t fill, void* scratch, void* out, void* residue, uint8_t* extrema,
                                        uint8_t* out_valid, void* stream) {
  const char* who = "insar_reconstruct_finish";
  if (int rc = rc_check_shape(who, planes, H, W)) return rc;
  if (int rc = rc_check_maps(who, marker, mask, elem_type, mode, flip, has_nodata, nodata, scratch)) return rc;
  if (rounds_run < 0 || rounds_run > RC_MAX_ROUNDS) INSAR_FAIL(INSAR_E_ARG, "%s: rounds_run %d outside 0..%d", who, rounds_run, RC_MAX_ROUNDS);
  if (elem_type == INSAR_ZONAL_U8 && (fill < 0 || fill > 255)) INSAR_FAIL(INSAR_E_ARG, "%s: fill %d is no uint8 value", who, fill);
  if (!out && !residue && !extrema && !out_valid) INSAR_FAIL(INSAR_E_ARG, "%s: no output", who);
  if (out == mask || (marker && out == marker)) INSAR_FAIL(INSAR_E_ARG, "%s: out is the mask or the marker itself", who);
  if ((elem_type != INSAR_ZONAL_U8 && (((uintptr_t)out) & 3u)) || (((uintptr_t)residue) & 3u))
    INSAR_FAIL(INSAR_E_ALIGN, "%s: out / residue not 4-byte aligned", who);
  const RcLayout L(planes, H, W);
  RcArgs a = {};
  a.marker = marker; a.mask = mask; a.valid = valid;
  a.J = scratch_at<uint32_t>(scratch, (rounds_run & 1) ? L.j1 : L.j0); a.G = scratch_at<uint32_t>(scratch, L.g);
  a.out = out; a.residue = residue; a.extrema = extrema; a.out_valid = out_valid;
  a.H = H; a.W = W; a.mode = mode; a.flip = flip; a.has_nodata = has_nodata; a.fill = fill;
  a.nodata = nodata;
  const dim3 grid = rc_pixel_grid(planes, H, W), block(RC_THREADS);
  if (elem_type == INSAR_ZONAL_F32) hipLaunchKernelGGL(rc_finish_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
  else if (elem_type == INSAR_ZONAL_U8) hipLaunchKernelGGL(rc_finish_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rc_finish_kernel<int>, grid, block, 0, (hipStream_t)stream, a);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
