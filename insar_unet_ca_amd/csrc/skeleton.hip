// Centre lines: Guo and Hall's two-subiteration parallel thinning of every region of a label map int32 [H][W] at once, the kind
// of every skeleton pixel and the per-region accumulators a table of linear features is made of (include/insar_hip.h,
// "centre lines"). Integers only, no read-back, no work-group waits on another; the number of launches is a function of
// max_iterations alone: 1 (planes) + ceil(max_iterations / SK_T) (steps) + 1 (stats).
//
// Layout: bit planes. One 64-bit word holds 64 consecutive pixels of a row (bit x % 64 of word x / 64; Ww = ceil(W / 64) words
// per row, the bits past W are 0). Ten planes of H * Ww words: the alive map twice (ping-pong between launches) and EIGHT link
// planes, one per neighbour direction p2 .. p9, ALIGNED AT THE PIXEL: bit p of link k says "the neighbour k of p is inside the
// image and carries p's positive label". The issue's four planes (E, S, SE, SW) hold the same information in half the bytes, but
// each of W, N, NW, NE is then a shifted read of a neighbouring word of a neighbouring row; the aligned planes cost 0.5 byte per
// pixel more and make "neighbour k is set" one AND: p_k = alive shifted by direction k & link k, for 64 pixels at once. The
// deletion rule is boolean algebra on those eight words (sk_delete).
//
//   planes  one wave per word: every lane compares its pixel's label with its eight neighbours', nine ballots give the alive word
//           and the eight link words. The same launch clears the table and the iteration flags.
//   step    one work-group of 1024 threads per tile, one thread per staged word: SK_RH = 128 rows x SK_RW = 8 words, of which the
//           inner SK_TH = 96 rows x SK_TW = 6 words (384 pixels) are the tile and the rest is halo: 2 SK_T = 16 rows above and
//           below, one word (64 pixels >= 16) left and right. A sub-iteration looks one pixel away, so whatever is wrong at the
//           rim of the staged area (its outside reads as 0) moves inwards one pixel per sub-iteration and after SK_T = 8
//           iterations has not reached the tile. The alive words ping-pong between two LDS buffers with a zero border (2 x 130 x
//           10 x 8 = 20 800 bytes); the thread keeps its eight link words in registers. The loop leaves early when an iteration
//           deleted nothing in the whole staged area (every further one would be a no-op there). A tile in whose 3 x 3 tile
//           neighbourhood the previous launch deleted nothing copies its words through: a change outside that neighbourhood is
//           at least 96 pixels away and travels two pixels per iteration. Every launch writes the whole alive map.
//           iterflag[i] is set by whoever deletes a TILE pixel in iteration i (never a halo pixel: those may be wrong).
//   stats   one wave per word: the neighbour words once more, then per lane the kind, the link counts and the moments; runs of
//           equal labels are folded over the wave (wave_runs) before one set of agent-scope integer atomics per run. Waves
//           without a skeleton pixel write zeros and go on. Integer adds commute: the table is bitwise reproducible.
#include "scene_common.h"

#define SK_T 8
#define SK_HALO (2 * SK_T)
#define SK_RW 8
#define SK_RH 128
#define SK_TW (SK_RW - 2)
#define SK_TH (SK_RH - 2 * SK_HALO)
#define SK_THREADS (SK_RW * SK_RH)
#define SK_ST_THREADS 256
#define SK_MAX_DIM 32767
#define SK_MAX_ITER 32768

static_assert(SK_THREADS == 1024, "one thread per staged word");
static_assert(SK_HALO <= 64 && SK_TH >= 2 * SK_T && 64 * SK_TW >= 2 * SK_T, "halo within one word; copy-through needs a tile >= 2 T");
static_assert(sizeof(InsarSkeletonStat) == 80, "InsarSkeletonStat is 80 bytes: five 16-byte stores clear a record");

// ---- the rule on words --------------------------------------------------------------------------------------------------------
struct SkNb { uint64_t p2, p3, p4, p5, p6, p7, p8, p9; };

// a[j][i]: the alive word of row y - 1 + j, word w - 1 + i; L[k]: link plane k (p2 .. p9) of (y, w)
__device__ __forceinline__ SkNb sk_neighbours(const uint64_t (&a)[3][3], const uint64_t* L) {
  SkNb n;
  const uint64_t e0 = (a[0][1] >> 1) | (a[0][2] << 63), w0 = (a[0][1] << 1) | (a[0][0] >> 63);
  const uint64_t e1 = (a[1][1] >> 1) | (a[1][2] << 63), w1 = (a[1][1] << 1) | (a[1][0] >> 63);
  const uint64_t e2 = (a[2][1] >> 1) | (a[2][2] << 63), w2 = (a[2][1] << 1) | (a[2][0] >> 63);
  n.p2 = a[0][1] & L[0]; n.p3 = e0 & L[1]; n.p4 = e1 & L[2]; n.p5 = e2 & L[3];
  n.p6 = a[2][1] & L[4]; n.p7 = w2 & L[5]; n.p8 = w1 & L[6]; n.p9 = w0 & L[7];
  return n;
}
__device__ __forceinline__ uint64_t sk_ge2(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }
// the pixels of `alive` that sub-iteration `sub` (0, 1) deletes
__device__ __forceinline__ uint64_t sk_delete(const SkNb& n, uint64_t alive, int sub) {
  const uint64_t c1 = ~n.p2 & (n.p3 | n.p4), c2 = ~n.p4 & (n.p5 | n.p6), c3 = ~n.p6 & (n.p7 | n.p8), c4 = ~n.p8 & (n.p9 | n.p2);
  const uint64_t one = ((c1 ^ c2) ^ (c3 ^ c4)) & ~(c1 & c2) & ~(c3 & c4);                       // C == 1
  const uint64_t a1 = n.p9 | n.p2, a2 = n.p3 | n.p4, a3 = n.p5 | n.p6, a4 = n.p7 | n.p8;       // N1's terms
  const uint64_t b1 = n.p2 | n.p3, b2 = n.p4 | n.p5, b3 = n.p6 | n.p7, b4 = n.p8 | n.p9;       // N2's terms
  // 2 <= min(N1, N2) <= 3: both at least 2, not both 4
  const uint64_t nn = sk_ge2(a1, a2, a3, a4) & sk_ge2(b1, b2, b3, b4) & ~(a1 & a2 & a3 & a4 & b1 & b2 & b3 & b4);
  const uint64_t m = sub == 0 ? (n.p6 | n.p7 | ~n.p9) & n.p8 : (n.p2 | n.p3 | ~n.p5) & n.p4;
  return alive & one & nn & ~m;
}

// ---- planes -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SK_ST_THREADS)
sk_planes_kernel(const int* __restrict__ labels, int H, int W, int Ww, int64_t nw, uint64_t* __restrict__ link,
                 uint64_t* __restrict__ alive, int4* __restrict__ table16, int64_t table_n16, int* __restrict__ iterflag, int max_iter) {
  const int64_t t0 = blockIdx.x * (int64_t)SK_ST_THREADS + threadIdx.x, nt = (int64_t)gridDim.x * SK_ST_THREADS;
  for (int64_t i = t0; i < table_n16; i += nt) table16[i] = make_int4(0, 0, 0, 0);
  for (int64_t i = t0; i < max_iter; i += nt) iterflag[i] = 0;
  const int lane = (int)__lane_id();
  const int64_t wave = __builtin_amdgcn_readfirstlane((int)(t0 >> 6)), nwaves = nt >> 6;
  for (int64_t item = wave; item < nw; item += nwaves) {
    const int y = (int)(item / Ww), x = (int)(item % Ww) * 64 + lane;
    const int c = x < W ? labels[(int64_t)y * W + x] : 0;
    bool s[8];
    const int dy[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, dx[8] = {0, 1, 1, 1, 0, -1, -1, -1};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int yy = y + dy[k], xx = x + dx[k];
      s[k] = c > 0 && yy >= 0 && yy < H && xx >= 0 && xx < W && labels[(int64_t)yy * W + xx] == c;
    }
    const uint64_t a = __ballot(c > 0);
    uint64_t b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = __ballot(s[k]);
    if (lane == 0) {
      alive[item] = a;
#pragma unroll
      for (int k = 0; k < 8; ++k) link[k * nw + item] = b[k];
    }
  }
}

// ---- step ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t sk_sub(const uint64_t (*buf)[SK_RW + 2], int r, int c, const uint64_t* L, uint64_t alive, int sub) {
  uint64_t a[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) a[j][i] = buf[r + j][c + i];                  // the buffer carries a border: (r, c) is (r + 1, c + 1)
  return sk_delete(sk_neighbours(a, L), alive, sub);
}

__global__ void __launch_bounds__(SK_THREADS)
sk_step_kernel(const uint64_t* __restrict__ link, const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, int H, int Ww,
               int64_t nw, int tiles_x, int tiles_y, const int* __restrict__ changed_prev, int* __restrict__ changed_cur,
               int* __restrict__ iterflag, int niter) {
  __shared__ uint64_t buf[2][SK_RH + 2][SK_RW + 2];
  const int tid = (int)threadIdx.x, c = tid & (SK_RW - 1), r = tid / SK_RW;
  const int tile = (int)blockIdx.x, tyi = tile / tiles_x, txi = tile % tiles_x;
  const int gy = tyi * SK_TH - SK_HALO + r, gw = txi * SK_TW - 1 + c;
  const bool inimg = gy >= 0 && gy < H && gw >= 0 && gw < Ww;
  const bool interior = inimg && r >= SK_HALO && r < SK_HALO + SK_TH && c >= 1 && c < SK_RW - 1;
  const int64_t g = inimg ? (int64_t)gy * Ww + gw : 0;
  int near = changed_prev ? 0 : 1;
  if (changed_prev && tid < 9) {
    const int ny = tyi + tid / 3 - 1, nx = txi + tid % 3 - 1;
    if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x) near = changed_prev[ny * tiles_x + nx];
  }
  const int work = __syncthreads_or(near);
  uint64_t a = inimg ? src[g] : 0;
  if (!work) {                                                                 // uniform over the work-group
    if (interior) dst[g] = a;
    if (tid == 0) changed_cur[tile] = 0;
    return;
  }
  uint64_t L[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) L[k] = inimg ? link[k * nw + g] : 0;
  uint64_t* flat = &buf[0][0][0];
  for (int i = tid; i < 2 * (SK_RH + 2) * (SK_RW + 2); i += SK_THREADS) flat[i] = 0;
  __syncthreads();
  buf[0][r + 1][c + 1] = a;
  __syncthreads();
  const int lane = (int)__lane_id();
  int anyint = 0;
  for (int it = 0; it < niter; ++it) {
    const uint64_t d0 = sk_sub(buf[0], r, c, L, a, 0);
    a &= ~d0;
    buf[1][r + 1][c + 1] = a;
    __syncthreads();
    const uint64_t d1 = sk_sub(buf[1], r, c, L, a, 1);
    a &= ~d1;
    buf[0][r + 1][c + 1] = a;
    const int del = (d0 | d1) != 0, idel = del && interior;
    const uint64_t who = __ballot(idel);
    if (who && lane == __ffsll((unsigned long long)who) - 1) iterflag[it] = 1;
    anyint |= idel;
    if (!__syncthreads_or(del)) break;
  }
  if (interior) dst[g] = a;
  const int ch = __syncthreads_or(anyint);
  if (tid == 0) changed_cur[tile] = ch;
}

// ---- stats --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SK_ST_THREADS)
sk_stats_kernel(const int* __restrict__ labels, const int* __restrict__ d2, const uint64_t* __restrict__ link,
                const uint64_t* __restrict__ alive, int H, int W, int Ww, int64_t nw, const int* __restrict__ iterflag, int max_iter,
                int max_regions, InsarSkeletonStat* table, uint8_t* __restrict__ skel) {
  const int lane = (int)__lane_id();
  const int64_t t0 = blockIdx.x * (int64_t)SK_ST_THREADS + threadIdx.x, nt = (int64_t)gridDim.x * SK_ST_THREADS;
  const int64_t wave = __builtin_amdgcn_readfirstlane((int)(t0 >> 6)), nwaves = nt >> 6;
  int lmax = 0;
  for (int64_t item = wave; item < nw; item += nwaves) {
    const int y = (int)(item / Ww), w = (int)(item % Ww), x = w * 64 + lane;
    const bool in = x < W;
    const int64_t p = (int64_t)y * W + x;
    const int lab = in ? labels[p] : 0;
    lmax = max(lmax, lab);
    const uint64_t mine = alive[item];
    if (mine == 0) {                                                           // uniform over the wave
      if (in) skel[p] = 0;
      continue;
    }
    uint64_t a[3][3], L[8];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int yy = y - 1 + j, ww = w - 1 + i;
        a[j][i] = (yy >= 0 && yy < H && ww >= 0 && ww < Ww) ? alive[(int64_t)yy * Ww + ww] : 0;
      }
#pragma unroll
    for (int k = 0; k < 8; ++k) L[k] = link[k * nw + item];
    const SkNb n = sk_neighbours(a, L);
    const bool sk = (mine >> lane) & 1;
    const int b2 = (n.p2 >> lane) & 1, b3 = (n.p3 >> lane) & 1, b4 = (n.p4 >> lane) & 1, b5 = (n.p5 >> lane) & 1;
    const int b6 = (n.p6 >> lane) & 1, b7 = (n.p7 >> lane) & 1, b8 = (n.p8 >> lane) & 1, b9 = (n.p9 >> lane) & 1;
    const int X = (b3 & ~b2) + (b4 & ~b3) + (b5 & ~b4) + (b6 & ~b5) + (b7 & ~b6) + (b8 & ~b7) + (b9 & ~b8) + (b2 & ~b9);
    const int kind = !sk ? 0 : X == 0 ? 1 : X == 1 ? 2 : X == 2 ? 3 : 4;
    if (in) skel[p] = (uint8_t)kind;
    const int key = (sk && lab > 0 && lab <= max_regions) ? lab : 0;          // a label above the capacity is never an index
    const bool on = key > 0;
    const int dv = (on && d2) ? d2[p] : 0;
    const bool far = dv == INSAR_DIST_FAR;
    // six small counts in 10-bit fields of one word: a run has at most 64 pixels and 128 links
    const unsigned long long packed = !on ? 0ull
        : 1ull | ((unsigned long long)(kind == 2) << 10) | ((unsigned long long)(kind == 4) << 20) |
              ((unsigned long long)(b4 + b6) << 30) | ((unsigned long long)((b5 & !b4 & !b6) + (b7 & !b8 & !b6)) << 40) |
              ((unsigned long long)far << 50);
    const WaveRuns runs = wave_runs(key);
    const unsigned long long cnt = wave_run_reduce(runs, packed, WaveAdd());
    const int sx = wave_run_reduce(runs, on ? x : 0, WaveAdd());
    const long long sxx = wave_run_reduce(runs, on ? (long long)x * x : 0ll, WaveAdd());
    const long long sd = wave_run_reduce(runs, far ? 0ll : (long long)dv, WaveAdd());
    const int md = wave_run_reduce(runs, far ? 0 : dv, WaveMax());
    if (runs.head && on) {
      InsarSkeletonStat* r = table + key;
      const int cn = (int)(cnt & 1023), ce = (int)((cnt >> 10) & 1023), cj = (int)((cnt >> 20) & 1023);
      const int co = (int)((cnt >> 30) & 1023), cd = (int)((cnt >> 40) & 1023), cf = (int)((cnt >> 50) & 1023);
      atomicAdd(&r->n, cn);
      if (ce) atomicAdd(&r->n_end, ce);
      if (cj) atomicAdd(&r->n_junction, cj);
      if (co) atomicAdd(&r->n_orth, co);
      if (cd) atomicAdd(&r->n_diag, cd);
      if (cf) atomicAdd(&r->n_far, cf);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_y), (unsigned long long)((long long)y * cn));
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_x), (unsigned long long)(long long)sx);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_yy), (unsigned long long)((long long)y * y * cn));
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_xx), (unsigned long long)sxx);
      atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_xy), (unsigned long long)((long long)y * sx));
      if (sd) atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_d2), (unsigned long long)sd);
      if (md) atomicMax(&r->max_d2, md);
    }
  }
  // header: the largest label and the overflow flag by atomics, iterations and converged from the flags by the first wave
  const int m = (int)wave_max((unsigned long long)lmax);
  if (lane == 0 && m > 0) {
    atomicMax(&table[0].n_junction, m);
    if (m > max_regions) atomicOr(&table[0].n_orth, 1);
  }
  if (wave == 0) {
    int cnt = 0;
    for (int i = lane; i < max_iter; i += INSAR_WAVE) cnt += iterflag[i] != 0;
#pragma unroll
    for (int o = INSAR_WAVE / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, INSAR_WAVE);
    if (lane == 0) {
      table[0].n = cnt;
      table[0].n_end = cnt < max_iter;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct SkLayout {
  int Ww, tiles_x, tiles_y, steps;
  int64_t nw, ntiles, off_alive, off_changed, off_iter, bytes;
};

static int sk_layout(const char* who, int32_t H, int32_t W, int32_t max_iter, SkLayout* l) {
  if (H < 1 || W < 1 || H > SK_MAX_DIM || W > SK_MAX_DIM)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: map %d x %d: H and W in 1..%d", who, H, W, SK_MAX_DIM);
  if (max_iter < 1 || max_iter > SK_MAX_ITER) INSAR_FAIL(INSAR_E_ARG, "%s: max_iterations %d outside 1..%d", who, max_iter, SK_MAX_ITER);
  l->Ww = (W + 63) / 64;
  l->nw = (int64_t)H * l->Ww;
  l->tiles_x = (l->Ww + SK_TW - 1) / SK_TW;
  l->tiles_y = (H + SK_TH - 1) / SK_TH;
  l->ntiles = (int64_t)l->tiles_x * l->tiles_y;
  l->steps = (max_iter + SK_T - 1) / SK_T;
  l->off_alive = 8 * l->nw * 8;
  l->off_changed = l->off_alive + 2 * l->nw * 8;
  l->off_iter = l->off_changed + ((2 * l->ntiles * 4 + 15) & ~(int64_t)15);
  l->bytes = l->off_iter + (((int64_t)max_iter * 4 + 15) & ~(int64_t)15);
  return INSAR_OK;
}

static int sk_check_table(const char* who, const void* table, int32_t max_regions) {
  if (max_regions < 1 || max_regions > (1 << 30)) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d outside 1..2^30", who, max_regions);
  if (!table) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (table)", who);
  if (!insar_aligned16(table)) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 16-byte aligned", who);
  return INSAR_OK;
}

extern "C" int insar_skeleton_scratch_bytes(int32_t H, int32_t W, int32_t max_iterations, int32_t max_regions, int64_t* scratch_bytes,
                                            int64_t* table_bytes) {
  const char* who = "insar_skeleton_scratch_bytes";
  if (!scratch_bytes || !table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  SkLayout l;
  if (int rc = sk_layout(who, H, W, max_iterations, &l)) return rc;
  if (max_regions < 1 || max_regions > (1 << 30)) INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d outside 1..2^30", who, max_regions);
  *scratch_bytes = l.bytes;
  *table_bytes = (int64_t)sizeof(InsarSkeletonStat) * ((int64_t)max_regions + 1);
  return INSAR_OK;
}

extern "C" int insar_skeleton_launches(int32_t H, int32_t W, int32_t max_iterations, int32_t widths) {
  SkLayout l;
  if (int rc = sk_layout("insar_skeleton_launches", H, W, max_iterations, &l)) return rc;
  return 2 + l.steps + (widths ? 2 : 0);
}

extern "C" int insar_skeleton_planes(const int32_t* labels, int32_t H, int32_t W, int32_t max_iterations, int32_t max_regions,
                                     void* scratch, void* table, void* stream) {
  const char* who = "insar_skeleton_planes";
  if (!labels || !scratch) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !labels ? "labels" : "scratch");
  SkLayout l;
  if (int rc = sk_layout(who, H, W, max_iterations, &l)) return rc;
  if (int rc = sk_check_table(who, table, max_regions)) return rc;
  if (((uintptr_t)labels) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: labels not 4-byte aligned", who);
  if (!insar_aligned16(scratch)) INSAR_FAIL(INSAR_E_ALIGN, "%s: scratch not 16-byte aligned", who);
  char* s = (char*)scratch;
  const int64_t n16 = ((int64_t)max_regions + 1) * (int64_t)(sizeof(InsarSkeletonStat) / 16);
  hipLaunchKernelGGL(sk_planes_kernel, dim3(insar_grid_cap((l.nw + 3) / 4)), dim3(SK_ST_THREADS), 0, (hipStream_t)stream, labels, H, W,
                     l.Ww, l.nw, (uint64_t*)s, (uint64_t*)(s + l.off_alive), (int4*)table, n16, (int*)(s + l.off_iter),
                     (int)max_iterations);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_skeleton_step(int32_t H, int32_t W, int32_t max_iterations, int32_t step, void* scratch, void* stream) {
  const char* who = "insar_skeleton_step";
  if (!scratch) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (scratch)", who);
  SkLayout l;
  if (int rc = sk_layout(who, H, W, max_iterations, &l)) return rc;
  if (step < 0 || step >= l.steps) INSAR_FAIL(INSAR_E_ARG, "%s: step %d outside 0..%d", who, step, l.steps - 1);
  if (!insar_aligned16(scratch)) INSAR_FAIL(INSAR_E_ALIGN, "%s: scratch not 16-byte aligned", who);
  char* s = (char*)scratch;
  uint64_t* alive = (uint64_t*)(s + l.off_alive);
  int* changed = (int*)(s + l.off_changed);
  const int cur = step & 1, niter = max_iterations - step * SK_T < SK_T ? max_iterations - step * SK_T : SK_T;
  hipLaunchKernelGGL(sk_step_kernel, dim3((unsigned)l.ntiles), dim3(SK_THREADS), 0, (hipStream_t)stream, (const uint64_t*)s,
                     (const uint64_t*)(alive + cur * l.nw), alive + (cur ^ 1) * l.nw, H, l.Ww, l.nw, l.tiles_x, l.tiles_y,
                     step == 0 ? (const int*)nullptr : (const int*)(changed + (cur ^ 1) * l.ntiles), changed + cur * l.ntiles,
                     (int*)(s + l.off_iter) + step * SK_T, niter);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_skeleton_stats(const int32_t* labels, const int32_t* d2, int32_t H, int32_t W, int32_t max_iterations,
                                    int32_t max_regions, void* scratch, void* table, uint8_t* skeleton, void* stream) {
  const char* who = "insar_skeleton_stats";
  if (!labels || !scratch || !skeleton)
    INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !labels ? "labels" : !scratch ? "scratch" : "skeleton");
  SkLayout l;
  if (int rc = sk_layout(who, H, W, max_iterations, &l)) return rc;
  if (int rc = sk_check_table(who, table, max_regions)) return rc;
  if ((((uintptr_t)labels) | ((uintptr_t)d2)) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: labels / d2 not 4-byte aligned", who);
  if (!insar_aligned16(scratch)) INSAR_FAIL(INSAR_E_ALIGN, "%s: scratch not 16-byte aligned", who);
  char* s = (char*)scratch;
  const uint64_t* alive = (const uint64_t*)(s + l.off_alive) + (l.steps & 1) * l.nw;
  hipLaunchKernelGGL(sk_stats_kernel, dim3(insar_grid_cap((l.nw + 3) / 4)), dim3(SK_ST_THREADS), 0, (hipStream_t)stream, labels, d2,
                     (const uint64_t*)s, alive, H, W, l.Ww, l.nw, (const int*)(s + l.off_iter), (int)max_iterations, (int)max_regions,
                     (InsarSkeletonStat*)table, skeleton);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
