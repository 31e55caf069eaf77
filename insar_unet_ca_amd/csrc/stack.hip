// Detections through a stack of dates. The state is two bit-plane tensors, hit and valid, int64 [words][H][W]: date t is
// bit t & 63 of plane t >> 6. Five launches, one per entry point:
//
//   push     n dates of class maps into n bits (read-modify-write of the words touched, the inputs read once)
//   shift    the k oldest dates dropped, in place
//   summary  per pixel over a window: counts, first / last hit, the longest run of hits among the valid dates, the rule
//   clear    the series table zeroed
//   series   per label of a map and per date of the window: how many of its pixels are hits, how many are valid
//
// The scan of the summary skips dates whose valid bit is 0. Its kernel does not walk dates: inside the window the maximal
// runs of ones of x = hit | ~valid are exactly the runs of the scan, widened by unobserved dates at either end and between
// the hits; the length of a run is the number of hit bits under it, its start the lowest of them. A pixel therefore costs
// one step per run and gap, at most 64 per word, and a pixel whose window is all hits or all valid costs one per word.
//
// The series kernel folds before the table's atomics, three levels:
//   wave        a wave takes 4 x 64 consecutive pixels, slot j of lane i holds pixel 64 j + i: the ballot of one date's bit
//               over a slot is a 64-bit word of pixels, and popcount(ballot & the lanes of a run) is the run's count. The
//               head lane of a run adds it to the table if it is not 0.
//   hot label   ONE label per work-group (the vote of zonal.hip: the longest run of the pass) is counted with no atomic at
//               all: popcount(ballot & lanes of the hot label) is uniform over the wave, and lane b of the wave keeps the sum
//               for date b of each plane in a register.
//   work-group  when the vote changes, and at the end, the waves add those registers into one LDS record, which goes to the
//               table with one add per date that is not 0. A map that is one region sends 1 + 2 nt adds per work-group.
// Agent-scope relaxed integer adds only (the rule of overlap.hip and zonal.hip), no work-group waits on another, nothing is
// read back. hit / valid under background pixels are not read.
#include "scene_common.h"

#define SK_THREADS 256
#define SK_MAX_WORDS 4
#define SK_MAX_DATES (64 * SK_MAX_WORDS)
#define SK_MAX_REGIONS (1 << 24)
#define SK_HEADER 4                                              // int32 words before the first row of the series table

typedef unsigned long long sk_u64;

struct SkClasses { sk_u64 w[4]; };
struct SkPlanes { int16_t *n_valid, *n_hit, *longest_run, *run_start, *first_hit, *last_hit; uint8_t *known, *persistent; };

#define SK_ADD(p, v, scope) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, scope)

// ---- four consecutive pixels of one plane ------------------------------------------------------------------------------------
__device__ __forceinline__ void quad_load_u64(const int64_t* p, int64_t i, int64_t n, bool vec, sk_u64* v) {
  if (vec) {
    const insar_i64x2* q = reinterpret_cast<const insar_i64x2*>(p + i);
    const insar_i64x2 a = q[0], b = q[1];
    v[0] = (sk_u64)a.a; v[1] = (sk_u64)a.b; v[2] = (sk_u64)b.a; v[3] = (sk_u64)b.b;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (i + j < n) ? (sk_u64)p[i + j] : 0ull;
  }
}
__device__ __forceinline__ void quad_store_u64(int64_t* p, int64_t i, int64_t n, bool vec, const sk_u64* v) {
  if (vec) {
    const int64_t s[4] = {(int64_t)v[0], (int64_t)v[1], (int64_t)v[2], (int64_t)v[3]};
    quad_store_i64(p + i, s);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = (int64_t)v[j];
  }
}
__device__ __forceinline__ void quad_store_i16(int16_t* p, int64_t i, int64_t n, bool vec, const int* v) {
  if (vec) {
    const uint32_t lo = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
    const uint32_t hi = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
    *reinterpret_cast<uint2*>(p + i) = make_uint2(lo, hi);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = (int16_t)v[j];
  }
}
// bits lo .. hi - 1 of a word, 0 <= lo < hi <= 64
__host__ __device__ __forceinline__ sk_u64 sk_bits(int lo, int hi) {
  const sk_u64 m = (hi - lo) >= 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull);
  return m << lo;
}

// ---- push ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SK_THREADS)
stack_push_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ valid_in, const float* __restrict__ conf, float min_conf,
                  SkClasses cs, int ignore, int n, int t, int64_t npix, int vec_u8, int vec_f32, int vec_w, int64_t* hit, int64_t* valid) {
  const int64_t nquads = (npix + 3) >> 2;
  const int w_first = t >> 6, w_last = (t + n - 1) >> 6;
  for (int64_t qd = blockIdx.x * (int64_t)SK_THREADS + threadIdx.x; qd < nquads; qd += (int64_t)gridDim.x * SK_THREADS) {
    const int64_t i0 = qd << 2;
    for (int w = w_first; w <= w_last; ++w) {                    // at most SK_MAX_WORDS
      const int lo = t > 64 * w ? t : 64 * w;
      const int hi = t + n < 64 * w + 64 ? t + n : 64 * w + 64;
      sk_u64 hb[4] = {0ull, 0ull, 0ull, 0ull}, vb[4] = {0ull, 0ull, 0ull, 0ull};
      for (int d = lo; d < hi; ++d) {                            // at most 64
        const int64_t off = (int64_t)(d - t) * npix;
        int m[4], vi[4] = {1, 1, 1, 1};
        float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        quad_load_u8(mask + off, i0, npix, vec_u8 != 0, 0, m);
        if (valid_in) quad_load_u8(valid_in + off, i0, npix, vec_u8 != 0, 0, vi);
        if (conf) quad_load(conf + off, i0, npix, vec_f32 != 0, 0.0f, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int cw = m[j] >> 6;
          const sk_u64 set = cw == 0 ? cs.w[0] : cw == 1 ? cs.w[1] : cw == 2 ? cs.w[2] : cs.w[3];
          const bool v = m[j] != ignore && vi[j] != 0;
          const bool h = v && ((set >> (m[j] & 63)) & 1ull) && (!conf || c[j] >= min_conf);       // a NaN compares false
          vb[j] |= (sk_u64)v << (d & 63);
          hb[j] |= (sk_u64)h << (d & 63);
        }
      }
      const sk_u64 wm = sk_bits(lo & 63, (lo & 63) + (hi - lo));
      int64_t* hp = hit + (int64_t)w * npix;
      int64_t* vp = valid + (int64_t)w * npix;
      if (wm != ~0ull) {
        sk_u64 oh[4], ov[4];
        quad_load_u64(hp, i0, npix, vec_w != 0, oh);
        quad_load_u64(vp, i0, npix, vec_w != 0, ov);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          hb[j] |= oh[j] & ~wm;
          vb[j] |= ov[j] & ~wm;
        }
      }
      quad_store_u64(hp, i0, npix, vec_w != 0, hb);
      quad_store_u64(vp, i0, npix, vec_w != 0, vb);
    }
  }
}

// ---- shift -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SK_THREADS)
stack_shift_kernel(int64_t* hit, int64_t* valid, int words, int64_t npix, int vec_w, int k) {
  if (k == 0) return;
  const int64_t nquads = (npix + 3) >> 2;
  const bool clear = k >= 64 * words;
  const int q = k >> 6, r = k & 63;
  for (int64_t qd = blockIdx.x * (int64_t)SK_THREADS + threadIdx.x; qd < nquads; qd += (int64_t)gridDim.x * SK_THREADS) {
    const int64_t i0 = qd << 2;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      int64_t* p = which ? valid : hit;
      sk_u64 o[SK_MAX_WORDS + 1][4];
#pragma unroll
      for (int w = 0; w <= SK_MAX_WORDS; ++w) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[w][j] = 0ull;
        if (w < words && !clear) quad_load_u64(p + (int64_t)w * npix, i0, npix, vec_w != 0, o[w]);
      }
#pragma unroll
      for (int s = 0; s < SK_MAX_WORDS - 1; ++s)                 // whole planes, with constant indices
        if (s < q) {
#pragma unroll
          for (int w = 0; w < SK_MAX_WORDS; ++w)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[w][j] = o[w + 1][j];
        }
#pragma unroll
      for (int w = 0; w < SK_MAX_WORDS; ++w) {
        if (w >= words) break;
        sk_u64 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = r ? (o[w][j] >> r) | (o[w + 1][j] << (64 - r)) : o[w][j];
        quad_store_u64(p + (int64_t)w * npix, i0, npix, vec_w != 0, v);
      }
    }
  }
}

// ---- summary ---------------------------------------------------------------------------------------------------------------------
struct SkScan { int n_valid, n_hit, best, best_start, first, last, cur, cur_start; };

// one word of the window: h = hits (already & valid & window), x = (hit | ~valid) & window, base = 64 * plane
__device__ __forceinline__ void sk_scan_word(SkScan& s, sk_u64 h, sk_u64 v, sk_u64 x, int base, bool want_run) {
  s.n_valid += __popcll(v);
  s.n_hit += __popcll(h);
  if (h) {
    if (s.first < 0) s.first = base + (int)__builtin_ctzll(h);
    s.last = base + 63 - (int)__builtin_clzll(h);
  }
  if (!want_run) return;
  sk_u64 rem = x;
  int b = 0;
  while (b < 64) {                                               // one step per gap and run: at most 64 per word
    if (!(rem & 1ull)) {                                         // a valid miss (or the window's edge) ends the open run
      if (s.cur > s.best) { s.best = s.cur; s.best_start = s.cur_start; }
      s.cur = 0;
      s.cur_start = -1;
      if (!rem) break;
      const int z = (int)__builtin_ctzll(rem);
      rem >>= z;
      b += z;
    }
    const sk_u64 inv = ~rem;
    const int o = inv ? (int)__builtin_ctzll(inv) : 64;          // b + o <= 64: the shifts brought zeros in from the top
    const sk_u64 under = h & sk_bits(b, b + o);
    if (under) {
      if (s.cur_start < 0) s.cur_start = base + (int)__builtin_ctzll(under);
      s.cur += __popcll(under);
    }
    b += o;
    if (b >= 64) break;                                          // the run reaches bit 63 and stays open into the next plane
    rem >>= o;
  }
}

__global__ void __launch_bounds__(SK_THREADS)
stack_summary_kernel(const int64_t* __restrict__ hit, const int64_t* __restrict__ valid, int64_t npix, int vec_w, int vec_16, int vec_8,
                     int t0, int t1, int min_hits, int min_run, int min_valid, long long num, long long den, int want_run, SkPlanes out) {
  const int64_t nquads = (npix + 3) >> 2;
  const int w_first = t0 >> 6, w_last = (t1 - 1) >> 6;           // an empty window never enters the loop (t1 = t0 is checked)
  for (int64_t qd = blockIdx.x * (int64_t)SK_THREADS + threadIdx.x; qd < nquads; qd += (int64_t)gridDim.x * SK_THREADS) {
    const int64_t i0 = qd << 2;
    SkScan s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = SkScan{0, 0, 0, -1, -1, -1, 0, -1};
    if (t1 > t0)
      for (int w = w_first; w <= w_last; ++w) {
        const int lo = t0 > 64 * w ? t0 : 64 * w;
        const int hi = t1 < 64 * w + 64 ? t1 : 64 * w + 64;
        const sk_u64 wm = sk_bits(lo & 63, (lo & 63) + (hi - lo));
        sk_u64 hw[4], vw[4];
        quad_load_u64(hit + (int64_t)w * npix, i0, npix, vec_w != 0, hw);
        quad_load_u64(valid + (int64_t)w * npix, i0, npix, vec_w != 0, vw);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const sk_u64 v = vw[j] & wm, h = hw[j] & v;
          sk_scan_word(s[j], h, v, (h | ~v) & wm, 64 * w, want_run != 0);
        }
      }
    int nv[4], nh[4], lr[4], rs[4], fh[4], lh[4], kn[4], ps[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (s[j].cur > s[j].best) { s[j].best = s[j].cur; s[j].best_start = s[j].cur_start; }
      nv[j] = s[j].n_valid; nh[j] = s[j].n_hit; lr[j] = s[j].best; rs[j] = s[j].best_start; fh[j] = s[j].first; lh[j] = s[j].last;
      // without the runs (min_run <= 1 and no run plane asked for) the longest run is >= 1 exactly where there is a hit
      const bool run_ok = want_run ? lr[j] >= min_run : (min_run <= 0 || nh[j] >= 1);
      kn[j] = nv[j] >= min_valid;
      ps[j] = kn[j] && nh[j] >= min_hits && run_ok && (long long)nh[j] * den >= num * (long long)nv[j];
    }
    if (out.n_valid) quad_store_i16(out.n_valid, i0, npix, vec_16 != 0, nv);
    if (out.n_hit) quad_store_i16(out.n_hit, i0, npix, vec_16 != 0, nh);
    if (out.longest_run) quad_store_i16(out.longest_run, i0, npix, vec_16 != 0, lr);
    if (out.run_start) quad_store_i16(out.run_start, i0, npix, vec_16 != 0, rs);
    if (out.first_hit) quad_store_i16(out.first_hit, i0, npix, vec_16 != 0, fh);
    if (out.last_hit) quad_store_i16(out.last_hit, i0, npix, vec_16 != 0, lh);
    if (out.known) quad_store_u8(out.known, i0, npix, vec_8 != 0, kn);
    if (out.persistent) quad_store_u8(out.persistent, i0, npix, vec_8 != 0, ps);
  }
}

// ---- series ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SK_THREADS)
stack_clear_kernel(int4* __restrict__ table, int64_t chunks) {
  for (int64_t i = blockIdx.x * (int64_t)SK_THREADS + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * SK_THREADS)
    table[i] = make_int4(0, 0, 0, 0);
}

// the lanes lane .. (next head above lane) - 1
__device__ __forceinline__ sk_u64 sk_run_lanes(sk_u64 heads, int lane) {
  const sk_u64 above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
  const int end = above ? (int)__builtin_ctzll(above) : 64;
  return sk_bits(lane, end);
}

__global__ void __launch_bounds__(SK_THREADS)
stack_series_kernel(const int64_t* __restrict__ hit, const int64_t* __restrict__ valid, const int* __restrict__ labels, int64_t npix,
                    int t0, int t1, int max_regions, int* table) {
  __shared__ int rec[1 + 2 * SK_MAX_DATES];                      // the hot label: area, hits by date of the stack, valids
  __shared__ unsigned long long vote[2];
  const int tid = threadIdx.x, lane = tid & (INSAR_WAVE - 1), wave = tid / INSAR_WAVE;
  for (int i = tid; i < 1 + 2 * SK_MAX_DATES; i += SK_THREADS) rec[i] = 0;
  if (tid < 2) vote[tid] = 0ull;
  __syncthreads();

  const int nt = t1 - t0, row = 1 + 2 * nt;
  const int w_first = t0 >> 6, w_last = nt ? (t1 - 1) >> 6 : w_first - 1;
  int* rows = table + SK_HEADER;
  int acc_h[SK_MAX_WORDS] = {0, 0, 0, 0}, acc_v[SK_MAX_WORDS] = {0, 0, 0, 0};   // lane b: date 64 (w_first + wi) + b of the hot label
  int acc_area = 0;                                              // uniform over the wave
  int hot = 0, par = 0, oor = 0;
  const int64_t pass = 4 * (int64_t)SK_THREADS;

  // what the registers hold goes to the LDS record; uniform over the work-group, with its own barrier
  auto spill = [&]() {
#pragma unroll
    for (int wi = 0; wi < SK_MAX_WORDS; ++wi) {                  // a plane past the window holds zeros and is never an index
      if (acc_h[wi]) SK_ADD(&rec[1 + 64 * (w_first + wi) + lane], acc_h[wi], __HIP_MEMORY_SCOPE_WORKGROUP);
      if (acc_v[wi]) SK_ADD(&rec[1 + SK_MAX_DATES + 64 * (w_first + wi) + lane], acc_v[wi], __HIP_MEMORY_SCOPE_WORKGROUP);
      acc_h[wi] = acc_v[wi] = 0;
    }
    if (lane == 0 && acc_area) SK_ADD(&rec[0], acc_area, __HIP_MEMORY_SCOPE_WORKGROUP);
    acc_area = 0;
    __syncthreads();
    int* r = rows + (int64_t)(hot - 1) * row;
    for (int i = tid; i < 1 + 2 * SK_MAX_DATES; i += SK_THREADS) {
      const int v = rec[i];
      if (!v) continue;
      rec[i] = 0;
      if (i == 0) { SK_ADD(r, v, __HIP_MEMORY_SCOPE_AGENT); continue; }
      const int kind = (i - 1) / SK_MAX_DATES, d = (i - 1) % SK_MAX_DATES - t0;       // only window dates were ever added
      if (d >= 0 && d < nt) SK_ADD(r + 1 + kind * nt + d, v, __HIP_MEMORY_SCOPE_AGENT);
    }
  };

  for (int64_t p0 = blockIdx.x * pass; p0 < npix; p0 += (int64_t)gridDim.x * pass, par ^= 1) {   // uniform over the work-group
    const int64_t base = p0 + (int64_t)wave * (4 * INSAR_WAVE) + lane;
    int key[4];
    sk_u64 heads[4], mine[4];
    unsigned long long best = 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + j * INSAR_WAVE;
      const int l = i < npix ? labels[i] : 0;
      oor += l > max_regions;
      key[j] = (l > 0 && l <= max_regions) ? l : 0;
      const WaveRuns r = wave_runs(key[j]);
      heads[j] = __ballot(r.head);
      mine[j] = sk_run_lanes(heads[j], lane);
      const unsigned long long cand = r.head && key[j] ? ((unsigned long long)(unsigned int)__popcll(mine[j]) << 32) | (unsigned int)key[j] : 0ull;
      best = cand > best ? cand : best;
      if (!r.head) mine[j] = 0ull;                               // only the head of a run reports it
    }
    best = wave_max(best);
    if (lane == 0 && best) __hip_atomic_fetch_max(&vote[par], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();                                             // A: the votes are in
    const unsigned long long won = vote[par];
    const int next_hot = won ? (int)(unsigned int)won : hot;     // a pass without a candidate keeps the label
    if (next_hot != hot && hot != 0) spill();
    if (tid == 0) vote[par ^ 1] = 0ull;                          // read last before barrier B of the pass before
    __syncthreads();                                             // B
    hot = next_hot;

#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const sk_u64 labelled = __ballot(key[j] != 0);
      if (!labelled) continue;                                   // uniform over the wave
      const sk_u64 hotl = __ballot(key[j] == hot);               // hot != 0 here: some key is not 0, so a vote was cast
      const bool cold = key[j] != 0 && key[j] != hot && mine[j] != 0ull;
      const bool any_cold = __ballot(cold) != 0ull;
      const int64_t i = base + j * INSAR_WAVE;
      int* r = rows + (int64_t)(key[j] > 0 ? key[j] - 1 : 0) * row;
      acc_area += __popcll(hotl);
      if (cold) SK_ADD(r, __popcll(mine[j]), __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int wi = 0; wi < SK_MAX_WORDS; ++wi) {
        const int w = w_first + wi;
        if (w > w_last) break;                                   // uniform
        const int lo = t0 > 64 * w ? t0 : 64 * w;
        const int hi = t1 < 64 * w + 64 ? t1 : 64 * w + 64;
        const sk_u64 wm = sk_bits(lo & 63, (lo & 63) + (hi - lo));
        sk_u64 vw = 0ull, hw = 0ull;
        if (key[j] != 0) {
          vw = (sk_u64)valid[(int64_t)w * npix + i] & wm;
          hw = (sk_u64)hit[(int64_t)w * npix + i] & vw;
        }
        int ah = 0, av = 0;
        for (int d = lo; d < hi; ++d) {                          // at most 64
          const int b = d & 63;
          const sk_u64 vb = __ballot((vw >> b) & 1ull);
          if (!vb) continue;                                     // uniform: nobody saw this date
          const sk_u64 hb = __ballot((hw >> b) & 1ull);
          const int cv = __popcll(vb & hotl), ch = __popcll(hb & hotl);
          if (lane == b) { av += cv; ah += ch; }
          if (any_cold && cold) {
            const int rv = __popcll(vb & mine[j]), rh = __popcll(hb & mine[j]);
            if (rv) SK_ADD(r + 1 + nt + (d - t0), rv, __HIP_MEMORY_SCOPE_AGENT);
            if (rh) SK_ADD(r + 1 + (d - t0), rh, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        acc_h[wi] += ah;                                         // constant indices once unrolled: registers
        acc_v[wi] += av;
      }
    }
  }
  if (hot != 0) spill();                                         // uniform: hot comes from the shared vote
#pragma unroll
  for (int o = INSAR_WAVE / 2; o > 0; o >>= 1) oor += __shfl_xor(oor, o, INSAR_WAVE);
  if (lane == 0 && oor) SK_ADD(table, oor, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int stack_check_state(const char* who, const void* hit, const void* valid, int32_t words, int32_t H, int32_t W, int64_t* npix) {
  if (!hit || !valid) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (%s)", who, !hit ? "hit" : "valid");
  if (words < 1 || words > SK_MAX_WORDS) INSAR_FAIL(INSAR_E_SHAPE, "%s: words %d outside 1..%d", who, words, SK_MAX_WORDS);
  if (H < 1 || W < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: empty map %d x %d", who, H, W);
  *npix = (int64_t)H * W;
  if (*npix >= ((int64_t)1 << 31)) INSAR_FAIL(INSAR_E_SHAPE, "%s: map %d x %d has 2^31 pixels or more", who, H, W);
  if ((((uintptr_t)hit) & 7u) || (((uintptr_t)valid) & 7u)) INSAR_FAIL(INSAR_E_ALIGN, "%s: hit / valid not 8-byte aligned", who);
  return INSAR_OK;
}
static int stack_check_window(const char* who, int32_t words, int32_t t0, int32_t t1) {
  if (t0 < 0 || t1 < t0 || t1 > 64 * words)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: window %d..%d: 0 <= t0 <= t1 <= %d dates", who, t0, t1, 64 * words);
  return INSAR_OK;
}
static inline dim3 stack_quad_grid(int64_t npix) { return dim3(insar_grid_cap(((npix + 3) / 4 + SK_THREADS - 1) / SK_THREADS)); }
static inline int stack_vec_words(int64_t npix, const void* hit, const void* valid) {
  return npix % 4 == 0 && insar_aligned16(hit) && insar_aligned16(valid);
}

extern "C" int insar_stack_push(const uint8_t* mask, const uint8_t* valid_in, const float* conf, float min_conf, uint64_t classes_w0,
                                uint64_t classes_w1, uint64_t classes_w2, uint64_t classes_w3, int32_t ignore, int32_t n, int32_t t,
                                int32_t words, int32_t H, int32_t W, int64_t* hit, int64_t* valid, void* stream) {
  const char* who = "insar_stack_push";
  if (!mask) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (mask)", who);
  int64_t npix = 0;
  if (int rc = stack_check_state(who, hit, valid, words, H, W, &npix)) return rc;
  if (n < 1 || t < 0 || (int64_t)t + n > 64 * words)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: dates %d..%d: n >= 1 and 0 <= t, t + n <= %d", who, t, t + n - 1, 64 * words);
  if (ignore < -1 || ignore > 255) INSAR_FAIL(INSAR_E_ARG, "%s: ignore %d outside -1..255", who, ignore);
  if (!(fabsf(min_conf) <= 3.402823466e38f)) INSAR_FAIL(INSAR_E_ARG, "%s: min_conf is not finite", who);
  if (conf && (((uintptr_t)conf) & 3u)) INSAR_FAIL(INSAR_E_ALIGN, "%s: conf not 4-byte aligned", who);
  const bool quads = npix % 4 == 0;
  const int vec_u8 = quads && (((uintptr_t)mask) & 3u) == 0 && (((uintptr_t)valid_in) & 3u) == 0;
  const int vec_f32 = quads && insar_aligned16(conf);
  SkClasses cs;
  cs.w[0] = classes_w0; cs.w[1] = classes_w1; cs.w[2] = classes_w2; cs.w[3] = classes_w3;
  hipLaunchKernelGGL(stack_push_kernel, stack_quad_grid(npix), dim3(SK_THREADS), 0, (hipStream_t)stream, mask, valid_in, conf, min_conf, cs,
                     (int)ignore, (int)n, (int)t, npix, vec_u8, vec_f32, stack_vec_words(npix, hit, valid), hit, valid);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_stack_shift(int64_t* hit, int64_t* valid, int32_t words, int32_t H, int32_t W, int32_t k, void* stream) {
  const char* who = "insar_stack_shift";
  int64_t npix = 0;
  if (int rc = stack_check_state(who, hit, valid, words, H, W, &npix)) return rc;
  if (k < 0) INSAR_FAIL(INSAR_E_ARG, "%s: k %d is negative", who, k);
  hipLaunchKernelGGL(stack_shift_kernel, k == 0 ? dim3(1) : stack_quad_grid(npix), dim3(SK_THREADS), 0, (hipStream_t)stream, hit, valid,
                     (int)words, npix, stack_vec_words(npix, hit, valid), (int)k);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_stack_summary(const int64_t* hit, const int64_t* valid, int32_t words, int32_t H, int32_t W, int32_t t0, int32_t t1,
                                   int32_t min_hits, int32_t min_run, int32_t min_valid, int32_t num, int32_t den, int16_t* n_valid,
                                   int16_t* n_hit, int16_t* longest_run, int16_t* run_start, int16_t* first_hit, int16_t* last_hit,
                                   uint8_t* known, uint8_t* persistent, void* stream) {
  const char* who = "insar_stack_summary";
  int64_t npix = 0;
  if (int rc = stack_check_state(who, hit, valid, words, H, W, &npix)) return rc;
  if (int rc = stack_check_window(who, words, t0, t1)) return rc;
  if (min_hits < 0 || min_hits > 32767 || min_run < 0 || min_run > 32767 || min_valid < 0 || min_valid > 32767)
    INSAR_FAIL(INSAR_E_ARG, "%s: min_hits %d, min_run %d, min_valid %d: each in 0..32767", who, min_hits, min_run, min_valid);
  if (den < 1 || num < 0 || num > den) INSAR_FAIL(INSAR_E_ARG, "%s: fraction %d / %d: 0 <= num <= den, den >= 1", who, num, den);
  int16_t* const p16[6] = {n_valid, n_hit, longest_run, run_start, first_hit, last_hit};
  bool any = known || persistent, al16 = true;
  for (int i = 0; i < 6; ++i) {
    any = any || p16[i];
    if (((uintptr_t)p16[i]) & 1u) INSAR_FAIL(INSAR_E_ALIGN, "%s: an int16 plane is not 2-byte aligned", who);
    al16 = al16 && (((uintptr_t)p16[i]) & 7u) == 0;
  }
  if (!any) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (every output plane)", who);
  const bool quads = npix % 4 == 0;
  const int vec_8 = quads && (((uintptr_t)known) & 3u) == 0 && (((uintptr_t)persistent) & 3u) == 0;
  const int want_run = longest_run || run_start || (persistent && min_run > 1);
  SkPlanes out = {n_valid, n_hit, longest_run, run_start, first_hit, last_hit, known, persistent};
  hipLaunchKernelGGL(stack_summary_kernel, stack_quad_grid(npix), dim3(SK_THREADS), 0, (hipStream_t)stream, hit, valid, npix,
                     stack_vec_words(npix, hit, valid), (int)(quads && al16), vec_8, (int)t0, (int)t1, (int)min_hits, (int)min_run,
                     (int)min_valid, (long long)num, (long long)den, want_run, out);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

static int stack_series_layout(const char* who, int32_t max_regions, int32_t n_dates, int64_t* bytes) {
  if (max_regions < 1 || max_regions > SK_MAX_REGIONS)
    INSAR_FAIL(INSAR_E_SHAPE, "%s: max_regions %d outside 1..%d", who, max_regions, SK_MAX_REGIONS);
  if (n_dates < 0 || n_dates > SK_MAX_DATES) INSAR_FAIL(INSAR_E_SHAPE, "%s: %d dates outside 0..%d", who, n_dates, SK_MAX_DATES);
  *bytes = (4 * (SK_HEADER + (int64_t)max_regions * (1 + 2 * (int64_t)n_dates)) + 15) & ~(int64_t)15;
  return INSAR_OK;
}
static int stack_check_table(const char* who, const void* table) {
  if (!table) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (table)", who);
  if (!insar_aligned16(table)) INSAR_FAIL(INSAR_E_ALIGN, "%s: table not 16-byte aligned", who);
  return INSAR_OK;
}

extern "C" int insar_stack_series_bytes(int32_t max_regions, int32_t n_dates, int64_t* table_bytes) {
  const char* who = "insar_stack_series_bytes";
  if (!table_bytes) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", who);
  return stack_series_layout(who, max_regions, n_dates, table_bytes);
}

extern "C" int insar_stack_series_clear(void* table, int32_t max_regions, int32_t n_dates, void* stream) {
  const char* who = "insar_stack_series_clear";
  int64_t bytes = 0;
  if (int rc = stack_series_layout(who, max_regions, n_dates, &bytes)) return rc;
  if (int rc = stack_check_table(who, table)) return rc;
  const int64_t chunks = bytes / 16;
  hipLaunchKernelGGL(stack_clear_kernel, dim3(insar_grid_cap((chunks + SK_THREADS - 1) / SK_THREADS)), dim3(SK_THREADS), 0,
                     (hipStream_t)stream, (int4*)table, chunks);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}

extern "C" int insar_stack_series(const int64_t* hit, const int64_t* valid, int32_t words, const int32_t* labels, int32_t H, int32_t W,
                                  int32_t t0, int32_t t1, int32_t max_regions, void* table, void* stream) {
  const char* who = "insar_stack_series";
  int64_t npix = 0, bytes = 0;
  if (int rc = stack_check_state(who, hit, valid, words, H, W, &npix)) return rc;
  if (!labels) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer (labels)", who);
  if (((uintptr_t)labels) & 3u) INSAR_FAIL(INSAR_E_ALIGN, "%s: labels not 4-byte aligned", who);
  if (int rc = stack_check_window(who, words, t0, t1)) return rc;
  if (int rc = stack_series_layout(who, max_regions, t1 - t0, &bytes)) return rc;
  if (int rc = stack_check_table(who, table)) return rc;
  const int64_t passes = (npix + 4 * SK_THREADS - 1) / (4 * SK_THREADS);
  hipLaunchKernelGGL(stack_series_kernel, dim3(insar_grid_cap(passes, 4 * insar_num_cus())), dim3(SK_THREADS), 0, (hipStream_t)stream, hit,
                     valid, (const int*)labels, npix, (int)t0, (int)t1, (int)max_regions, (int*)table);
  INSAR_CHECK_LAUNCH(who);
  return INSAR_OK;
}
