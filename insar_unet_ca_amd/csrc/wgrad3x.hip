// Weight gradient of a 3x3 / stride-1 convolution (Unet-ChannalAttention.py:81,84 inside loss.backward(), :345) for the
// layers with >= 128 channels on one side and >= 256 on the other: the row-of-taps decomposition of wgrad3.hip
//
//   part[split][3*ty + tx][co][ci] = sum_p dY[p, co] * X[p + (ty-1)*(W+2) + (tx-1), ci],   tx = 0, 1, 2
//
// on a 256 x 128 (or 128 x 256) tile of (ci, co) with a K loop that never drains the LDS-DMA queue:
//
//   * 8 waves, each a 64 (ci) x 64 (co) tile of all three taps: 192 accumulator registers a lane, 16 MFMAs per
//     8 + 8 transposing fragment reads (wgrad3's 128 x 128 tile: 8 MFMAs per 8 + 4), 6.5 one-KB DMA pieces per wave
//     per 96 MFMAs (there: 4.25 per 48);
//   * a K step (64 pixels) is SIX phases (pixel half s = 0, 1 x tap tx = 0, 1, 2) of
//         [load part: the phase's fragment reads + some DMA pieces of the step after next] -> s_barrier ->
//         [compute part: 16 MFMAs under s_setprio 1] -> s_barrier,
//     and waves 4-7 run one barrier behind waves 0-3 (the two waves of every SIMD alternate roles: one's MFMA cluster
//     runs beside its partner's LDS reads and DMA issue);
//   * a THREE-slot LDS ring (3 x 52 KB): the pieces of step k + 2 are issued during step k, and the only vector-memory
//     wait of the loop is a COUNTED one at the end of a step — s_waitcnt vmcnt(pieces issued during this step) — which
//     retires the pieces of step k + 1, a whole step old by then. Nothing in the loop waits for vmcnt(0).
//
// Ordering argument (P = 6k + p counts phases, g(n) the work-group's n-th barrier; group 0's load part of phase P lies
// between g(2P) and g(2P+1), its compute part between g(2P+1) and g(2P+2); group 1 is one barrier later in both):
//   RAW  every wave waits for its own pieces of step k+1 before the barrier that ends its load part of phase 6k+5
//        (group 0: g(12k+11), group 1: g(12k+12)); the first read of step k+1 is group 0's, after g(12k+12).
//   WAR  slot (k+2) % 3 was last read in step k-1, whose last reads (group 1, load part of phase 6k-1) were waited for
//        (lgkmcnt(0)) before group 1 arrived at g(12k); the first DMA into it is issued by group 0 after g(12k+2).
// Same LDS image (pixel rows of 256 bytes, XOR-swizzled on the DMA source side, ds_read_b64_tr_b16), same products in the
// same order per accumulator as wgrad3.hip's: the slabs are bit for bit that kernel's at the same split.
#include "wgrad3_common.h"

#define WX_BKP 64       // pixels per K step
#define WX_XR 72        // X rows staged per step: padded pixel p0 - 1 + r
#define WX_RB 256       // bytes per LDS row (128 channels)

WGRAD3_STAMPS(wgrad3x)

// LDS image: the plane layout of wgrad3_common.h, NB = WM / WN blocks per plane row
template <int TM, int TN>
struct Wgrad3xCfg {
  static constexpr int THREADS = 512, NW = 8;
  static constexpr int WM = TM / 64, WN = TN / 64;                    // waves along ci / co = blocks per plane row
  static constexpr int RBX = 32 * WM, RBY = 32 * WN;                  // bytes per plane row
  static constexpr int XPL = WX_XR * RBX, YPL = WX_BKP * RBY;         // bytes per plane
  static constexpr int X_STAGE = 4 * XPL, Y_STAGE = 4 * YPL;
  static constexpr int STAGE = X_STAGE + Y_STAGE;
  static constexpr int NSLOT = 3;
  static constexpr int LDS_BYTES = NSLOT * STAGE;
  static constexpr int XP = X_STAGE / 1024, YP = Y_STAGE / 1024;      // 1-KB pieces per step
  static constexpr int NXI = (XP + NW - 1) / NW, NYI = YP / NW;       // DMA instructions per wave per step (the last X one: waves < XP % 8 only)
  static constexpr int XTAIL = XP % NW;                               // waves that issue the last X instruction (0: all)
  static_assert(WM * WN == NW, "eight 64 x 64 wave tiles");
  static_assert(YP % NW == 0, "dY stage: whole block-wide DMA instructions");
  static_assert(LDS_BYTES <= 160 * 1024, "three slots must fit the CU's LDS");
};

// SINV: W >= 64 — a K step lies inside one image row, + 32 pixels is + 32 staged rows for X too (an immediate).
// VAR: 0 = the kernel. Experiment builds (-DINSAR_EXP_WX, tools/gemm_bench.py --what x3var) instantiate timing ablations of the
// K loop, whose RESULTS ARE WRONG by construction: bit 0 = no LDS-DMA inside the loop, bit 2 = the two wave groups in
// lockstep, bit 3 = no MFMAs, bit 4 = no fragment reads.
template <int TM, int TN, bool SINV, int VAR = 0>
__global__ __launch_bounds__(512) void wgrad3x_kernel(Wgrad3Args a) {
  using Cfg = Wgrad3xCfg<TM, TN>;
  constexpr int NXI = Cfg::NXI, NYI = Cfg::NYI, NPW = NXI + NYI;      // pieces per wave per step (waves beyond XTAIL: one less)
  constexpr int WM = Cfg::WM, WN = Cfg::WN, RBX = Cfg::RBX, RBY = Cfg::RBY;
  constexpr int NSX = SINV ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;                                          // 0: waves 0-3, 1: waves 4-7 (SIMD partners)
#ifdef INSAR_STAMPS
  unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long stamp_prev = __builtin_amdgcn_s_memtime();
  const unsigned long long stamp_t0 = stamp_prev, stamp_r0 = __builtin_amdgcn_s_memrealtime();   // [6] / [7]: shader clock vs 100 MHz
#endif
  int t = xcd_tile(blockIdx.x, gridDim.x);
  const int ty = t % 3; t /= 3;
  const int ni = t % a.ntc; t /= a.ntc;
  const int mi = t % a.mtc; t /= a.mtc;
  const int split = t;

  const int ks0 = split * a.steps_per_split;
  int ks1 = ks0 + a.steps_per_split;
  if (ks1 > (int)a.ksteps) ks1 = (int)a.ksteps;
  const int nsteps = ks1 > ks0 ? ks1 - ks0 : 0;

  // per-lane byte offsets of its DMA chunks relative to the step's scalar base. Piece q = i*8 + wave holds the 16-byte
  // chunks q*64 + lane of the stage: plane, row, slot in the row -> the block stored there (slot ^ f(row)) and its half.
  // X rows the step does not need (beyond 64 + 2*rpk) are fetched from the last needed row instead: every piece is issued
  // whole, with the same count on every step (counted vmcnt), nothing outside the buffer is touched; those LDS rows are
  // never read.
  const long long xpitch = (long long)a.Cx * 2, ypitch = (long long)a.Cdy * 2;
  const int xneed = WX_BKP + 2 * a.rpk;
  uint32_t xoff_i[NXI], yoff_i[NYI];
#pragma unroll
  for (int i = 0; i < NXI; ++i) {
    constexpr int CPR = RBX / 16;
    const int c = (i * 8 + wave) * 64 + lane;
    const int plane = c / (WX_XR * CPR), row = (c / CPR) % WX_XR, cc = c % CPR;
    const int blk = plane * WM + ((cc >> 1) ^ wgrad3_slot<WM>(row));
    const int srow = row < xneed ? row : xneed - 1;
    xoff_i[i] = (uint32_t)(srow * xpitch) + blk * 32 + (cc & 1) * 16;
  }
#pragma unroll
  for (int i = 0; i < NYI; ++i) {
    constexpr int CPR = RBY / 16;
    const int c = (i * 8 + wave) * 64 + lane;
    const int plane = c / (WX_BKP * CPR), row = (c / CPR) % WX_BKP, cc = c % CPR;
    const int blk = plane * WN + ((cc >> 1) ^ wgrad3_slot<WN>(row));
    yoff_i[i] = (uint32_t)((row + 2 * (row >> a.lw)) * ypitch) + blk * 32 + (cc & 1) * 16;
  }
  // X row r of a step <-> padded pixel p0 + (ty-1)*Wp - 1 + r; dY row k <-> padded pixel p0 + k + 2*(k / W)
  const char* xbase = a.x + ((long long)(ty - 1) * a.Wp - 1) * xpitch + ((long long)a.cx_off + mi * TM) * 2;
  const char* ybase = a.dy + ((long long)a.cdy_off + ni * TN) * 2;

  // padded index of the first pixel of a K step, advanced step by step (wave-uniform)
  int seg, hrow, img;
  {
    const int g = ks0 / a.spr, gpi = a.H / a.rpk;
    seg = ks0 - g * a.spr;
    img = g / gpi;
    hrow = (g - img * gpi) * a.rpk;
  }
  auto next_pixel = [&]() -> long long {
    const long long p = ((long long)img * (a.H + 2) + hrow + 1) * a.Wp + seg * WX_BKP + 1;
    if (++seg == a.spr) {
      seg = 0; hrow += a.rpk;
      if (hrow >= a.H) { hrow = 0; ++img; }
    }
    return p;
  };
  const uint32_t ldsb = lds_offset_of(smem);
  const uint32_t lds0 = ldsb + wave * 1024;
  const bool xtail = Cfg::XTAIL == 0 || wave < Cfg::XTAIL;            // this wave issues the last X instruction
  // DMA instruction j of a step (j < NXI: X piece j*8 + wave, else dY piece (j - NXI)*8 + wave) into ring slot `slot`
  auto piece = [&](int slot, const char* sx, const char* sy, int j) {
    const uint32_t l = lds0 + slot * Cfg::STAGE;
    if (j < NXI) {
      if (j < NXI - 1 || xtail) wgrad3_dma(sx, xoff_i[j], l + j * 8192);
    } else {
      wgrad3_dma(sy, yoff_i[j - NXI], l + Cfg::X_STAGE + (j - NXI) * 8192);
    }
  };

  f32x4_t acc[3][4][4];
#pragma unroll
  for (int t3 = 0; t3 < 3; ++t3)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t3][i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int wm = wave % WM, wn = wave / WM;
  const int r16 = lane & 15, kq = lane >> 4;

  if (nsteps > 0) {
    WGRAD3_STAMP(0);        // set-up
    {
      const long long p0 = next_pixel();
      const char* sx = xbase + p0 * xpitch; const char* sy = ybase + p0 * ypitch;
#pragma unroll
      for (int j = 0; j < NPW; ++j) piece(0, sx, sy, j);
    }
    if (nsteps > 1) {
      const long long p1 = next_pixel();
      const char* sx = xbase + p1 * xpitch; const char* sy = ybase + p1 * ypitch;
#pragma unroll
      for (int j = 0; j < NPW; ++j) piece(1, sx, sy, j);
      if (xtail) wgrad3_wait_vm_lgkm<NPW>(); else wgrad3_wait_vm_lgkm<NPW - 1>();      // step 0 landed, step 1 in flight
    } else {
      wgrad3_wait_vm_lgkm<0>();
    }
    __builtin_amdgcn_s_barrier();
    WGRAD3_STAMP(1);        // first step landed
    if (grp == 1 && !(VAR & 4)) __builtin_amdgcn_s_barrier();          // group 1 runs one barrier behind

    // lane bases of the fragment reads (slot 0). A transposing read hands lane r16 of a 16-lane group channel r16 of the
    // four pixel rows the group addresses (lane 4q + p: row q, 8-byte column p): two reads (h) fill a lane's 8 pixels of
    // a 32-pixel MFMA step; for odd kq the two halves are swapped on both operands alike, so that the partner group of a
    // 32-lane half always holds the other four row residues mod 8.
    //   dY row of (s, h)      = lrow[h] + 32*s                    lrow[h] = kq*8 + ((h ^ (kq & 1)) << 2) + (r16 >> 2)
    //   X  row of (s, h, tx)  = xrow[h] + s*SS + tx               xrow[h] = lrow[h] + 2*(lrow[h] >> lw), SS = 32 + 2*(32 >> lw)
    uint32_t by[2], bx[NSX][2][3];
    {
      const int SS = 32 + 2 * (32 >> a.lw);
      const int p8 = (r16 & 3) * 8;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int lr = kq * 8 + ((h ^ (kq & 1)) << 2) + (r16 >> 2);
        by[h] = ldsb + Cfg::X_STAGE + lr * RBY + ((wn ^ wgrad3_slot<WN>(lr)) << 5) + p8;
        const int xr = lr + 2 * (lr >> a.lw);
#pragma unroll
        for (int sx = 0; sx < NSX; ++sx)
#pragma unroll
          for (int t3 = 0; t3 < 3; ++t3) {
            const int r = xr + sx * SS + t3;
            bx[sx][h][t3] = ldsb + r * RBX + ((wm ^ wgrad3_slot<WM>(r)) << 5) + p8;
          }
      }
    }
    typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_p;
    int slot = 0;
    for (int k = 0; k < nsteps; ++k) {
      const bool more2 = k + 2 < nsteps;
      int slot2 = slot + 2; if (slot2 >= 3) slot2 -= 3;
      const char* nsx = xbase; const char* nsy = ybase;
      if (more2) {
        const long long p2 = next_pixel();
        nsx = xbase + p2 * xpitch; nsy = ybase + p2 * ypitch;
      }
      bf16x8_t yf[4], xf[4];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int t3 = 0; t3 < 3; ++t3) {
          const int ph = s * 3 + t3;
          // ---- load part ----
          if (t3 == 0 && !(VAR & 16)) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
              for (int nt = 0; nt < 4; ++nt) {
                s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(uintptr_t)(by[h] + (s * 32 * RBY + nt * Cfg::YPL)));
                yf[nt][4 * h + 0] = v[0]; yf[nt][4 * h + 1] = v[1]; yf[nt][4 * h + 2] = v[2]; yf[nt][4 * h + 3] = v[3];
              }
          }
          if (!(VAR & 16)) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
              for (int mt = 0; mt < 4; ++mt) {
                s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (lds_s16x4_p)(uintptr_t)(bx[SINV ? 0 : s][h][t3] + ((SINV ? s * 32 * RBX : 0) + mt * Cfg::XPL)));
                xf[mt][4 * h + 0] = v[0]; xf[mt][4 * h + 1] = v[1]; xf[mt][4 * h + 2] = v[2]; xf[mt][4 * h + 3] = v[3];
              }
          }
          // DMA pieces of step k + 2: none beside the 16-read phases (tx = 0), the rest spread over the other four
          if (more2 && !(VAR & 1)) {
            if (ph == 1) { piece(slot2, nsx, nsy, 0); piece(slot2, nsx, nsy, 1); }
            if (ph == 2) { piece(slot2, nsx, nsy, 2); piece(slot2, nsx, nsy, 3); }
            if (ph == 4) {
#pragma unroll
              for (int j = 4; j < NPW - 1; ++j) piece(slot2, nsx, nsy, j);
            }
            if (ph == 5) piece(slot2, nsx, nsy, NPW - 1);
          }
          if (ph == 5) {
            // the one vector-memory wait of the step: everything but the pieces issued during this step has landed
            if (!more2 || (VAR & 1)) wgrad3_wait_vm_lgkm<0>();
            else if (xtail) wgrad3_wait_vm_lgkm<NPW>();
            else wgrad3_wait_vm_lgkm<NPW - 1>();
          } else {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          }
          __builtin_amdgcn_s_barrier();
          // ---- compute part ----
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(1);
          if (VAR & 16) {                                              // keep the stale fragments "live"
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(xf[i]), "+v"(yf[i]));
          }
          if (!(VAR & 8)) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
              for (int nt = 0; nt < 4; ++nt)
                acc[t3][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[mt], yf[nt], acc[t3][mt][nt], 0, 0, 0);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" :: "v"(xf[i]), "v"(yf[i]));
          }
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_barrier();
        }
      }
      // next ring slot: the lane bases move with it, in place
      const int delta = slot == 2 ? -2 * Cfg::STAGE : Cfg::STAGE;
      if (++slot == 3) slot = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        by[h] += delta;
#pragma unroll
        for (int sx = 0; sx < NSX; ++sx)
#pragma unroll
          for (int t3 = 0; t3 < 3; ++t3) bx[sx][h][t3] += delta;
      }
    }
    if (grp == 0 && !(VAR & 4)) __builtin_amdgcn_s_barrier();          // group 0 meets group 1's last barrier
  }

  WGRAD3_STAMP(2);          // K loop
  // C layout of a 16x16 accumulator: row (ci) = kq*4 + reg, col (co) = r16  ->  16-byte stores into [co][ci];
  // tile mt of wave wm is channel block mt*WM + wm (see the LDS image above)
#pragma unroll
  for (int t3 = 0; t3 < 3; ++t3) {
    float* out = a.part + ((long long)split * 9 + ty * 3 + t3) * a.Cout * a.Cin;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int ci = mi * TM + (mt * WM + wm) * 16 + kq * 4;
        const int co = ni * TN + (nt * WN + wn) * 16 + r16;
        *(f32x4_t*)(out + (long long)co * a.Cin + ci) = acc[t3][mt][nt];
      }
  }
#ifdef INSAR_STAMPS
  WGRAD3_STAMP(3);          // slab stores
  stamp_acc[6] = __builtin_amdgcn_s_memtime() - stamp_t0;
  stamp_acc[7] = __builtin_amdgcn_s_memrealtime() - stamp_r0;
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) atomicAdd(&g_wgrad3x_stamps[(blockIdx.x & 1023) * 8 + k], stamp_acc[k]);
  }
#endif
}

template <int TM, int TN, bool SINV, int VAR = 0>
static int launch_wgrad3x_s(Wgrad3Args& a, hipStream_t s) {
  using Cfg = Wgrad3xCfg<TM, TN>;
  return wgrad3_launch<wgrad3x_kernel<TM, TN, SINV, VAR>>(a, TM, TN, Cfg::LDS_BYTES, Cfg::THREADS, "insar_wgrad_conv3x", s);
}
template <int TM, int TN, int VAR = 0>
static int launch_wgrad3x(Wgrad3Args& a, hipStream_t s) {
  return a.lw == 6 ? launch_wgrad3x_s<TM, TN, true, VAR>(a, s) : launch_wgrad3x_s<TM, TN, false, VAR>(a, s);
}

// (tile(Cin) << 16) | tile(Cout) of this kernel for the layer, or 0 where it does not apply (insar_wgrad_conv3 then):
// bf16, image rows that are whole K steps (or K steps that are whole image rows), 256 channels on one side and 128 on
// the other. The wider side goes to x when both fit (its fragments are re-read per tap, dY's are not).
extern "C" int insar_wgrad_conv3x_tile(const InsarAct* x, int32_t Cout) {
  if (!x || x->dtype != INSAR_BF16) return 0;
  const bool rows_ok = (x->W % WX_BKP) == 0 || ((x->W == 16 || x->W == 32) && (x->H % (WX_BKP / x->W)) == 0);
  if (!rows_ok) return 0;
  if (x->c_len % 256 == 0 && Cout % 128 == 0) return (256 << 16) | 128;
  if (x->c_len % 128 == 0 && Cout % 256 == 0) return (128 << 16) | 256;
  return 0;
}

// part[split][tap][co][ci] as insar_wgrad_conv3 writes it (same fold: insar_wgrad_reduce)
extern "C" int insar_wgrad_conv3x(const InsarAct* x, const InsarAct* dy, float* part, int32_t nsplit, void* stream) {
  int rc;
  if ((rc = wgrad3_check_operands("insar_wgrad_conv3x", x, dy, part))) return rc;
  const int pair = insar_wgrad_conv3x_tile(x, dy->c_len);
  if (!pair) INSAR_FAIL(INSAR_E_SHAPE, "insar_wgrad_conv3x: unsupported layer (bf16; W %% 64 == 0, or W = 16 / 32 with whole K steps per image; 256 x 128 or 128 x 256 channel tiles); use insar_wgrad_conv3");
  Wgrad3Args a;
  // 32-bit lane offsets of the DMA source: 72 pixel rows of the wider buffer
  if ((rc = wgrad3_fill_args(a, "insar_wgrad_conv3x", x, dy, part, nsplit, WX_BKP, WX_XR, WX_XR))) return rc;
  hipStream_t s = (hipStream_t)stream;
#ifdef INSAR_EXP_WX
  if ((pair >> 16) == 256) {
    switch (insar_knob(KNOB_WGRAD3X_VAR)) {
      case 1: return launch_wgrad3x<256, 128, 1>(a, s);
      case 4: return launch_wgrad3x<256, 128, 4>(a, s);
      case 8: return launch_wgrad3x<256, 128, 8>(a, s);
      case 9: return launch_wgrad3x<256, 128, 9>(a, s);
      case 17: return launch_wgrad3x<256, 128, 17>(a, s);
      case 25: return launch_wgrad3x<256, 128, 25>(a, s);
      default: break;
    }
  }
#endif
  if ((pair >> 16) == 256) return launch_wgrad3x<256, 128>(a, s);
  return launch_wgrad3x<128, 256>(a, s);
}
