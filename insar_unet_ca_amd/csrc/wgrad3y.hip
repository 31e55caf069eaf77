// Weight gradient of a 3x3 / stride-1 convolution (Unet-ChannalAttention.py:81,84 inside loss.backward(), :345): wgrad3x.hip's
// row-of-taps decomposition
//
//   part[split][3*ty + tx][co][ci] = sum_p dY[p, co] * X[p + (ty-1)*(W+2) + (tx-1), ci],   tx = 0, 1, 2
//
// built for TWO CO-RESIDENT WORK-GROUPS PER CU, as conv3x3_flat2.hip is for the forward / input-gradient convolutions:
//   * a work-group is 4 waves (one per SIMD) on a 128 (ci) x 128 (co) tile, each wave the same 64 x 64 x three-tap tile as in
//     wgrad3x.hip (192 accumulator registers, same plane-layout LDS image: every fragment address a lane register plus an
//     immediate, same ds_read_b64_tr_b16 reads);
//   * LDS: a TWO-slot ring of 34 KB stages (X 72 pixel rows x 128 ci + dY 64 x 128 co) = 68 KB — two work-groups per CU, each
//     wave with the 256-register budget of two waves per SIMD;
//   * a K step (64 pixels) = [LDS-DMA of step k + 1 (9 one-KB pieces per wave, spread over the step's first phases) | six
//     phases of 8 (+ 8) fragment reads and 16 MFMAs, NO barrier between them] -> s_waitcnt vmcnt(0) (the pieces are a whole
//     step old) -> ONE s_barrier. The two work-groups of a CU are not coupled at all: the MFMA pipe alternates between the two
//     waves of a SIMD by itself, and one group's slab stores / first-step wait run under the other's K loop.
// wgrad3x.hip couples its eight waves through twelve barriers per K step (two wave groups in opposite roles) and reaches
// 59 - 63 % MFMA-busy; the decoupled form is what took the flat kernel's K loop from ~57 % to ~70 %. It stages 89 bytes per MFMA
// through the L2 -> LDS path (wgrad3x: 68), still under the ~88 B/MFMA that path sustains at the MFMA peak.
// Same products in the same order per accumulator as wgrad3.hip / wgrad3x.hip: the slabs are bit for bit theirs at the same
// split.
#include "wgrad3_common.h"

#define WY_BKP 64       // pixels per K step
#define WY_XR 72        // X rows staged per step: padded pixel p0 - 1 + r
#define WY_RB 256       // bytes per LDS row (128 channels)

WGRAD3_STAMPS(wgrad3y)

// LDS image: the plane layout of wgrad3_common.h, NB = WM / WN blocks per plane row
template <int TM, int TN>
struct Wgrad3yCfg {
  static constexpr int THREADS = 256, NW = 4;
  static constexpr int WM = TM / 64, WN = TN / 64;                    // waves along ci / co = blocks per plane row
  static constexpr int RBX = 32 * WM, RBY = 32 * WN;                  // bytes per plane row
  static constexpr int XPL = WY_XR * RBX, YPL = WY_BKP * RBY;         // bytes per plane
  static constexpr int X_STAGE = 4 * XPL, Y_STAGE = 4 * YPL;
  static constexpr int STAGE = X_STAGE + Y_STAGE;                     // 34 KB
  static constexpr int NSLOT = 2;
  static constexpr int LDS_BYTES = NSLOT * STAGE;
  static constexpr int XP = X_STAGE / 1024, YP = Y_STAGE / 1024;      // 1-KB pieces per step: 18 + 16
  static constexpr int NXI = (XP + NW - 1) / NW, NYI = YP / NW;       // DMA instructions per wave per step (the last X one: waves < XP % 4 only)
  static constexpr int XTAIL = XP % NW;                               // waves that issue the last X instruction (0: all)
  static_assert(WM * WN == NW, "four 64 x 64 wave tiles");
  static_assert(YP % NW == 0, "dY stage: whole block-wide DMA instructions");
  static_assert(2 * LDS_BYTES <= 160 * 1024, "two work-groups per CU");
};

// SINV: W >= 64 — a K step lies inside one image row, + 32 pixels is + 32 staged rows for X too (an immediate).
template <int TM, int TN, bool SINV>
__global__ __launch_bounds__(256, 2) void wgrad3y_kernel(Wgrad3Args a) {
  using Cfg = Wgrad3yCfg<TM, TN>;
  constexpr int NW = Cfg::NW;
  constexpr int NXI = Cfg::NXI, NYI = Cfg::NYI, NPW = NXI + NYI;      // pieces per wave per step (waves beyond XTAIL: one less)
  constexpr int WM = Cfg::WM, WN = Cfg::WN, RBX = Cfg::RBX, RBY = Cfg::RBY;
  constexpr int NSX = SINV ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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

  // per-lane byte offsets of its DMA chunks relative to the step's scalar base. Piece q = i*4 + wave holds the 16-byte
  // chunks q*64 + lane of the stage: plane, row, slot in the row -> the block stored there (slot ^ f(row)) and its half.
  // X rows the step does not need (beyond 64 + 2*rpk) are fetched from the last needed row instead: every piece is issued
  // whole, with the same count on every step (counted vmcnt), nothing outside the buffer is touched; those LDS rows are
  // never read.
  const long long xpitch = (long long)a.Cx * 2, ypitch = (long long)a.Cdy * 2;
  const int xneed = WY_BKP + 2 * a.rpk;
  uint32_t xoff_i[NXI], yoff_i[NYI];
#pragma unroll
  for (int i = 0; i < NXI; ++i) {
    constexpr int CPR = RBX / 16;
    const int c = (i * NW + wave) * 64 + lane;
    const int plane = c / (WY_XR * CPR), row = (c / CPR) % WY_XR, cc = c % CPR;
    const int blk = plane * WM + ((cc >> 1) ^ wgrad3_slot<WM>(row));
    const int srow = row < xneed ? row : xneed - 1;
    xoff_i[i] = (uint32_t)(srow * xpitch) + blk * 32 + (cc & 1) * 16;
  }
#pragma unroll
  for (int i = 0; i < NYI; ++i) {
    constexpr int CPR = RBY / 16;
    const int c = (i * NW + wave) * 64 + lane;
    const int plane = c / (WY_BKP * CPR), row = (c / CPR) % WY_BKP, cc = c % CPR;
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
    const long long p = ((long long)img * (a.H + 2) + hrow + 1) * a.Wp + seg * WY_BKP + 1;
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
      if (j < NXI - 1 || xtail) wgrad3_dma(sx, xoff_i[j], l + j * (NW * 1024));
    } else {
      wgrad3_dma(sy, yoff_i[j - NXI], l + Cfg::X_STAGE + (j - NXI) * (NW * 1024));
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
    wgrad3_wait_vm_lgkm<0>();
    __builtin_amdgcn_s_barrier();
    WGRAD3_STAMP(1);        // first step landed

    // lane bases of the fragment reads (slot 0): see wgrad3x.hip
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
      // the other slot was last read in step k - 1, whose reads every wave finished before the barrier that ended it
      const bool more = k + 1 < nsteps;
      const char* nsx = xbase; const char* nsy = ybase;
      if (more) {
        const long long p1 = next_pixel();
        nsx = xbase + p1 * xpitch; nsy = ybase + p1 * ypitch;
      }
      bf16x8_t yf[4], xf[4];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int t3 = 0; t3 < 3; ++t3) {
          const int ph = s * 3 + t3;
          if (t3 == 0) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
              for (int nt = 0; nt < 4; ++nt) {
                s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(uintptr_t)(by[h] + (s * 32 * RBY + nt * Cfg::YPL)));
                yf[nt][4 * h + 0] = v[0]; yf[nt][4 * h + 1] = v[1]; yf[nt][4 * h + 2] = v[2]; yf[nt][4 * h + 3] = v[3];
              }
          }
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
              s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                  (lds_s16x4_p)(uintptr_t)(bx[SINV ? 0 : s][h][t3] + ((SINV ? s * 32 * RBX : 0) + mt * Cfg::XPL)));
              xf[mt][4 * h + 0] = v[0]; xf[mt][4 * h + 1] = v[1]; xf[mt][4 * h + 2] = v[2]; xf[mt][4 * h + 3] = v[3];
            }
          // the pieces of step k + 1, two per phase behind the phase's reads (the last phase issues none)
          if (more) {
#pragma unroll
            for (int j = 2 * ph; j < 2 * ph + 2; ++j)
              if (j < NPW && ph < 5) piece(slot ^ 1, nsx, nsy, j);
          }
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
              acc[t3][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[mt], yf[nt], acc[t3][mt][nt], 0, 0, 0);
          __builtin_amdgcn_s_setprio(0);
        }
      }
      // the pieces of step k + 1 were issued at least a phase ago, most of them a whole step: wait them out, then meet
      wgrad3_wait_vm_lgkm<0>();
      __builtin_amdgcn_s_barrier();
      const int delta = slot ? -Cfg::STAGE : Cfg::STAGE;
      slot ^= 1;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        by[h] += delta;
#pragma unroll
        for (int sx = 0; sx < NSX; ++sx)
#pragma unroll
          for (int t3 = 0; t3 < 3; ++t3) bx[sx][h][t3] += delta;
      }
    }
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
    for (int k = 0; k < 8; ++k) atomicAdd(&g_wgrad3y_stamps[(blockIdx.x & 1023) * 8 + k], stamp_acc[k]);
  }
#endif
}

template <int TM, int TN, bool SINV>
static int launch_wgrad3y_s(Wgrad3Args& a, hipStream_t s) {
  using Cfg = Wgrad3yCfg<TM, TN>;
  return wgrad3_launch<wgrad3y_kernel<TM, TN, SINV>>(a, TM, TN, Cfg::LDS_BYTES, Cfg::THREADS, "insar_wgrad_conv3y", s);
}

// (128 << 16) | 128 where this kernel applies (bf16, image rows that are whole K steps or K steps that are whole image rows,
// both channel counts multiples of 128), else 0
extern "C" int insar_wgrad_conv3y_tile(const InsarAct* x, int32_t Cout) {
  if (!x || x->dtype != INSAR_BF16) return 0;
  const bool rows_ok = (x->W % WY_BKP) == 0 || ((x->W == 16 || x->W == 32) && (x->H % (WY_BKP / x->W)) == 0);
  if (!rows_ok) return 0;
  return (x->c_len % 128 == 0 && Cout % 128 == 0) ? ((128 << 16) | 128) : 0;
}

// part[split][tap][co][ci] as insar_wgrad_conv3 / insar_wgrad_conv3x write it (same fold: insar_wgrad_reduce)
extern "C" int insar_wgrad_conv3y(const InsarAct* x, const InsarAct* dy, float* part, int32_t nsplit, void* stream) {
  int rc;
  if ((rc = wgrad3_check_operands("insar_wgrad_conv3y", x, dy, part))) return rc;
  if (!insar_wgrad_conv3y_tile(x, dy->c_len))
    INSAR_FAIL(INSAR_E_SHAPE, "insar_wgrad_conv3y: unsupported layer (bf16; W %% 64 == 0, or W = 16 / 32 with whole K steps per image; channels in 128s); use insar_wgrad_conv3");
  Wgrad3Args a;
  if ((rc = wgrad3_fill_args(a, "insar_wgrad_conv3y", x, dy, part, nsplit, WY_BKP, WY_XR, WY_XR))) return rc;
  hipStream_t s = (hipStream_t)stream;
  return a.lw == 6 ? launch_wgrad3y_s<128, 128, true>(a, s) : launch_wgrad3y_s<128, 128, false>(a, s);
}
