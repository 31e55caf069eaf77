// What the four row-of-taps weight-gradient kernels (wgrad3.hip, wgrad3x.hip, wgrad3y.hip, wgrad3k.hip) share: the kernel
// argument block, the LDS-DMA / counted-wait / plane-slot helpers of the plane-layout kernels (3x, 3y, 3k), the -DINSAR_STAMPS
// scaffold, and the host side of an entry point (operand checks, argument fill, launch). The K loops, the *Cfg structs and
// the _tile / _slices predicates are the kernels' own.
#pragma once
#include <type_traits>
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// Kernel arguments of wgrad3, wgrad3x and wgrad3y.
struct Wgrad3Args {
  const char* x; const char* dy; float* part;
  long long ksteps;             // B*H*W / pixels per K step
  int nsplit, steps_per_split;
  int H, W, Wp;
  int spr, rpk, lw;             // K steps per image row (W >= step) / image rows per K step (W < step) / log2(W) (6 if W >= step)
  int Cx, cx_off, Cin; int Cdy, cdy_off, Cout;
  int mtc, ntc;
};
// wgrad3k's: the same without rpk and lw (its K steps lie inside one image row). It keeps a struct of its own because with
// Wgrad3Args the compiler groups the kernel-argument loads differently and allocates other registers throughout (compared on
// the gfx950 assembly): not the same device code.
struct Wgrad3kArgs {
  const char* x; const char* dy; float* part;
  long long ksteps;
  int nsplit, steps_per_split;
  int H, W, Wp, spr;
  int Cx, cx_off, Cin; int Cdy, cdy_off, Cout;
  int mtc, ntc;
};

// LDS-DMA of one 1-KB piece: per-lane source = scalar base + 32-bit lane offset, wave-uniform LDS destination in M0
__device__ __forceinline__ void wgrad3_dma(const char* sbase, uint32_t voff, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

template <int N> __device__ __forceinline__ void wgrad3_wait_vm_lgkm() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory"); }

// LDS image of an operand tile (X: 72 pixel rows x TM channels, dY: 64 x TN), cut for ADDRESSES THAT NEED NO ARITHMETIC:
// the wave at position w of NB (= 4 or 2) along the operand's channel dimension owns the 16-channel blocks t*NB + w,
// t = 0..3 (its four MFMA tiles), and block t*NB + w lives in PLANE t: plane t = [rows][NB blocks x 32 bytes], the NB
// adjacent blocks t*NB .. t*NB + NB - 1 of a pixel (one 128- or 64-byte run of the NHWC row: whole-line gathers). A tile
// index is then a compile-time plane offset, and inside a plane row the 32-byte slot of block w is w ^ f(row) with
// f(row) = (row / RPL) % NB, RPL = 8 / NB rows per 256-byte bank line: the eight pixel rows a 32-lane half of a
// ds_read_b64_tr_b16 touches (r0 .. r0+3 from one 16-lane group, the other four residues mod 8 from its partner) land in
// eight different 32-byte bank segments whatever r0 is — so the tap shift (row + tx) and the pixel half (row + 32) only
// move r0. What depends on the lane — row base, f(row), the 8-byte column inside the block — is folded into ONE base
// register per (k half h, tap tx) (and per pixel half where the halo rows make + 32 pixels a shift that is not a multiple
// of 8 rows: W < 64), kept across the loop and advanced in place by one ring slot per step; every fragment read is that
// register + an immediate. (The first build of wgrad3x recomputed XOR-swizzled addresses per phase, ~1.5 VALU
// operations per MFMA in the load part: 41 % of its run time, profiles/r04_wgrad3x_ablation.txt.)
template <int NB> __device__ __forceinline__ int wgrad3_slot(int row) { return NB == 4 ? (row >> 1) & 3 : (row >> 2) & 1; }

// Diagnostic build only (-DINSAR_STAMPS, tools/stamp_gemm.py). WGRAD3_STAMPS(wgrad3x) at file scope: the device array
// g_wgrad3x_stamps (8 counters for each of 1024 work-group slots) and its getter insar_debug_wgrad3x_stamps. WGRAD3_STAMP(k)
// inside a kernel that declares stamp_acc[8] and stamp_prev: the s_memtime ticks since the previous stamp go to counter k.
#ifdef INSAR_STAMPS
#define WGRAD3_STAMPS(name)                                                                                                      \
  __device__ unsigned long long g_##name##_stamps[1024 * 8];                                                                     \
  extern "C" int insar_debug_##name##_stamps(unsigned long long* out, int reset) {                                               \
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_##name##_stamps), sizeof(g_##name##_stamps)) != hipSuccess) return -1;      \
    if (reset) { static unsigned long long z[1024 * 8]; if (hipMemcpyToSymbol(HIP_SYMBOL(g_##name##_stamps), z, sizeof(z)) != hipSuccess) return -2; } \
    return 0;                                                                                                                    \
  }
#define WGRAD3_STAMP(k) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); stamp_acc[k] += now_ - stamp_prev; stamp_prev = now_; } while (0)
#else
#define WGRAD3_STAMPS(name)
#define WGRAD3_STAMP(k)
#endif

// Host side of an entry point `name`, in the order every entry keeps: wgrad3_check_operands, then the entry's own _tile
// predicate (its message names the kernel's conditions), then wgrad3_fill_args, then wgrad3_launch.
static int wgrad3_check_operands(const char* name, const InsarAct* x, const InsarAct* dy, const float* part) {
  if (!x || !dy || !part) INSAR_FAIL(INSAR_E_ARG, "%s: null pointer", name);
  int rc;
  if ((rc = insar_check_act(x, name, "x"))) return rc;
  if ((rc = insar_check_act(dy, name, "dy"))) return rc;
  if (x->B != dy->B || x->H != dy->H || x->W != dy->W) INSAR_FAIL(INSAR_E_SHAPE, "%s: x/dy grids differ", name);
  if (x->dtype != dy->dtype) INSAR_FAIL(INSAR_E_DTYPE, "%s: x/dy dtype differ", name);
  return INSAR_OK;
}

// bkp: pixels per K step. xrows / yrows: the X / dY pixel rows a K step's 32-bit DMA lane offsets span (bf16 kernels), whose
// byte extent must fit 31 bits; xrows = 0: the kernel addresses with 64-bit pointers (wgrad3.hip), no bound.
template <typename Args>
static int wgrad3_fill_args(Args& a, const char* name, const InsarAct* x, const InsarAct* dy, float* part, int32_t nsplit,
                            int bkp, int xrows, int yrows) {
  if (nsplit < 1) INSAR_FAIL(INSAR_E_SHAPE, "%s: nsplit", name);
  if (xrows && ((long long)xrows * x->C * 2 >= 0x7fffffffLL || (long long)yrows * dy->C * 2 >= 0x7fffffffLL))
    INSAR_FAIL(INSAR_E_SHAPE, "%s: channel pitch too large", name);
  a.x = (const char*)x->ptr; a.dy = (const char*)dy->ptr; a.part = part;
  a.ksteps = (long long)x->B * x->H * x->W / bkp;
  a.nsplit = nsplit;
  a.steps_per_split = (int)((a.ksteps + nsplit - 1) / nsplit);
  a.H = x->H; a.W = x->W; a.Wp = x->W + 2;
  a.spr = x->W >= bkp ? x->W / bkp : 1;
  if constexpr (std::is_same_v<Args, Wgrad3Args>) {
    a.rpk = x->W >= bkp ? 1 : bkp / x->W;
    a.lw = x->W >= bkp ? 6 : (x->W == 32 ? 5 : 4);
  }
  a.Cx = x->C; a.cx_off = x->c_off; a.Cin = x->c_len;
  a.Cdy = dy->C; a.cdy_off = dy->c_off; a.Cout = dy->c_len;
  return INSAR_OK;
}

// One work-group per (split, kernel row, Cin tile, Cout tile). Kernel is a template parameter so that the per-device
// "attribute set" mask (see insar_set_lds_once in common.h) is one per kernel instantiation.
template <auto Kernel, typename Args>
static int wgrad3_launch(Args& a, int tm, int tn, int lds_bytes, int threads, const char* name, hipStream_t s) {
  static std::atomic<uint64_t> attr_mask{0};
  {
    hipError_t e = insar_set_lds_once(attr_mask, (const void*)Kernel, lds_bytes);
    if (e != hipSuccess) INSAR_FAIL(-(int)e, "%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
  }
  a.mtc = a.Cin / tm; a.ntc = a.Cout / tn;
  const long long grid = (long long)a.nsplit * 3 * a.mtc * a.ntc;
  if (grid > 0x7fffffffLL) INSAR_FAIL(INSAR_E_SHAPE, "%s: grid too large", name);
  hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(threads), lds_bytes, s, a);
  INSAR_CHECK_LAUNCH(name);
  return INSAR_OK;
}
