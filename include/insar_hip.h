/*
 * insar_hip.h — flat C ABI of libinsar_hip.so (gfx950 / MI355X).
 *
 * The reference (Createroner/InSAR-Unet-CA) has no FFI layer: its boundary is the
 * torch nn.Module API of Unet-ChannalAttention.py. This header is the thin C ABI the
 * Python host (insar_unet_ca_amd/) binds with ctypes; every entry point names the
 * reference arithmetic it replaces (file:line into /root/reference).
 *
 * Conventions
 *  - Every function returns 0 on success, a negative INSAR_E_* code or -hipError_t on
 *    failure; insar_last_error() returns a thread-local message. No C++ exception
 *    crosses the ABI.
 *  - The library never allocates, frees or synchronises: every buffer is caller-owned
 *    device memory (torch tensors passed as raw pointers); kernels are enqueued on the
 *    caller's hipStream_t (passed as void*) and the call returns immediately.
 *  - Activations are NHWC with a one-pixel zero halo: [B][H+2][W+2][C] elements of
 *    `dtype` (INSAR_F32 / INSAR_BF16). Kernels write interiors only, so the halo of a
 *    buffer allocated zeroed stays zero (that is what pads the 3x3 convolutions).
 *    An InsarAct describes a channel slice [c_off, c_off+c_len) of such a buffer, which
 *    is how the skip-concat (Unet-ChannalAttention.py:140,146,152,158) is zero-copy.
 */
#ifndef INSAR_HIP_H
#define INSAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INSAR_ABI_VERSION 8

enum { INSAR_F32 = 0, INSAR_BF16 = 1 };

enum {
  INSAR_OK = 0,
  INSAR_E_SHAPE = -1001, /* unsupported / inconsistent shape */
  INSAR_E_DTYPE = -1002,
  INSAR_E_ALIGN = -1003, /* pointer not 16-byte aligned */
  INSAR_E_WS = -1004,    /* workspace too small */
  INSAR_E_ARG = -1005
};

typedef struct InsarAct {
  void* ptr;     /* base of the padded buffer (pixel (-1,-1) of image 0, channel 0) */
  int32_t B, H, W; /* interior extent */
  int32_t C;     /* channels of the whole buffer (pixel pitch, elements) */
  int32_t c_off; /* first channel of the slice */
  int32_t c_len; /* channels in the slice */
  int32_t dtype; /* INSAR_F32 | INSAR_BF16 */
  int32_t _pad;
} InsarAct;

int insar_version(void);
const char* insar_last_error(void);

/* Kernel-variant selectors for same-process A/B measurements (tools/, bench.py --tune): named integer knobs read by
 * the launchers at launch time. Every value of every knob selects between kernels that the parity tests hold to
 * the same tolerances (tests/test_switch_routes_gpu.py, test_switch_wgrad_gpu.py, test_wgrad3_exact_gpu.py), except
 * wgrad3x_var, which only experiment builds read and the product library ignores; unknown names return INSAR_E_ARG. Not part of the reference's surface (it has no kernels). */
int insar_tune_set(const char* name, int32_t value);
int insar_tune_get(const char* name);   /* value, or INSAR_E_ARG */

/* ---- layout conversion at the nn.Module boundary (forward(x:[B,C,H,W]), :127) ------------ */
/* NCHW contiguous fp32 -> padded NHWC slice (cast to dst.dtype). */
int insar_pack_nchw(const float* src, const InsarAct* dst, void* stream);
/* padded NHWC slice -> NCHW contiguous fp32. */
int insar_unpack_nchw(const InsarAct* src, float* dst, void* stream);

/* ---- weight re-layout: torch fp32 parameter -> GEMM operand [t][n][k] of `dtype` ----------
 * out[(t*N + n)*K + k] = cast(in[t*st + n*sn + k*sk]).  Used for Conv2d (Co,Ci,3,3) weights
 * (:81,84), ConvTranspose2d (Ci,Co,2,2) weights (:112-121) in their forward and dgrad forms. */
int insar_weight_prep(const float* in, void* out, int32_t dtype, int32_t T, int32_t N, int32_t K,
                      int64_t st, int64_t sn, int64_t sk, void* stream);

/* batched form, one launch for every weight of the network. jobs (device): int64[njobs][10] =
 * {in*, out*, T, N, K, st, sn, sk, first_tile, dtype}; a job owns T*ceil(N/32)*ceil(K/32) consecutive tiles
 * starting at first_tile; total_tiles = sum over jobs. */
int insar_weight_prep_batch(const int64_t* jobs, int32_t njobs, int64_t total_tiles, void* stream);
/* Paired form: both GEMM layouts from one read of the fp32 master in[a][b][T] (T <= 9 taps contiguous):
 * out_ab[t][a][b] and out_ba[t][b][a]. jobs: int64[njobs][8] = {in*, out_ab*, out_ba*, A, B, T, first_tile,
 * dtype}; one work-group per 32x32 (a x b) tile, tiles numbered job after job. */
int insar_weight_prep_pair_batch(const int64_t* jobs, int32_t njobs, int64_t total_tiles, void* stream);

/* ---- implicit-GEMM convolution family (MFMA) ------------------------------------------------
 * y[pix(m), n] = sum_{tap, k} x[in_pix(m, tap), k] * w[tap][n][k]  (+ bias[n])
 *   m enumerates the out.B x Ho x Wo grid row-major; in_pix = (ho*stride + dy[tap], wo*stride + dx[tap]).
 * mode 0: Conv2d 3x3 pad 1 forward (:81,84) / its dgrad (flipped taps, transposed weights) /
 *         ConvTranspose2d dgrad (stride 2, taps {0,1}^2): out pixel (ho,wo), channel n.
 * mode 1: ConvTranspose2d(k=2,s=2) forward (:112,115,118,121): N = 4*Cout, n=(a*2+b)*Cout+co
 *         is scattered to out pixel (2ho+a, 2wo+b), channel co.
 * stats (nullable): per-M-tile partial column sums of the GEMM result as rounded to the output type, BEFORE bias / add
 *         (the raw, bias-free conv output insar_bn_finalize expects; without bias / add that is the stored output),
 *         float[insar_igemm_num_mtiles(M, N)][2][N] (sum, sum of squares) for BatchNorm (:82,85). */
/* BatchNorm-backward sums taken in the epilogue of the GEMM that PRODUCES a unit's incoming gradient ("bstat"), instead of
 * a pass of its own over (dout, y) (insar_bnrelu_bwd_reduce; :82-83,85-86 inside loss.backward(), :345): with g = the
 * stored output element and yv = y at the same (pixel, channel),
 *   stats[row][0][n] = sum_pixels g * [scale[n]*yv + shift[n] > 0],   stats[row][1][n] = sum_pixels g * [...] * yv
 * in the slab the forward statistics would use (same rows). y = the consumer unit's raw conv output in a buffer with the
 * OUTPUT's layout (same B, H, W, C, c_off, dtype); y == NULL switches the mode off. */
typedef struct InsarBstat {
  const void* y;
  const float* scale;
  const float* shift;
} InsarBstat;

typedef struct InsarIgemm {
  InsarAct x;          /* input slice, c_len = K per tap */
  InsarAct y;          /* output slice */
  const void* w;       /* [ntaps][N][K] of x.dtype */
  const float* bias;   /* nullable, per output channel */
  float* stats;        /* nullable */
  int32_t N;           /* GEMM N (mode 1: 4*Cout) */
  int32_t Ho, Wo;      /* GEMM row grid (per image) */
  int32_t stride;      /* 1 or 2 */
  int32_t ntaps;       /* 1, 4 or 9 */
  int32_t mode;        /* 0 | 1 */
  int8_t dy[12], dx[12];
  int32_t flags;       /* INSAR_IGEMM_* */
  int32_t out_stride;  /* mode 0: 0 / 1 = dense output; s > 1: GEMM row (ho, wo) is stored at output pixel (ho*s + out_oy, */
  int32_t out_oy, out_ox; /*   wo*s + out_ox) — one parity class of the input gradient of a stride-s convolution */
  int32_t _pad;
  const void* add;     /* nullable, mode 0: a tensor with y's buffer layout (same C, c_off, dtype), added to the result */
  InsarBstat bstat;    /* mode 0, dense output, with stats: BatchNorm-backward sums instead of (sum, sum of squares) */
  const void* gate;    /* nullable, mode 0, no stats (ABI 4): a tensor with y's buffer layout; the result (after bias / add) is stored as
                        * zero where it is <= 0 — the ReLU mask of a residual block's input applied to the block's input gradient by
                        * the GEMM that writes it (torchvision Bottleneck `out = relu(out + identity)`, DeepLabV3-ChannelAttention.py:95) */
} InsarIgemm;
/* flags. OOB_ZERO: taps may leave the padded input and read zeros there (dilated 3x3 convolutions of DeepLabV3's
 * layer3 / layer4 / ASPP, torchvision resnet.py / deeplabv3.py; the 1-pixel halo covers only |dy|,|dx| <= 1). */
enum { INSAR_IGEMM_OOB_ZERO = 1,
       INSAR_IGEMM_PINGPONG = 2 /* 256 x 256 bf16 tiles: the ping-pong K loop (csrc/igemm.hip); same results, bit for bit */ };
/* rows of the stats slab = number of M tiles the library will use for a GEMM with M rows and N columns
 * (the tile height, 128 or 256 pixels, is chosen from M and N so that the grid fills the 256 CUs). */
int insar_igemm_num_mtiles(int64_t M, int32_t N);
int insar_igemm_tile_rows(int64_t M, int32_t N);
int insar_igemm_tile_cols(int64_t M, int32_t N);   /* 128 or 64 output channels per tile (any dtype) */
int insar_igemm_tile_cols_dt(int64_t M, int32_t N, int32_t dtype);   /* + 256 (bf16, N % 256 == 0, >= 256 such tiles) */
int insar_igemm(const InsarIgemm* d, void* stream);

/* ---- 3x3 / stride-1 convolution over the flat padded pixel space (MFMA) -------------------------------
 * Same arithmetic as insar_igemm mode 0 with the 9 forward taps (Conv2d 3x3 pad 1 forward, :81,84, and its
 * input gradient with flip = 1), for large grids: the three dx taps of a dy share one LDS tile of input
 * rows, so A rows cross the L2->LDS path 3 times instead of 9. x and y cover the same B x H x W grid.
 * flip: bit 0 = walk the taps backwards (input gradient); bit 1 = the ping-pong K loop (bf16; same results bit for bit);
 * bit 2 = persistent work-groups (one per CU, each walking its tiles in the same XCD-aware order; same outputs bit for bit,
 * the statistics summed per work-group instead of per tile).
 * w: [9][N][K] in the raster order produced by insar_weight_prep; stats (nullable):
 * float[insar_conv3x3_flat_stat_rows(x, N, flip)][2][N]. insar_conv3x3_flat_ok() is the library's own
 * eligibility heuristic (enough tiles to fill the chip, W,H >= 30). */
int insar_conv3x3_flat_ok(const InsarAct* x, int32_t N);
int insar_conv3x3_flat_num_mtiles(const InsarAct* x);
/* Row tiles (flip bit 3 = 8; bf16): a tile is 256 REAL output pixels = 256 / W whole image rows, staged with their halo
 * pixels, so that the three dx taps share one staged tile as in the flat geometry while the tile count is M / 256 (the deep
 * levels of the U-Net, where the flat geometry's 254-pixel step breaks the one-round-of-work-groups grid). Needs W a power
 * of two in 16..256 and H a multiple of 256 / W: insar_conv3x3_flat_rows_ok. flip bit 4 = 16: 64-column tiles whatever N.
 * The statistics slab has insar_conv3x3_flat_stat_rows(x, N, flip) rows, with the same bits. Row tiles need K and N multiples
 * of 64 and have no persistent form: flip bit 2 together with bit 3 is INSAR_E_ARG. */
int insar_conv3x3_flat_rows_ok(const InsarAct* x, int32_t N);
/* Row tiles of a DILATED 3x3 convolution (padding = dilation; flip bits 8-11 carry the dilation, 0 = 1): taps that reach beyond
 * the one-pixel halo read zeros, as insar_igemm's INSAR_IGEMM_OOB_ZERO. Needs 256 / W * (W + 2 * dil) <= 320 besides the above. */
int insar_conv3x3_flat_rows_dil_ok(const InsarAct* x, int32_t N, int32_t dil);
/* flip bit 5 = 32 (bf16; K a multiple of 32, N of 64): the kernel built as TWO co-resident 4-wave work-groups per CU
 * (csrc/conv3x3_flat2.hip: 32-channel K slabs, 128 x 64 wave tiles; one group's prologue / epilogue under the other's K loop).
 * Flat geometry, or with bit 3 row tiles (W a power of two in 16..256, H a multiple of 256 / W: insar_conv3x3_flat2_rows_ok;
 * the halo pixels are not staged); bit 2 = persistent work-groups (two per CU) in both geometries. Results equal the 8-wave kernel's up to fp32
 * summation order (channels are added 32 by 32 instead of 64 by 64 per tap). Dilation bits with bit 5: INSAR_E_ARG. */
int insar_conv3x3_flat2_rows_ok(const InsarAct* x, int32_t N);
/* rows of the statistics slab for a launch with these flags: one per M tile, or one per work-group for persistent
 * work-groups (flip bit 2) with a single N tile, which carry the sums over their tiles */
int insar_conv3x3_flat_stat_rows(const InsarAct* x, int32_t N, int32_t flip);
int insar_conv3x3_flat(const InsarAct* x, const InsarAct* y, const void* w, int32_t flip, float* stats,
                       void* stream);
/* the same with BatchNorm-backward sums in the statistics slab (InsarBstat above; bstat->y has y's layout) */
int insar_conv3x3_flat_bstat(const InsarAct* x, const InsarAct* y, const void* w, int32_t flip, float* stats,
                             const InsarBstat* bstat, void* stream);

/* ---- 3x3 conv with 64 -> 64 channels, bf16 (the full-resolution level; :81,84 and their dgrad) -------
 * Persistent work-groups, weights in registers, activations through a rolling LDS window over the flat
 * padded pixel space (csrc/conv3x3_c64.hip). Same operands and tap order as insar_conv3x3_flat.
 * stats: [insar_conv3x3_c64_rows(x)][2][64] BatchNorm partial sums (one row per work-group) or null. */
int insar_conv3x3_c64_ok(const InsarAct* x, int32_t N);
int insar_conv3x3_c64_rows(const InsarAct* x);
/* host-side query of the rolling-window geometry: out[6] = {A, Af, o, R, ntiles, TILE}; 1 if the shape is accepted */
int insar_conv3x3_c64_geometry(const InsarAct* x, int32_t* out);
int insar_conv3x3_c64(const InsarAct* x, const InsarAct* y, const void* w, int32_t flip, float* stats,
                      void* stream);
/* the same with BatchNorm-backward sums in the statistics slab (InsarBstat; scale / shift 16-byte aligned) */
int insar_conv3x3_c64_bstat(const InsarAct* x, const InsarAct* y, const void* w, int32_t flip, float* stats,
                            const InsarBstat* bstat, void* stream);

/* ---- weight-gradient GEMM (MFMA, split-K over pixels, no atomics) ------------------------------
 * part[split][tap][co][ci] = sum_{p in split} dy[pixB(p,tap), co] * x[pixA(p,tap), ci]
 * with pixA/pixB given as int32 pixel-index tables (padded-buffer pixel index of tap (0,0) for
 * every flattened p, length Mpad = multiple of 64, tail entries 0 = a halo pixel) plus a per-tap
 * pixel offset. Covers Conv2d wgrad (x taps move) and ConvTranspose2d wgrad (dy taps move). */
typedef struct InsarWgrad {
  InsarAct x;             /* c_len = Cin */
  InsarAct dy;            /* c_len = Cout */
  const int32_t* tabx;    /* [Mpad] */
  const int32_t* tabdy;   /* [Mpad] */
  float* part;            /* [nsplit][ntaps][Cout][Cin] fp32 */
  int64_t Mpad;           /* padded pixel count (multiple of 64) */
  int32_t nsplit;
  int32_t ntaps;
  int32_t offx[12];       /* per-tap pixel offset added to tabx entries */
  int32_t offdy[12];      /* per-tap pixel offset added to tabdy entries */
  int64_t tabx_tap_stride; /* 0: tabx serves every tap (offx moves it); else tap t reads tabx + t*tabx_tap_stride (per-tap
                            * tables from insar_pixel_table_taps: strided / dilated convolutions, out-of-bounds -> pixel 0) */
} InsarWgrad;
/* tile extent the kernel uses along a channel dimension of C channels: 64 | 128 | 256 (256 only when both
 * Cin and Cout allow it, otherwise capped at 128); needed by callers that size the split-K factor. */
int insar_wgrad_tile(int32_t C, int32_t dtype);
/* the (Cin, Cout) tile of a layer as (tile(Cin) << 16) | tile(Cout): 256x256 (8 waves), 128x128, 128x64, 64x128,
 * 64x64 in bf16; 128x128 (8 waves) or 64x64 in fp32. */
int insar_wgrad_tile_pair(int32_t Cin, int32_t Cout, int32_t dtype);
int insar_wgrad(const InsarWgrad* d, void* stream);
/* The same slabs for a 3x3 / stride-1 / pad-1 convolution (Unet-ChannalAttention.py:81,84; tap = 3*ty + tx) from a
 * kernel whose work-groups compute the three taps of a kernel row together: dy staged once per 64-pixel K step, x
 * once with a one-pixel lead and tail, a third of the LDS-DMA pieces of insar_wgrad (which these layers are bound by).
 * x (B,H,W,Cin), dy (B,H,W,Cout) on the same grid, part[nsplit][9][Cout][Cin]. insar_wgrad_conv3_tile returns
 * (tile(Cin) << 16) | tile(Cout) (tiles <= 128), or 0 when the layer needs insar_wgrad (W neither a multiple of 64
 * nor 16 / 32). */
int insar_wgrad_conv3_tile(const InsarAct* x, int32_t Cout);
int insar_wgrad_conv3(const InsarAct* x, const InsarAct* dy, float* part, int32_t nsplit, void* stream);
/* The same slabs again (bit for bit insar_wgrad_conv3's at the same nsplit) for the bf16 layers with >= 256 channels on one
 * side and >= 128 on the other, from 256 x 128 (Cin x Cout; 128 x 256 where only Cout has 256) tiles: 8 waves of 64 x 64 x
 * three taps, a K step as six [fragment reads + LDS-DMA issue | 16 MFMAs] phases with the two waves of a SIMD in opposite
 * roles, a three-slot LDS ring whose only vector-memory wait is a counted one per K step (csrc/wgrad3x.hip).
 * insar_wgrad_conv3x_tile: (tile(Cin) << 16) | tile(Cout), or 0 where the layer keeps insar_wgrad_conv3. */
int insar_wgrad_conv3x_tile(const InsarAct* x, int32_t Cout);
int insar_wgrad_conv3x(const InsarAct* x, const InsarAct* dy, float* part, int32_t nsplit, void* stream);
/* ... and from 128 x 128 tiles by 4-wave work-groups built to run TWO PER CU (csrc/wgrad3y.hip: the same 64 x 64 x three-tap wave
 * tiles and LDS image, a two-slot LDS ring of 34 KB stages, one barrier per K step, the two work-groups of a CU not coupled at all):
 * bf16 layers with both channel counts multiples of 128. insar_wgrad_conv3y_tile: (128 << 16) | 128, or 0. */
int insar_wgrad_conv3y_tile(const InsarAct* x, int32_t Cout);
int insar_wgrad_conv3y(const InsarAct* x, const InsarAct* dy, float* part, int32_t nsplit, void* stream);
/* The same decomposition for the bf16 layers with 64 or 128 channels on BOTH sides (the 256^2 / 128^2 levels): the tile is
 * too small to give eight waves a 64 x 64 x three-tap tile each, so the waves of a work-group split the PIXELS of a K step
 * (KS = 8 / wave tiles slices of 32 pixels) and a work-group writes KS slabs: part[nsplit * KS][9][Cout][Cin], folded by
 * insar_wgrad_reduce over nsplit * KS slabs (csrc/wgrad3k.hip). Slab split * KS + slice holds the products of pixels
 * [slice * 32, slice * 32 + 32) of each of the split's K steps. A K step (KS * 32 pixels) must lie inside one image row:
 * insar_wgrad_conv3k_tile returns (tile(Cin) << 16) | tile(Cout) or 0 (insar_wgrad_conv3 then), _slices returns KS.
 * The sums are partitioned differently from insar_wgrad_conv3's: equal to fp32 summation order, not bit for bit. */
int insar_wgrad_conv3k_tile(const InsarAct* x, int32_t Cout);
int insar_wgrad_conv3k_slices(const InsarAct* x, int32_t Cout);
int insar_wgrad_conv3k(const InsarAct* x, const InsarAct* dy, float* part, int32_t nsplit, void* stream);
/* grad = sum_split part[...] re-laid out to the torch parameter layout.
 * layout 0: Conv2d (Co,Ci,kh,kw): grad[(co*Ci+ci)*ntaps + tap]
 * layout 1: ConvTranspose2d (Ci,Co,2,2): grad[(ci*Co+co)*ntaps + tap]
 * accumulate != 0 adds into grad instead of overwriting. */
int insar_wgrad_reduce(const float* part, float* grad, int32_t nsplit, int32_t ntaps, int32_t Co,
                       int32_t Ci, int32_t layout, int32_t accumulate, void* stream);
/* first stage of the fold when nsplit is large: part_out[g] = sum of `group` consecutive slabs of
 * part_in (slab_floats = ntaps*Co*Ci); the result feeds insar_wgrad_reduce with nsplit = ceil(nsplit/group). */
int insar_wgrad_fold(const float* part_in, float* part_out, int64_t slab_floats, int32_t nsplit,
                     int32_t group, void* stream);
/* pixel-index table for a B x H x W grid mapped with stride s into a padded buffer of interior
 * (Hb, Wb): tab[p] = (n*(Hb+2) + h*s + 1)*(Wb+2) + w*s + 1 ; entries p >= B*H*W are `tail`
 * (0 = a zero halo pixel for the operand whose taps do not move; Wb+3 = the first interior pixel,
 * in bounds under every 3x3 tap, for the operand whose taps move). */
int insar_pixel_table(int32_t* tab, int64_t Mpad, int32_t B, int32_t H, int32_t W, int32_t s,
                      int32_t Hb, int32_t Wb, int32_t tail, void* stream);

/* ---- first layer: direct 3x3 conv for tiny Cin (inc.double_conv.0, Cin<=4; :81 with :464) ---- */
/* rows of the statistics slab insar_conv3x3_small_fwd writes for this (x, y): stats[rows][2][Cout] */
int insar_conv3x3_small_fwd_rows(const InsarAct* x, const InsarAct* y);
int insar_conv3x3_small_fwd(const InsarAct* x, const float* w /*torch (Co,Ci,3,3) fp32*/,
                            const InsarAct* y, float* stats /*[B*H][2][Co]*/, void* stream);
/* part: [insar_conv3x3_small_wgrad_blocks(B,H)][Co*Ci*9] partial rows (torch (Co,Ci,3,3) order). */
int insar_conv3x3_small_wgrad_blocks(int32_t B, int32_t H);
int insar_conv3x3_small_wgrad(const InsarAct* x, const InsarAct* dy, float* part, void* stream);
/* The same with the unit's BatchNorm / ReLU backward apply pass (insar_bnrelu_bwd_apply without an SE gate) evaluated on the
 * way in: dy — which only this launch would read, the network's first layer having no input gradient (:81 under :345) — is never
 * written. g: the unit's incoming gradient, y: its conv output; bf16, Cin = 2, Cout = 64, W % 64 == 0 (insar_..._fused_ok).
 * Bit for bit the two launches it replaces. */
int insar_conv3x3_small_wgrad_fused_ok(const InsarAct* x, const InsarAct* y);
int insar_conv3x3_small_wgrad_fused(const InsarAct* x, const InsarAct* g, const InsarAct* y, const float* scale,
                                    const float* shift, const float* mean, const float* invstd, const float* k1,
                                    const float* k2, int32_t relu, float* part, void* stream);

/* ---- segmented column sum of partial slabs: out[s][c] (+)= sum_r part[s][r][c] ---------------
 * Two-stage (deterministic, no atomics) when rows > 256: stage 1 writes into `tmp`
 * (>= ceil(rows/128)*segments*cols floats), stage 2 folds it. */
int insar_colsum(const float* part, float* out, int32_t segments, int64_t rows, int32_t cols,
                 int32_t accumulate, float* tmp, int64_t tmp_floats, void* stream);
/* The same over the first `cols` columns of rows that are `ld` >= cols floats apart: a bias / 1x1-weight gradient summed
 * straight into its place in the flat gradient buffer (no staging tensor and no device copy behind it). */
int insar_colsum_ld(const float* part, float* out, int32_t segments, int64_t rows, int32_t cols, int64_t ld,
                    int32_t accumulate, float* tmp, int64_t tmp_floats, void* stream);

/* first stage only: out[ceil(rows/rps)][cols]; insar_bn_finalize folds the remaining rows itself. */
int insar_colsum_partial(const float* part, float* out, int64_t rows, int32_t cols, int32_t rps,
                         void* stream);

/* ---- BatchNorm2d (+ReLU) (:82-83, :85-86) -------------------------------------------------------
 * finalize: from `rows` (<= 4096) remaining partial rows part[rows][2][C] (sum, sum of squares) of
 * the raw (bias-free) conv output over `count` pixels (larger slabs go through insar_colsum first): batch mean/var -> scale = gamma*invstd, shift = beta - mean*scale; running stats
 * (momentum, unbiased var; the conv bias is added to the mean) and num_batches_tracked.
 * training == 0: scale/shift from the running stats (+ conv bias), slabs ignored. */
typedef struct InsarBnFinalize {
  const float* part; int64_t rows; int64_t count; int32_t C; int32_t training;
  const float* conv_bias; const float* gamma; const float* beta;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;
  float momentum; float eps;
  float* scale; float* shift; float* mean; float* invstd; /* outputs, [C] each */
} InsarBnFinalize;
int insar_bn_finalize(const InsarBnFinalize* d, void* stream);
/* z = relu(y*scale + shift) * gate[n][c] (gate nullable) -> dst slice. `relu` = 0 drops the ReLU
 * (and the mask in the reductions below): that is the stand-alone SELayer applied to a raw tensor. */
int insar_bn_relu_apply(const InsarAct* y, const float* scale, const float* shift,
                        const float* gate /*[B][C] or null*/, const InsarAct* dst, int32_t relu,
                        void* stream);

/* the same pass for an encoder block, writing the 2x2 max-pool (:106-109) of dst as well: pooled is the
 * (B, H/2, W/2, C) slice; identical to insar_bn_relu_apply followed by insar_maxpool2_fwd, one read less. */
int insar_bn_relu_apply_pool(const InsarAct* y, const float* scale, const float* shift, const float* gate,
                             const InsarAct* dst, const InsarAct* pooled, int32_t relu, void* stream);

/* ---- SELayer (:45-72) ----------------------------------------------------------------------------
 * squeeze: partial sums of mask and mask*y, mask = (y*scale+shift > 0), over `rows_per_part` consecutive
 *   image rows: part[B][P][2][C], P = ceil(H / rows_per_part). */
int insar_se_squeeze(const InsarAct* y, const float* scale, const float* shift, float* part,
                     int32_t relu, int32_t rows_per_part, void* stream);
/* excitation: mean -> Linear(C,C/r) -> ReLU -> Linear(C/r,C) -> Sigmoid (two bias-free Linears,
 * :54-59). Saves sq[B][C] (the squeezed mean), hid[B][Cr] (post-ReLU), gate[B][C]. */
typedef struct InsarSeFwd {
  const float* part;   /* squeeze slabs [B][rows][2][C] (insar_se_squeeze: rows = P), folded in-kernel */
  int32_t B, H, W, C, Cr; int32_t rows;
  const float* scale; const float* shift;
  const float* w1; /* (Cr, C) */ const float* w2; /* (C, Cr) */
  float* pooled; /* out [B][2][C]: per image sum of mask, sum of mask*y (kept for backward) */
  float* sq; float* hid; float* gate;
} InsarSeFwd;
int insar_se_excite(const InsarSeFwd* d, void* stream);

/* ---- backward of [BN -> ReLU -> (SE gate)] ------------------------------------------------------
 * reduce: part[B][P][2][C] = sums over `rows_per_part` image rows of  g*mask  and  g*mask*y , g = dout (T),
 *   P = ceil(H / rows_per_part).  */
int insar_bnrelu_bwd_reduce(const InsarAct* dout, const InsarAct* y, const float* scale,
                            const float* shift, float* part, int32_t relu, int32_t rows_per_part, void* stream);
/* coefficient kernels: turn the reduce slabs red[B][rows][2][C] (insar_bnrelu_bwd_reduce: rows = P;
 * folded per image in-kernel) into everything the apply pass needs.
 *  with SE:  ds -> MLP backward (dW1, dW2, dsq);  g_eff = (dout*gate + dsq/HW) on the ReLU mask
 *  dgamma/dbeta; coefB[B][C] = dsq/HW and per-channel k1[C] = dbeta/N, k2[C] = dgamma/N (0 in eval):
 *    dy = scale_c * ( (dout*gate + coefB)*mask - k1 - xhat*k2 ).
 *  dconv_bias (nullable): gradient of the bias of the conv feeding this BN: exactly 0 in training
 *  (the batch mean removes it), scale*dbeta in eval.
 *  ws: float[B*(3C + Cr)] scratch. */
typedef struct InsarBnSeBwd {
  int32_t B, H, W, C, Cr; int32_t use_se;
  const float* mean; const float* invstd;
  const float* pooled; const float* sq; const float* hid; const float* gate;
  const float* w1; const float* w2;
  float* dw1; float* dw2; float* dgamma; float* dbeta;
  float* coefB; float* k1; float* k2;
  int32_t accumulate; int32_t _pad;
} InsarBnSeBwd;
int insar_bnse_bwd_coef(const InsarBnSeBwd* d, const float* red, int32_t rows, const float* scale,
                        const float* shift, float* ws, float* dconv_bias, int32_t training, void* stream);
/* The same in ONE launch: the work-group that finishes stage 1 last (a ticket counter; the hand-off data written through
 * to memory and read past the caches) runs stage 2. ticket: a zero-initialised 32-bit device word per call site (the
 * kernel resets it); bitwise the results of insar_bnse_bwd_coef. Pays for units without an SE gate, whose stage 2 is small. */
int insar_bnse_bwd_coef_fused(const InsarBnSeBwd* d, const float* red, int32_t rows, const float* scale,
                              const float* shift, float* ws, float* dconv_bias, int32_t training, uint32_t* ticket,
                              void* stream);
/* Units WITHOUT an SE gate (d->use_se == 0): the coefficients (k1, k2, dgamma, dbeta, conv-bias gradient) from ALL
 * `rows_total` rows of the reduction slab red[rows_total][2][C] in one channel-parallel launch; any partition of the pixels
 * into rows will do (BatchNorm backward, :82-83,85-86 inside loss.backward(), :345). */
int insar_bn_bwd_coef(const InsarBnSeBwd* d, const float* red, int64_t rows_total, const float* scale,
                      float* dconv_bias, int32_t training, void* stream);
int insar_bnrelu_bwd_apply(const InsarAct* dout, const InsarAct* y, const float* scale,
                           const float* shift, const float* mean, const float* invstd,
                           const float* gate, const float* coefB, const float* k1,
                           const float* k2, const InsarAct* dy, int32_t relu, void* stream);
/* The two stages of insar_bnse_bwd_coef on their own (stage = 1: per-image stage — SE backward, coefB and the
 * per-image partial sums tb/tg in ws; stage = 2: batch fold — k1, k2, dgamma, dbeta, dW1, dW2, conv-bias gradient),
 * and the apply pass that folds k1[c] = sum_n tb[n][c] / (B*H*W), k2[c] = sum_n tg[n][c] / (B*H*W) itself
 * (training mode; tb = ws + B*(C+Cr), tg = tb + B*C; C <= 1024). With these the input-gradient chain
 * (loss.backward(), Unet-ChannalAttention.py:345) needs only stage 1; stage 2 runs beside it on another stream.
 * Bitwise the same dy as insar_bnse_bwd_coef + insar_bnrelu_bwd_apply. */
int insar_bnse_bwd_coef_stage(const InsarBnSeBwd* d, const float* red, int32_t rows, const float* scale,
                              const float* shift, float* ws, float* dconv_bias, int32_t training, int32_t stage,
                              void* stream);
int insar_bnrelu_bwd_apply_part(const InsarAct* dout, const InsarAct* y, const float* scale, const float* shift,
                                const float* mean, const float* invstd, const float* gate, const float* coefB,
                                const float* tb, const float* tg, const InsarAct* dy, int32_t relu, void* stream);

/* ---- MaxPool2d(2) backward inside the encoder block's BatchNorm-backward passes -----------------------------------
 * insar_bn_relu_apply_pool_arg is insar_bn_relu_apply_pool that also records which element of each 2x2 window is
 * the maximum (arg[B][H/2][W/2][C] bytes 0..3 = 2*(row parity) + (column parity); insar_maxpool2_bwd's rule on the
 * stored values). The _pool variants of the reduce and apply passes then take
 *   dout = round_T(dskip + (arg == position ? dpooled : 0))
 * on the fly — the expression insar_maxpool2_bwd evaluates when it accumulates into dskip — so that launch (a read of
 * the full-resolution activation and a read-modify-write of its gradient) is not needed. Bitwise the same results. */
int insar_bn_relu_apply_pool_arg(const InsarAct* y, const float* scale, const float* shift, const float* gate,
                                 const InsarAct* dst, const InsarAct* pooled, uint8_t* arg, int32_t relu, void* stream);
int insar_bnrelu_bwd_reduce_pool(const InsarAct* dskip, const InsarAct* dpooled, const uint8_t* arg, const InsarAct* y,
                                 const float* scale, const float* shift, float* part, int32_t relu,
                                 int32_t rows_per_part, void* stream);
int insar_bnrelu_bwd_apply_pool(const InsarAct* dskip, const InsarAct* dpooled, const uint8_t* arg, const InsarAct* y,
                                const float* scale, const float* shift, const float* mean, const float* invstd,
                                const float* gate, const float* coefB, const float* k1, const float* k2,
                                const InsarAct* dy, int32_t relu, void* stream);

/* ---- the unit that feeds the 1x1 output conv (outc, Unet-ChannalAttention.py:125,162) ----------------------------
 * Its incoming gradient is g[n,h,w,c] = round_T(sum_k dlogits[n,k,h,w] * W[k][c]): 2K multiply-adds per element, so the
 * reduce and apply passes recompute it from dlogits (fp32 [B][K][H][W], K <= 4) and outc's weight ([K][C] fp32)
 * instead of reading a materialised 64-channel tensor, and insar_conv1x1_out_wgrad produces outc's parameter
 * gradients (part as insar_conv1x1_out_bwd) without writing that tensor. Bitwise the same results as
 * insar_conv1x1_out_bwd + insar_bnrelu_bwd_reduce + insar_bnrelu_bwd_apply, three activation-sized HBM passes less. */
int insar_conv1x1_out_wgrad(const InsarAct* x, const float* w, const float* dlogits, int32_t K, float* part, void* stream);
/* Forward counterpart: the last unit's BN/ReLU/gate pass hands z straight to outc and writes only the logits
 * (fp32 [B][K][H][W], K <= 4; bitwise insar_bn_relu_apply + insar_conv1x1_out_fwd); outc's parameter gradients then
 * come from insar_conv1x1_out_wgrad_y, which recomputes z = round(relu(y*scale+shift) * gate[n]) from y. */
int insar_bn_relu_apply_outc(const InsarAct* y, const float* scale, const float* shift, const float* gate /*nullable*/,
                             const float* wout, const float* bias /*nullable*/, float* logits, int32_t K, int32_t relu,
                             void* stream);
int insar_conv1x1_out_wgrad_y(const InsarAct* y, const float* scale, const float* shift, const float* gate /*nullable*/,
                              const float* w, const float* dlogits, int32_t K, float* part, void* stream);
/* wpart (nullable; gate [B][C] nullable): the same pass also writes the output conv's parameter-gradient partials,
 * wpart[B * ceil(H / rows_per_part)][K*C + K] in the layout of insar_conv1x1_out_wgrad_y's `part` (fold with insar_colsum):
 * the weight gradient of the output conv then needs no pass of its own over y. */
int insar_bnrelu_bwd_reduce_outc(const float* dlogits, const float* wout, int32_t K, const InsarAct* y,
                                 const float* scale, const float* shift, float* part, int32_t relu,
                                 int32_t rows_per_part, const float* gate, float* wpart, void* stream);
int insar_bnrelu_bwd_apply_outc(const float* dlogits, const float* wout, int32_t K, const InsarAct* y,
                                const float* scale, const float* shift, const float* mean, const float* invstd,
                                const float* gate, const float* coefB, const float* k1, const float* k2,
                                const InsarAct* dy, int32_t relu, void* stream);

/* ---- ChannelAttentionModule (DeepLabV3-ChannelAttention.py:49-79; config 5) ---------------------------
 * out = x * sigmoid(W2 relu(W1 avg_hw(x)) + W2 relu(W1 max_hw(x))), W1 (Cr,C), W2 (C,Cr), no biases.
 * forward : insar_cam_pool -> insar_cam_excite -> insar_bn_relu_apply(x, ones, zeros, gate, out, relu=0)
 * backward: insar_bnrelu_bwd_reduce(dout, x, ones, zeros, red, relu=0) -> insar_cam_bwd_coef ->
 *           insar_bnrelu_bwd_apply(dout, x, ones, zeros, zeros, ones, gate, coefB, zeros, zeros, dx, relu=0)
 *           -> insar_cam_scatter_max(dx, dmax, arg)
 * pool: per part (image, rows_per_part consecutive rows) and channel the sum, the maximum and the flat
 * index h*W+w of its first occurrence: psum/pmax/parg[B][P][C], P = ceil(H / rows_per_part). */
typedef struct InsarCam {
  int32_t B, H, W, C, Cr; int32_t rows;            /* rows = P of the pool slabs */
  const float* psum; const float* pmax; const int32_t* parg;
  const float* w1; const float* w2;
  float* avg; float* mx; int32_t* arg;             /* [B][C] saved for backward */
  float* ha; float* hm;                            /* [B][Cr] post-ReLU hidden activations of the two branches */
  float* gate;                                     /* [B][C] */
  float* coefB; float* dmax;                       /* backward: [B][C] mean-branch term /HW, max-branch term */
  float* ws;                                       /* backward scratch: float[B*(C + 2*Cr)] */
  float* dw1; float* dw2;
  int32_t accumulate; int32_t _pad;
} InsarCam;
int insar_cam_pool(const InsarAct* x, float* psum, float* pmax, int32_t* parg, int32_t rows_per_part,
                   void* stream);
int insar_cam_excite(const InsarCam* d, void* stream);
int insar_cam_bwd_coef(const InsarCam* d, const float* red /*[B][rows][2][C]*/, int32_t rows, void* stream);
int insar_cam_scatter_max(const InsarAct* dx, const float* dmax, const int32_t* arg, void* stream);

/* ---- SpatialAttention (Unet-SpatialAttention.py:59-82, applied to each skip-concat at :131,137,143,149) ----------
 * a = cat(mean_c x, max_c x); z = ReLU(BN2(conv(ReLU(BN1(conv(a, w1) + b1)), w2) + b2)); out = x * sigmoid(z).
 * forward : insar_sa_compress -> insar_sa_conv(1) -> insar_bn_finalize(BN1, part = stat1, C = 1) -> insar_sa_conv(2)
 *           -> insar_bn_finalize(BN2, part = stat2, C = 1) -> insar_sa_gate
 *           (eval: the finalize calls read the running statistics; stat1 / stat2 are not written)
 * backward: insar_sa_dscale -> insar_sa_bwd_coef(2) -> insar_sa_bwd_stencil(2) -> insar_sa_bwd_coef(1)
 *           -> insar_sa_bwd_stencil(1) -> insar_sa_bwd_coef(0) -> insar_sa_dx
 * The arg-max is the FIRST channel holding the maximum (torch.max(dim=1)); only that channel receives d max.
 * C (= x.c_len) must be a multiple of 8. The fp32 maps are [B][H][W] unless noted; every reduction is a fixed
 * partition of the image rows over `rows` work-groups, folded in a fixed order (bitwise reproducible). */
typedef struct InsarSa {
  InsarAct x;          /* the concat (un-gated) */
  InsarAct y;          /* forward: gated output (same geometry and dtype); backward: d out, overwritten with d x */
  float* comp;         /* [B][H+2][W+2][2] (mean, max), zero halo */
  uint16_t* arg;       /* first arg-max channel */
  float* z1; float* z2;  /* raw conv outputs (without bias) */
  float* s;            /* sigmoid gate */
  float* g2; float* g1;  /* backward: gradient wrt the BN2 / BN1 outputs (ReLU mask applied) */
  float* dcomp;        /* backward: [B][H][W][2] (d mean, d max) */
  float* stat1; float* stat2;  /* forward: [rows][2] BatchNorm partial sums (sum, sum of squares) */
  float* part;         /* backward: [rows][20] partial sums */
  int32_t rows;        /* work-groups of the row-partitioned passes, 1..4096 */
  int32_t training;
  const float* w1; const float* w2;  /* conv weights (1,2,3,3), (1,1,3,3) */
  const float* bn;     /* [8] scale1, shift1, mean1, invstd1, scale2, shift2, mean2, invstd2 (insar_bn_finalize outputs) */
  float* coef;         /* [4] backward: BN2 k1, k2; BN1 k1, k2 */
  float* dw1; float* db1; float* dgamma1; float* dbeta1;   /* gradients (db1 / db2 nullable) */
  float* dw2; float* db2; float* dgamma2; float* dbeta2;
} InsarSa;
int insar_sa_compress(const InsarSa* d, void* stream);
int insar_sa_conv(const InsarSa* d, int32_t which /* 1 | 2 */, void* stream);
int insar_sa_gate(const InsarSa* d, void* stream);
int insar_sa_dscale(const InsarSa* d, void* stream);
int insar_sa_bwd_coef(const InsarSa* d, int32_t stage /* 2, 1, 0 */, void* stream);
int insar_sa_bwd_stencil(const InsarSa* d, int32_t which /* 2 | 1 */, void* stream);
int insar_sa_dx(const InsarSa* d, void* stream);

/* ---- MaxPool2d(2) (:106-109): y is the (H/2, W/2) grid rounded down (an odd last row / column belongs to no window) ---- */
int insar_maxpool2_fwd(const InsarAct* x, const InsarAct* y, void* stream);
/* dx (+)= route(dy) to the first maximum in scan order (torch semantics). */
int insar_maxpool2_bwd(const InsarAct* x, const InsarAct* dy, const InsarAct* dx, int32_t accumulate,
                       void* stream);

/* ---- F_T.resize(x, size, BILINEAR) of an NHWC slice (:138-139,144-145,150-151,156-157: the decoder's fallback for tile
 * sizes that are not multiples of 16), bilinear with align_corners = False, and its adjoint. src / dst: any two grids with
 * the same batch, channel slice width and dtype. */
int insar_resize_bilinear_fwd(const InsarAct* src, const InsarAct* dst, void* stream);
int insar_resize_bilinear_bwd(const InsarAct* ddst, const InsarAct* dsrc, void* stream);

/* ---- outc: Conv2d(64, num_classes, 1) (:125,162) ------------------------------------------------ */
int insar_conv1x1_out_fwd(const InsarAct* x, const float* w /*(K,C)*/, const float* bias,
                          float* logits /*NCHW fp32*/, int32_t K, void* stream);
/* dx slice <- dlogits * W ; part[insar_conv1x1_out_bwd_blocks(B,H)][K*C + K] partial (dW, dbias) sums. */
int insar_conv1x1_out_bwd_blocks(int32_t B, int32_t H);
int insar_conv1x1_out_bwd(const InsarAct* x, const float* w, const float* dlogits, int32_t K,
                          const InsarAct* dx, float* part, void* stream);

/* ---- loss entry: CrossEntropyLoss(ignore_index) (:465,344), fused forward + gradient ----------- */
/* ws: float[2 + 2*blocks] scratch (blocks = insar_ce_blocks(npix)); loss_out[0] = mean loss,
 * dlogits = (softmax - onehot)/n_valid on valid pixels, 0 elsewhere. */
int insar_ce_blocks(int64_t npix);
int insar_cross_entropy(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW,
                        int64_t ignore_index, float* dlogits, float* loss_out, float* ws, void* stream);
/* soft-Dice on softmax probabilities (build-side addition; the reference has no Dice). */
int insar_dice(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW,
               int64_t ignore_index, float smooth, float* dlogits, float* loss_out, float* ws,
               void* stream);

/* ce_weight*CE + dice_weight*Dice in one statistics pass + one gradient pass. ws: float[3 + 3K + blocks*(2 + 3K)];
 * loss_out[0] = combined, [1] = CE, [2] = Dice; dlogits = gradient of the combined loss. */
int insar_dice_ce(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW,
                  int64_t ignore_index, float smooth, float ce_weight, float dice_weight, float* dlogits,
                  float* loss_out, float* ws, void* stream);

/* ---- imbalance-aware losses (build-side addition): csrc/loss_weighted.hip -------------------------------------------
 * Same conventions as the three entry points above. A pixel is valid when its target is not ignore_index and lies in
 * [0, K); K <= 16. weight / alpha: device float[K], read by the kernels (never by the host), so the launch arguments do
 * not change from step to step. Results are bitwise reproducible (block partials folded in fixed order).
 *
 * Class-weighted, label-smoothed CE with torch's mean reduction (divide by W = sum of w[target] over valid pixels).
 * ws: float[2 + 2*blocks]; dlogits = [(1-e) w[y] (p - onehot) + (e/K) (S p - w)] / W, S = sum of the weights. */
int insar_cross_entropy_w(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW,
                          int64_t ignore_index, const float* weight, float label_smoothing, float* dlogits,
                          float* loss_out, float* ws, void* stream);
/* Focal loss: mean over valid pixels of alpha[y] (1 - p_t)^gamma (-log p_t); alpha nullable (ones); 0 <= gamma <= 64.
 * ws: float[2 + 2*blocks]. */
int insar_focal(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW, int64_t ignore_index,
                float gamma, const float* alpha, float* dlogits, float* loss_out, float* ws, void* stream);
/* ce_weight * (weighted / smoothed CE; or focal with alpha = weight when focal_gamma >= 0) + dice_weight * Dice (unweighted),
 * one statistics pass + one gradient pass like insar_dice_ce. weight nullable (ones); focal_gamma < 0 = no focal term;
 * label smoothing and focal do not combine. ws: float[4 + 3K + blocks*(3 + 3K)]; loss_out[0..2] = combined, CE term, Dice. */
int insar_dice_ce_w(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW,
                    int64_t ignore_index, float smooth, float ce_weight, float dice_weight, const float* weight,
                    float label_smoothing, float focal_gamma, float* dlogits, float* loss_out, float* ws,
                    void* stream);
/* Per-class pixel counts: counts[c] += pixels with target c (c < K), counts[K] += pixels equal to ignore_index. The call
 * ADDS to counts (the caller clears it once and accumulates batches); other labels are counted nowhere.
 * ws: int64[(K + 1) * blocks], blocks = insar_ce_blocks(npix). */
int insar_label_hist(const int64_t* target, int64_t npix, int32_t K, int64_t ignore_index, int64_t* counts,
                     int64_t* ws, void* stream);

/* ---- metrics (compute_metrics, :215-269): argmax (ties -> lower class) + TP/FP/FN counts -------- */
int insar_confusion(const float* logits, const int64_t* target, int32_t B, int32_t K, int64_t HW,
                    int64_t ignore_index, int64_t* counts /*[3][K], zeroed by the call*/, void* stream);

/* ---- whole-scene inference (build-side addition; the reference stops at fixed-size tiles): csrc/scene.hip -----------
 * A scene [H][W] (row-major, one channel) is cut into T x T tiles whose origins (y0, x0) the caller lists in a device
 * table int32 [n][2]; every tile lies inside the scene (infer.plan_tiles; there is no padding path). T is a multiple of
 * 16, 0 <= overlap <= T / 2, 2 <= K <= 8 classes (INSAR_E_SHAPE otherwise). All three validate before they launch. */
enum { INSAR_SCENE_U8 = 0, INSAR_SCENE_F32 = 1 };
/* out [n][1][T][T] fp32 (16-byte aligned) <- the n tiles. A uint8 scene gets the reference's ToTensor + Normalize(0.5, 0.5)
 * in its order, x = v / 255.0f; out = (x - 0.5f) / 0.5f (Unet-ChannalAttention.py:428-432); a float32 scene is copied. A table
 * entry that is not inside the scene gives a tile of zeros. */
int insar_scene_gather(const void* scene, int32_t dtype /*INSAR_SCENE_**/, int32_t H, int32_t W, const int32_t* origins,
                       int32_t n, int32_t T, float* out /*[n][1][T][T]*/, void* stream);
/* acc [K][H][W] += w * softmax_k(logits), wsum [H][W] += w for every pixel under the n tiles of `logits` [n][K][T][T]
 * (fp32 NCHW, what every net returns). Softmax over the class axis, max-subtracted, fp32. w(y, x) = r(y - y0) * r(x - x0),
 * r(i) = min(i + 1, T - i, overlap + 1) / (overlap + 1): strictly positive, 1 for overlap = 0, and two tiles at the regular
 * stride T - overlap sum to 1 across their overlap. Gather form, no atomics: the thread that owns a pixel adds the covering
 * tiles of this call in ascending table index (acc = fma(w, p, acc)), so feeding the tiles of a scene in index order in
 * batches of ANY size on one stream gives bitwise the same acc / wsum. [y_lo, y_hi) x [x_lo, x_hi) is a box of scene pixels
 * that contains every tile of the call (the caller knows the origins; the library reads nothing back): pixels outside it
 * are not visited. A table entry that is not inside the scene is ignored. The caller zeroes acc / wsum before the first
 * batch of a scene. */
int insar_scene_blend(const float* logits, const int32_t* origins, int32_t n, int32_t K, int32_t T, int32_t overlap,
                      float* acc, float* wsum, int32_t H, int32_t W, int32_t y_lo, int32_t y_hi, int32_t x_lo, int32_t x_hi,
                      void* stream);
/* prob [K][H][W] = acc / wsum (nullable: skipped), mask [H][W] uint8 = argmax over classes (ties -> lower class, the rule of
 * insar_confusion), conf [H][W] = the winning probability. A pixel with wsum == 0 (no tile) gets prob = 0, mask = 0, conf = 0. */
int insar_scene_finalize(const float* acc, const float* wsum, int32_t K, int32_t H, int32_t W, float* prob /*nullable*/,
                         uint8_t* mask, float* conf, void* stream);

/* ---- scenes with no-data: csrc/scene_valid.hip ------------------------------------------------------------------------------
 * A pixel of the scene is VALID iff its byte of the plane `valid` (uint8 [H][W], nullable: every pixel counts as observed) is
 * non-zero, its value is not `nodata` (looked at only with has_nodata != 0; an exact compare, of the byte for a uint8 scene,
 * where nodata must be an integer in 0 .. 255, of the float for a float32 one) and, in a float32 scene, it is finite: NaN and
 * +-inf are never valid, so a NaN `nodata` means "the non-finite pixels only". All three validate before they launch; the
 * scene and the plane are read at any alignment. */
/* counts [n] int32 <- the number of valid pixels of each T x T tile of the table `origins` (T a multiple of 16, at most 32768).
 * One work-group per tile, one plain store per tile, no atomics; an entry that is not inside the scene counts 0. 1 launch. */
int insar_scene_census(const void* scene, int32_t dtype /*INSAR_SCENE_**/, int32_t H, int32_t W, const uint8_t* valid /*nullable*/,
                       int32_t has_nodata, float nodata, const int32_t* origins, int32_t n, int32_t T, int32_t* counts /*[n]*/,
                       void* stream);
/* insar_scene_gather with the invalid pixels replaced: out [n][1][T][T] fp32 (16-byte aligned). A valid pixel of a uint8
 * scene gets insar_scene_gather's transform (has_norm must be 0), one of a float32 scene x = (v - offset) * scale with
 * has_norm != 0 (a subtraction, then a multiplication, in fp32: two roundings; offset finite, scale finite and not 0), else v.
 * An invalid pixel gives `fill` (finite), whatever its value: no arithmetic is done on it. With valid = null, has_nodata = 0
 * and has_norm = 0 the output equals insar_scene_gather's bit for bit on a scene of finite values. 1 launch. */
int insar_scene_gather_valid(const void* scene, int32_t dtype, int32_t H, int32_t W, const uint8_t* valid /*nullable*/,
                             int32_t has_nodata, float nodata, float fill, int32_t has_norm, float offset, float scale,
                             const int32_t* origins, int32_t n, int32_t T, float* out /*[n][1][T][T]*/, void* stream);
/* insar_scene_finalize with a per-pixel mask: at a pixel that is valid (the rule above, evaluated again from `scene` and
 * `valid`) and covered (wsum > 0) prob, mask and conf are insar_scene_finalize's, bit for bit, and valid_out [H][W] uint8 is 1;
 * at every other pixel prob = 0, mask = 0, conf = 0 and valid_out = 0, by a select: a NaN in acc does not get through and
 * nothing is divided by a wsum of 0. 1 launch. */
int insar_scene_finalize_valid(const float* acc, const float* wsum, int32_t K, int32_t H, int32_t W, const void* scene,
                               int32_t dtype, const uint8_t* valid /*nullable*/, int32_t has_nodata, float nodata,
                               float* prob /*nullable*/, uint8_t* mask, float* conf, uint8_t* valid_out, void* stream);

/* ---- regions of a class map (build-side addition; the reference has no post-processing): csrc/regions.hip --------------
 * Connected regions of a class map `mask` uint8 [H][W] (row-major, H * W < 2^31, no tile-multiple requirement). A pixel is
 * foreground if mask != 0 and, when `conf` fp32 [H][W] is given, conf >= min_conf; two foreground pixels are connected if
 * they are 4- / 8-neighbours (connectivity 4 | 8) AND carry the same class. A region's root is its smallest row-major pixel
 * index; regions of area >= min_area are kept and numbered 1..N in ascending root order (scipy.ndimage.label's numbering).
 * One call per phase, in this order on one stream; seven launches in all, whatever the mask holds; no work-group waits on
 * another. Every argument is checked before the device is touched (null pointers, H * W, connectivity, max_regions,
 * alignment).
 *   scratch: insar_regions_scratch_bytes(...) bytes, 16-byte aligned: int32 parent [H*W], int32 area / id [H*W], block counts.
 *            Nothing in it has to survive between calls or be cleared by the caller.
 *   table:   InsarRegion [1 + max_regions], 16-byte aligned. Record 0 is the header: its `area` is N, the TRUE number of kept
 *            regions, which may exceed max_regions; records 1..min(N, max_regions) are the regions. The kernels never write
 *            past record max_regions. All statistics are integers (no float atomics): bitwise reproducible. */
typedef struct InsarRegion {
  int64_t area;            /* pixels (header record: N) */
  int64_t sum_y, sum_x;    /* centroid = sum / area */
  int64_t sum_conf;        /* sum of llrint(clamp(conf, 0, 1) * 2^30); 0 without conf */
  int32_t y0, x0, y1, x1;  /* half-open bounding box */
  int32_t root;            /* smallest row-major pixel index */
  int32_t cls;             /* class value */
  int32_t _pad[2];
} InsarRegion;
/* host only: bytes of scratch for an H x W scene and of a table of max_regions regions */
int insar_regions_scratch_bytes(int32_t H, int32_t W, int32_t max_regions, int64_t* scratch_bytes, int64_t* table_bytes);
/* 1 launch: every 32 x 64 tile labelled in LDS; parent[i] = global index of the smallest pixel of i's component WITHIN its
 * tile, -1 for background; area cleared. conf nullable (then min_conf is ignored). */
int insar_regions_tiles(const uint8_t* mask, const float* conf /*nullable*/, float min_conf, int32_t H, int32_t W,
                        int32_t connectivity, void* scratch, void* stream);
/* 1 launch: unions across tile borders only; every access to parent is an agent-scope atomic. */
int insar_regions_merge(const uint8_t* mask, int32_t H, int32_t W, int32_t connectivity, void* scratch, void* stream);
/* 1 launch: parent[i] = root of i; area[root] = pixels of the region. */
int insar_regions_flatten(int32_t H, int32_t W, void* scratch, void* stream);
/* 3 launches (per-block counts of kept roots + table cleared; one-work-group scan, N to the header; per-block offsets):
 * area[root] becomes the region's id (0: dropped); records 1..min(N, max_regions) get root and cls. min_area >= 1. */
int insar_regions_number(const uint8_t* mask, int32_t H, int32_t W, int64_t min_area, int32_t max_regions, void* scratch,
                         void* table, void* stream);
/* 1 launch: labels int32 [H][W] (0: background or dropped), mask_out = mask where labels != 0 else 0, statistics added
 * into the table. conf nullable (sum_conf stays 0). */
int insar_regions_relabel(const uint8_t* mask, const float* conf /*nullable*/, int32_t H, int32_t W, int32_t max_regions,
                          void* scratch, void* table, int32_t* labels, uint8_t* mask_out, void* stream);

/* ---- splitting touching sites (build-side addition; the reference has no post-processing): csrc/split.hip ------------------
 * A watershed of a height map inside every label of a label map. labels int32 [H][W] (row-major, H * W < 2^31): a value <= 0 is
 * background, every other value a region; height int32 [H][W], >= 0 on the foreground (a negative one is counted in the
 * header and the result is then meaningless). key(p) = (height[p], -index(p)). Every foreground pixel points to the
 * greatest-key pixel among itself and its 8 neighbours of the same label; the pixels that point to themselves are the roots of
 * the basins; saddle(a, b) of two basins of one label is the maximum of min(height[p], height[q]) over 8-adjacent p in a, q in
 * b. Pieces start as the basins and merge in synchronous rounds: every piece u finds the neighbouring piece v with the greatest
 * (saddle(u, v), key(root v)) and merges into it iff depth(height[root u], saddle) <= threshold and key(root v) > key(root u),
 * where depth(P, S) = isqrt(256 P) - isqrt(256 S) (sixteenths of a pixel between two squared distances) with `squared`, else
 * P - S. Pieces are numbered 1..M by ascending smallest row-major pixel index. Integers only: bitwise reproducible.
 * One call per phase, in this order on one stream; no work-group waits on another. Every argument is checked before the
 * device is touched.
 *   scratch: insar_split_scratch_bytes(...) bytes, 16-byte aligned: int32 basin / piece [H*W], up [H*W], next / id [H*W],
 *            best index / first pixel [H*W], uint64 best word [H*W], block counts, the control words, the saddle table
 *            (2^k >= 2 max_pairs slots of 16 bytes) and the edge list (max_pairs x 16 bytes). Nothing in it has to survive
 *            between calls or be cleared by the caller. The control words are int32 [8 + max_rounds] at `ctrl_offset`:
 *            0 the TRUE number of basin pairs (may exceed max_pairs), 1 non-zero iff the saddle table overflowed, 2 the number
 *            of negative heights on the foreground, 3 the number of basins, 4 M (after finish), 8 + r the merges that round
 *            r decided (an upper bound: zero iff the round merged nothing).
 *   table:   InsarSplitRegion [1 + max_regions], 16-byte aligned. Record 0 is the header: area = M, the TRUE number of pieces,
 *            which may exceed max_regions; sum_y / sum_x / sum_conf = control words 0 / 1 / 2; y0 = control word 3. Records
 *            1..min(M, max_regions) are the pieces; the kernels never write past record max_regions. */
typedef struct InsarSplitRegion {
  int64_t area;            /* pixels (header record: M) */
  int64_t sum_y, sum_x;    /* centroid = sum / area */
  int64_t sum_conf;        /* sum of llrint(clamp(conf, 0, 1) * 2^30); 0 without conf */
  int32_t y0, x0, y1, x1;  /* half-open bounding box */
  int32_t first;           /* smallest row-major pixel index */
  int32_t cls;             /* mask[first]; 0 without mask */
  int32_t parent;          /* labels[first]: the region the piece was cut from */
  int32_t peak;            /* height at the piece's root */
  int32_t peak_index;      /* row-major index of the root */
  int32_t saddle;          /* greatest saddle towards a neighbouring piece; -1 if there is none */
  int32_t _pad[2];
} InsarSplitRegion;
/* host only: bytes of scratch and of a table, and where the control words lie in the scratch. 1 <= max_pairs <= 2^24,
 * 1 <= max_rounds <= 4096, max_regions >= 1. */
int insar_split_scratch_bytes(int32_t H, int32_t W, int32_t max_regions, int64_t max_pairs, int32_t max_rounds,
                              int64_t* scratch_bytes, int64_t* table_bytes, int64_t* ctrl_offset, int64_t* ctrl_bytes);
/* 5 launches: clear, ascent, resolve (basin of every pixel), saddles (pair table; piece state of every basin), compact (edge
 * list; control words 0..3 are final afterwards). */
int insar_split_basins(const int32_t* labels, const int32_t* height, int32_t H, int32_t W, int64_t max_pairs, int32_t max_rounds,
                       void* scratch, void* stream);
/* 4 launches per round (best saddle, tie on the root index, decide, compress), over the edge list only: rounds first_round ..
 * first_round + n_rounds - 1 <= max_rounds - 1. A round after the fixed point changes nothing. 0 <= threshold <= 2^20. */
int insar_split_rounds(const int32_t* height, int32_t H, int32_t W, int32_t squared, int32_t threshold, int32_t first_round,
                       int32_t n_rounds, int64_t max_pairs, int32_t max_rounds, void* scratch, void* stream);
/* 6 launches: remaining saddles, piece and first pixel of every pixel, count / scan / number, relabel: labels_out int32 [H][W]
 * (0 or the piece id) and the table. mask uint8 [H][W] and conf fp32 [H][W] nullable. */
int insar_split_finish(const int32_t* labels, const int32_t* height, const uint8_t* mask /*nullable*/, const float* conf /*nullable*/,
                       int32_t H, int32_t W, int32_t max_regions, int64_t max_pairs, int32_t max_rounds, void* scratch, void* table,
                       int32_t* labels_out, void* stream);

/* ---- sieving class maps (build-side addition; the reference has no post-processing): csrc/sieve.hip ------------------------
 * Regions of a class map below a per-class area threshold are absorbed by their largest neighbour, whatever its class. The
 * input regions are the connected components over ALL classes: the caller runs the insar_regions_* phases (min_area 1, no
 * conf) on the remapped map that insar_sieve_remap leaves at offset 0 of the scratch, which gives the label map (ids 1..N by
 * ascending smallest pixel index; void pixels 0) and the InsarRegion table (area, root).
 *   adjacency: every horizontally or vertically adjacent pixel pair whose labels a != b are both in 1..max_label counts once
 *              under (min(a, b), max(a, b)): the number of pixel edges two regions share. Always 4-adjacency.
 *   rounds:    pieces start as the regions; id, class = those of the root region, area = the sum over the members,
 *              key(u) = (area[u], -id[u]). Per synchronous round every piece u with area[u] < thresholds[cls[u]] and a
 *              neighbouring piece takes best(u), the neighbouring piece with the greatest key, and merges into it unless
 *              best(best(u)) == u and key(u) > key(best(u)); pointers are compressed, areas added into the roots.
 *   output:    out[p] = cls[root[label[p]]] for labelled pixels, mask[p] elsewhere.
 * Integers only: bitwise reproducible. One call per phase on one stream; no work-group waits on another. Every argument is
 * checked before the device is touched. 1 <= max_regions <= 2^30, 1 <= max_pairs <= 2^24, 1 <= max_rounds <= 4096.
 *   scratch: insar_sieve_scratch_bytes(...) bytes, 16-byte aligned: the remapped map uint8 [H*W] at offset 0, the control
 *            words, int32 root / next / area / class [1 + max_regions] (the roots directly behind the control words), uint64
 *            best word [1 + max_regions], the pair list (a 16-byte header {int32 n_pairs, overflow, 0, 0} at `pairs_offset`,
 *            then max_pairs records {int32 a, int32 b, int64 edges}) and the pair table (2^k >= 2 max_pairs slots of 16
 *            bytes). Nothing in it has to survive between calls or be cleared by the caller. n_pairs is the TRUE number of
 *            pairs, which may exceed max_pairs; overflow is non-zero iff the pair table overflowed. The control words are
 *            int32 [8 + max_rounds] at `ctrl_offset`: 0 / 1 the header's n_pairs / overflow and 2 the TRUE number of regions
 *            N (after the first rounds call), 3 pixels of class 255 where there is no void value (they have no code left in the
 *            remapped map; the result is then meaningless), 4 changed pixels and 5 absorbed regions (after apply), 8 + r
 *            the merges of round r. */
/* host only: bytes of the scratch and where the control words and the pair list lie in it. */
int insar_sieve_scratch_bytes(int32_t H, int32_t W, int32_t max_regions, int64_t max_pairs, int32_t max_rounds,
                              int64_t* scratch_bytes, int64_t* ctrl_offset, int64_t* ctrl_bytes, int64_t* pairs_offset);
/* 1 launch (2 with void_value -1): the remapped map (class c -> c + 1 below void_value or without one, c above it, void -> 0)
 * and zeroed control words. mask uint8 [H][W]; void_value -1 (none) or 0..255. */
int insar_sieve_remap(const uint8_t* mask, int32_t H, int32_t W, int32_t void_value, int32_t max_regions, int64_t max_pairs,
                      int32_t max_rounds, void* scratch, void* stream);
/* 3 launches: clear, pairs (the adjacency table of labels int32 [H][W]; labels <= 0 or > max_label are no region), compact
 * (the pair list and its header). Stands alone: it needs nothing of the other phases. */
int insar_sieve_pairs(const int32_t* labels, int32_t H, int32_t W, int32_t max_label, int32_t max_regions, int64_t max_pairs,
                      int32_t max_rounds, void* scratch, void* stream);
/* 3 launches per round (best neighbour, decide, compress), over the pair list and the region table only, plus 1 (the piece
 * state of every region from `table`, an InsarRegion table, and the classes mask[root]) when first_round is 0: rounds
 * first_round .. first_round + n_rounds - 1 <= max_rounds - 1. A round after the fixed point changes nothing. thresholds:
 * int32 [256] in device memory; 0: regions of that class are never absorbed. */
int insar_sieve_rounds(const void* table, const uint8_t* mask, const int32_t* thresholds, int32_t H, int32_t W, int32_t first_round,
                       int32_t n_rounds, int32_t max_regions, int64_t max_pairs, int32_t max_rounds, void* scratch, void* stream);
/* 1 launch: out uint8 [H][W], changed uint8 [H][W] (nullable; 1 where out != mask), control words 4 and 5. */
int insar_sieve_apply(const int32_t* labels, const uint8_t* mask, int32_t H, int32_t W, int32_t max_regions, int64_t max_pairs,
                      int32_t max_rounds, void* scratch, uint8_t* out, uint8_t* changed /*nullable*/, void* stream);

/* ---- hysteresis thresholds (build-side addition; the reference has no post-processing): csrc/hysteresis.hip ----------------
 * A site is a connected component of {score >= low} that holds at least min_seeds pixels with score >= high.
 *   candidates: score fp32 [planes][H][W] (row-major, H * W < 2^31), plane p belonging to class p + 1 (a background plane is
 *               not passed: it never takes part); thresholds fp32 [512] in device memory, low[c] at word c and high[c] at word
 *               256 + c, low[c] <= high[c] both finite, or low[c] = NaN for a class that is not selected. A pixel is a
 *               candidate of class c if score[c] >= low[c] in a float32 compare (NaN compares false) and its byte of `valid`
 *               (uint8 [H][W], nullable) is non-zero. Of several classes the greatest score wins, ties go to the smallest
 *               class. cand uint8 [H][W] is the class or 0, conf fp32 [H][W] the class's score, 0 where there is no candidate.
 *   regions:    the caller runs the five insar_regions_* phases on cand / conf with min_conf = -inf: the components of the
 *               candidate map of area >= min_area, numbered 1..N by ascending root, their InsarRegion table over the whole
 *               low-threshold extent, the label map and mask_out.
 *   seeds:      a labelled pixel is a seed if conf >= high[cand]. Per label the number of seeds and the peak key
 *               (ordered_u32(conf) << 32) | (0xFFFFFFFF - index), where ordered_u32 flips all bits of a negative float32 and
 *               the sign bit of any other: its maximum is the exact maximum of conf at the first pixel, in row-major order,
 *               that reaches it.
 *   keep:       a region is kept if n_seed >= min_seeds; kept regions are renumbered 1..N' in the same order and copied, with
 *               their seed fields, into a second, compact table.
 *   apply:      labels = remap[labels]; mask = cand where the new label is not 0, else 0.
 * Integers only behind the compares (agent-scope integer atomics, no float atomics): bitwise reproducible. One call per phase
 * on one stream, 12 launches in all with the seven of the regions phases, whatever the map holds; no work-group waits on
 * another. Every argument is checked before the device is touched.
 *   scratch: insar_hyst_scratch_bytes(...) bytes, 16-byte aligned: the seed table {int64 n_seed, uint64 peak_key}
 *            [1 + max_regions], then remap int32 [1 + max_regions]. Nothing in it has to survive between calls or be cleared
 *            by the caller.
 *   table:   InsarHystRegion [1 + max_regions], 16-byte aligned, NOT the InsarRegion table. Record 0 is the header: area = N',
 *            the number of kept regions, sum_y = N, the TRUE number of components of area >= min_area, which may exceed
 *            max_regions (the result is then meaningless); records 1..N' are the kept regions. */
typedef struct InsarHystRegion {
  int64_t area;            /* the fields of InsarRegion, over the whole low-threshold extent (header record: N') */
  int64_t sum_y, sum_x;    /* (header record: sum_y = N) */
  int64_t sum_conf;
  int32_t y0, x0, y1, x1;
  int32_t root;
  int32_t cls;
  int32_t _pad[2];
  int64_t n_seed;          /* pixels with conf >= high[cls] */
  uint64_t peak_key;       /* (ordered_u32(peak) << 32) | (0xFFFFFFFF - index of the first pixel that reaches the peak) */
} InsarHystRegion;
/* host only: bytes of the scratch (seed table and remap) and of the compact table for max_regions regions */
int insar_hyst_scratch_bytes(int32_t H, int32_t W, int32_t max_regions, int64_t* scratch_bytes, int64_t* table_bytes);
/* 1 launch: cand and conf from the score planes. 1 <= planes <= 255. 16-byte loads and stores wherever a quad lies inside the
 * map and its plane offset keeps the alignment; guarded scalars elsewhere. */
int insar_hyst_classify(const float* score, int32_t planes, int32_t H, int32_t W, const float* thresholds,
                        const uint8_t* valid /*nullable*/, uint8_t* cand, float* conf, void* stream);
/* 2 launches: the seed table cleared, then filled from labels (as insar_regions_relabel wrote them; ids above max_regions
 * are never an index), cand and conf. */
int insar_hyst_seeds(const int32_t* labels, const uint8_t* cand, const float* conf, const float* thresholds, int32_t H, int32_t W,
                     int32_t max_regions, void* scratch, void* stream);
/* 1 launch, one work-group: remap and the compact table from `regions` (the InsarRegion table) and the seed table.
 * min_seeds >= 1. */
int insar_hyst_keep(const void* regions, int64_t min_seeds, int32_t max_regions, void* scratch, void* table, void* stream);
/* 1 launch: labels renumbered in place, mask uint8 [H][W] written. */
int insar_hyst_apply(const uint8_t* cand, int32_t H, int32_t W, int32_t max_regions, const void* scratch, int32_t* labels,
                     uint8_t* mask, void* stream);

/* ---- region outlines (build-side addition; the reference has no post-processing): csrc/outline.hip ------------------------
 * The exact pixel-edge ("crack") outline of every region of a label map `labels` int32 [H][W] (row-major; 0 or an id >= 1, as
 * insar_regions_relabel writes it, but any int32 map is legal; H, W >= 1, H * W < 2^29), as ordered, closed rings of lattice
 * vertices. Vertex (y, x), 0 <= y <= H, 0 <= x <= W, is the top-left corner of pixel (y, x).
 *   edge:      side s (0 top, 1 right, 2 bottom, 3 left) of a pixel p = (y, x) with label L != 0 whose 4-neighbour across s
 *              carries another label or lies outside the scene; id 4 * (y * W + x) + s; directed with the region on its right:
 *              top east (y, x) -> (y, x+1), right south (y, x+1) -> (y+1, x+1), bottom west (y+1, x+1) -> (y+1, x), left north
 *              (y+1, x) -> (y, x). A crack between two non-zero labels belongs to both regions, once in each direction.
 *   successor: with A = p + d(s) the pixel ahead on the region side and B = A's neighbour across side s (outside the scene: 0),
 *              a = (A carries L), b = (B carries L): a && b: left, (B, (s+3)%4); a && !b: straight, (A, s); !a && !b: right,
 *              (p, (s+1)%4); !a && b (a saddle): left with connectivity 8, right with connectivity 4. A permutation of the edges.
 *   ring:      one cycle of the successor map; its leader is its smallest edge id; rings are numbered 0..R-1 in ascending leader
 *              order; an edge's rank is its distance from the leader along the successor. area2 = sum over the ring of
 *              x_i * y_{i+1} - x_{i+1} * y_i of the edges' tail vertices: positive for exteriors, negative for holes.
 *   vertices:  int32 [max_vertices][2] as (y, x), 8-byte aligned, ring after ring: the tails of a ring's edges in rank order. With
 *              corners_only only the tails of edges whose side differs from their predecessor's are kept, in the same order.
 *   table:     InsarRing [1 + max_rings], 16-byte aligned. Record 0 is the header: label = R, count = V, edges = E, the TRUE
 *              numbers of rings, vertices written and boundary edges, which may exceed the capacities; record 1 + r is ring r.
 *   scratch:   insar_outline_scratch_bytes(...) bytes, 16-byte aligned; nothing in it has to survive between calls or be cleared.
 * Call edges, lead, rank, rings, write in this order on one stream, with the same H, W and max_edges; read E from the header
 * after `edges` and pass it on as n_edges (lead .. write refuse n_edges > max_edges). 12 + 2 ceil(log2 E) launches in all, a
 * function of E alone; one launch per step, no work-group waits on another, integers only (bitwise reproducible). No kernel
 * writes an edge slot >= max_edges, a record > max_rings or a vertex >= max_vertices. Every argument is checked before the
 * device is touched (null pointers, H * W, connectivity, capacities, alignment). */
typedef struct InsarRing {
  int64_t area2;           /* signed doubled area */
  int32_t label, leader;   /* the region's label; the ring's smallest edge id (header record: label = R) */
  int32_t start, count;    /* first vertex and number of vertices in the vertex array (header: count = V) */
  int32_t edges;           /* crack length of the ring before corner compaction (header: E) */
  int32_t y0, x0, y1, x1;  /* half-open vertex box: y0 <= y < y1, x0 <= x < x1 over the ring's vertices */
  int32_t _pad;
} InsarRing;
/* host only: bytes of scratch for an H x W scene with max_edges edge slots, and of a table of max_rings rings */
int insar_outline_scratch_bytes(int32_t H, int32_t W, int32_t max_rings, int32_t max_edges, int64_t* scratch_bytes,
                                int64_t* table_bytes);
/* host only: the launches of the five calls below for n_edges boundary edges: 12 + 2 ceil(log2 n_edges) (n_edges < 1: 6) */
int insar_outline_launches(int32_t n_edges);
/* 4 launches (side masks and block counts; one-work-group scan, E to the header, the rest of it cleared; per-pixel offsets;
 * successor, id and turn flag of every edge below max_edges). 1 <= max_edges <= 2^30. */
int insar_outline_edges(const int32_t* labels, int32_t H, int32_t W, int32_t connectivity, int32_t max_edges, void* scratch,
                        void* table, void* stream);
/* ceil(log2 n_edges) launches: pointer doubling with a running minimum; every edge learns its ring's leader. */
int insar_outline_lead(int32_t H, int32_t W, int32_t n_edges, int32_t max_edges, void* scratch, void* stream);
/* 1 + ceil(log2 n_edges) launches: every ring cut in front of its leader, then Wyllie list ranking. */
int insar_outline_rank(int32_t H, int32_t W, int32_t n_edges, int32_t max_edges, void* scratch, void* stream);
/* 3 launches (leaders and ring lengths per block; one-work-group scan, R to the header; ring numbers, records initialised) */
int insar_outline_rings(const int32_t* labels, int32_t H, int32_t W, int32_t n_edges, int32_t max_rings, int32_t max_edges,
                        void* scratch, void* table, void* stream);
/* 4 launches (tails scattered into ring order; area2, box and vertex count per ring; one-work-group scan, V to the header; the
 * kept vertices and every ring's start written) */
int insar_outline_write(int32_t H, int32_t W, int32_t n_edges, int32_t corners_only, int32_t max_rings, int32_t max_vertices,
                        int32_t max_edges, void* scratch, void* table, int32_t* vertices, void* stream);

/* ---- contour lines (build-side addition; the reference has no post-processing): csrc/contour.hip ---------------------------
 * The iso-lines of a raster [H][W] (row-major; float32, uint8 or int32, INSAR_ZONAL_*; 1 <= H, W <= 2^22) at n_levels levels
 * (1 .. 32, n_levels * H * W < 2^30) as ordered polylines of sub-pixel vertices: marching squares in exact integers.
 *   q:         per pixel, by the rule of insar_zonal_accumulate: integer rasters q = v, float32 q = rint(clamp((double)v * scale,
 *              +-(2^31 - 1))) to nearest even. A pixel that is not finite, equals `nodata` in the raster's own type (has_nodata) or
 *              has valid[p] == 0 (valid: uint8 [H][W], nullable) is INVALID. levels_q: HOST int32 [n_levels], strictly increasing.
 *   node:      the centre of pixel (y, x), at (y + 1/2, x + 1/2) in the frame of the region outlines; every coordinate is an int32
 *              in 1/256 pixel: (256 y + 128, 256 x + 128). A node is ABOVE level l iff q >= levels_q[l].
 *   crossing:  lattice edge o = 0 joins node p = y * W + x to its right neighbour, o = 1 to the node below. It is crossed at l iff
 *              both ends are valid and exactly one is above, and it is a crossing iff one of the two cells (2 x 2 nodes) it bounds
 *              has four valid nodes (otherwise no segment ends on it and it is not counted). id (l * H * W + p) * 2 + o. Position,
 *              from the below end: s = floor(((q_l - q_below) * 512 + d) / (2 d)), d = q_above - q_below, in int64, clamped to
 *              1 .. 255; the offset from p is s if p is the below end, else 256 - s. No vertex lies on a node.
 *   segments:  a cell with four valid nodes emits the marching-squares segments of its above-mask, directed with the above side on
 *              the right (the handedness of the region outlines: the ring round a peak has positive area2); the saddle masks join
 *              the above corners iff the four q sum to >= 4 q_l in int64. A crossing starts at most one segment and ends at most one.
 *   lines:     the components: closed rings (leader = smallest crossing id) and open lines (leader = the head, the crossing no
 *              segment ends on; they end on the raster border or beside a cell with an invalid node). Lines are numbered in
 *              ascending leader order, so level by level; vertices are ranked from the leader; every crossing is kept (V = E).
 *   vertices:  int32 [n_crossings][2] as (Y, X), 8-byte aligned, line after line.
 *   table:     InsarContourLine [4 + max_lines], 16-byte aligned. Records 0 .. 3 are the header, 48 int32 slots: slot 2 = the
 *              TRUE number of lines (it may exceed max_lines), 3 = E, 5 = V, 16 + l = the crossings of level l; record 4 + r is line r.
 *   scratch:   insar_contour_scratch_bytes(...) bytes, 16-byte aligned; nothing in it has to survive between calls or be cleared.
 * Call edges, lead, rank, lines, write in this order on one stream with the same H, W, n_levels and max_vertices; read E from the
 * header after `edges` and pass it on as n_crossings (lead .. write refuse n_crossings > max_vertices). 11 + 2 ceil(log2 E)
 * launches in all, a function of E alone; one launch per step, no work-group waits on another, integers only behind the
 * quantisation (bitwise reproducible). No kernel writes a crossing slot >= max_vertices or a record > max_lines. Every argument
 * is checked before the device is touched. */
typedef struct InsarContourLine {
  int64_t area2;           /* rings: signed doubled area in 1/256^2 pixel, sum of X_i * Y_{i+1} - X_{i+1} * Y_i; open lines: 0 */
  int32_t level, leader;   /* level index; the leader's crossing id */
  int32_t start, count;    /* first vertex and number of vertices in the vertex array */
  int32_t closed;          /* 1 ring, 0 open line */
  int32_t y0, x0, y1, x1;  /* half-open box in 1/256 pixel: y0 <= Y < y1, x0 <= X < x1 over the line's vertices */
  int32_t _pad;
} InsarContourLine;
/* host only: bytes of scratch for an H x W raster at n_levels levels with max_vertices crossing slots, and of a table of max_lines */
int insar_contour_scratch_bytes(int32_t H, int32_t W, int32_t n_levels, int32_t max_lines, int32_t max_vertices,
                                int64_t* scratch_bytes, int64_t* table_bytes);
/* host only: the launches of the five calls below for n_crossings crossings: 11 + 2 ceil(log2 n_crossings) (n_crossings < 1: 5) */
int insar_contour_launches(int32_t n_crossings);
/* 5 launches (q and valid flag per pixel; crossing masks and counts per level and block; one-work-group scan, the header written;
 * compact index per mask word; vertex, id, successor and head flag of every crossing below max_vertices). */
int insar_contour_edges(const void* raster, int32_t elem_type, int32_t H, int32_t W, double scale, int32_t has_nodata, double nodata,
                        const uint8_t* valid, const int32_t* levels_q, int32_t n_levels, int32_t max_vertices, void* scratch,
                        void* table, void* stream);
/* ceil(log2 n_crossings) launches: pointer doubling with a running minimum; tails point at themselves. */
int insar_contour_lead(int32_t H, int32_t W, int32_t n_levels, int32_t n_crossings, int32_t max_vertices, void* scratch, void* stream);
/* 1 + ceil(log2 n_crossings) launches: rings cut in front of their leader, heads written at their tails' slots; Wyllie ranking. */
int insar_contour_rank(int32_t H, int32_t W, int32_t n_levels, int32_t n_crossings, int32_t max_vertices, void* scratch, void* stream);
/* 3 launches (leaders and line lengths per block; one-work-group scan, the line count to the header; numbers, records initialised) */
int insar_contour_lines(int32_t H, int32_t W, int32_t n_levels, int32_t n_crossings, int32_t max_lines, int32_t max_vertices,
                        void* scratch, void* table, void* stream);
/* 2 launches (vertices scattered into line order; area2 and box per line). vertices: n_crossings slots. */
int insar_contour_write(int32_t H, int32_t W, int32_t n_levels, int32_t n_crossings, int32_t max_lines, int32_t max_vertices,
                        void* scratch, void* table, int32_t* vertices, void* stream);

/* ---- outline simplification (build-side addition; the reference has no post-processing): csrc/simplify.hip -------------------
 * Douglas-Peucker over the rings of the region outlines, in exact integers, with the common border of two regions simplified
 * to the same vertices from both sides. A POSITION is an index into the input vertex array; the kept set is a set of positions.
 *   input:     vertices int32 [n_vertices][2] as (y, x), ring after ring, 0 <= y, x <= 16384; `rings`: InsarRing [1 + n_rings]
 *              on the device (record 0 is a header and is not read; of a ring only start and count are read, the other fields
 *              are copied), the rings contiguous and in order: start[0] = 0, start[r + 1] = start[r] + count[r], the counts
 *              adding up to n_vertices; optionally the label map int32 [H][W], H, W <= 16384, the rings were traced from.
 *              Vertex (y, x) is the top-left corner of pixel (y, x); its four pixels are p00 = (y-1, x-1), p01 = (y-1, x),
 *              p10 = (y, x-1), p11 = (y, x), a pixel outside the map counting as 0.
 *   anchors:   only with `labels`: a position whose four pixels hold three or more distinct values, or form a two-label saddle
 *              (p00 == p11, p01 == p10, p00 != p01, both non-zero). Anchors are always kept and split a ring into arcs along
 *              which the pair (own label, label across) is constant: both rings that border an arc see the same vertices
 *              between the same end points, in opposite order. This needs every lattice vertex in both rings (a T-junction
 *              on a straight side is a corner of one ring only): with `labels` the caller passes rings traced with
 *              corners_only = 0 (count == edges). Without `labels` there are no anchors and every ring stands alone.
 *   seeds:     a ring with no anchor position, or exactly one, is a closed arc. Seed 1 is the anchor's coordinates, else the
 *              lexicographically smallest (y, x) of the ring; seed 2 is the coordinates with the largest squared distance from
 *              seed 1, ties to the smallest (y, x). EVERY position of the ring that carries the coordinates of a seed is kept (a
 *              ring may pass a saddle twice). Neither seed depends on the ring's direction or start vertex.
 *   round:     a segment (a, b) is a pair of cyclically consecutive kept positions of a ring. Among the positions strictly
 *              between them the winner has the largest cross^2, cross = (b - a) x (p - a) as an integer, ties to the smallest
 *              (y, x) - never to the smallest index, so both directions agree; every position of the segment that equals the
 *              winner in both is a winner. Winners are kept iff 256 cross^2 > eps2q |b - a|^2, with eps2q = q^2 and q the
 *              tolerance in 1/16 pixel (0 <= q <= 16384), compared exactly: for integers this is cross^2 > floor(eps2q
 *              |b - a|^2 / 256), and cross^2 < 2^60, eps2q |b - a|^2 < 2^58 fit 64 bits. Where a and b carry the same
 *              coordinates (an arc that returns to its anchor) the distance from that point stands for the distance from the
 *              line: |p - a|^2 takes the place of cross^2 and 1 that of |b - a|^2. Round r is recursion level r of the
 *              sequential algorithm; all segments of all rings take part in every round. With eps2q = 0 exactly the vertices
 *              off their chord survive: collinear vertices are dropped.
 *   rounds:    rounds 0 .. max_rounds - 1 keep their winners (1 <= max_rounds <= 4095); round max_rounds is a probe that only
 *              counts them. A round whose predecessor kept nothing returns at once, so later rounds are no-ops. `rounds` is
 *              the number of rounds that kept a vertex; `converged` says that the probe found nothing to keep (or was not
 *              needed): otherwise the result is the sequential result truncated at depth max_rounds.
 *   output:    out_vertices int32 [n_vertices][2], out_kept int32 [n_vertices]: the kept vertices and their positions, in
 *              input order, compacted (the first `count` of the header are written). table: InsarRing [1 + n_rings], 16-byte
 *              aligned. Record 0: label = n_rings, count = kept vertices, edges = n_vertices, leader = rounds, start =
 *              converged. Record 1 + r: label, leader and edges of the input ring; start and count in the compacted array;
 *              area2 the exact shoelace sum and y0 .. x1 the half-open box of the kept vertices; _pad = 1 where the ring
 *              collapsed (fewer than 3 kept vertices, or area2 == 0), else 0.
 *   scratch:   insar_simplify_scratch_bytes(...) bytes, 16-byte aligned; setup clears what it needs. Its first 4096 int32
 *              are the per-round counters of kept vertices (slot max_rounds: the probe): a host that reads the counter of the
 *              last round it launched and finds 0 may stop launching rounds.
 * Guaranteed: every dropped vertex lies within the tolerance of the chord of the segment it ended in; the kept set of a larger
 * tolerance is a subset of that of a smaller one when both converged; a shared arc comes out identical from both sides. NOT
 * guaranteed: that two different arcs never cross at a large tolerance (Douglas-Peucker does not, and nothing is added).
 * Call setup, rounds (once, or in batches of consecutive rounds), finish in this order on one stream with the same counts and
 * capacities. 4 + 4 per round + 6 launches; no work-group waits on another, integer atomics only, nothing depends on launch
 * geometry. Every argument is checked before the device is touched (null pointers, counts against capacities, alignment,
 * H, W, eps2q, the round numbers); the ring table itself lives on the device and is the caller's promise, and no kernel
 * leaves its buffers whatever the table holds. */
/* host only: bytes of scratch and of the output table for these capacities (1 <= max_vertices <= 2^28, 1 <= max_rings <= 2^26) */
int insar_simplify_scratch_bytes(int32_t max_vertices, int32_t max_rings, int64_t* scratch_bytes, int64_t* table_bytes);
/* host only: the launches of setup, `rounds` rounds (the probe counts as one) and finish: 10 + 4 rounds */
int insar_simplify_launches(int32_t rounds);
/* 4 launches (clear; ring of every vertex, anchors, smallest key per ring; farthest vertex per ring; seeds kept). labels is
 * nullable; H and W are checked only with labels. */
int insar_simplify_setup(const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings,
                         const int32_t* labels /*nullable*/, int32_t H, int32_t W, int32_t max_vertices, int32_t max_rings,
                         void* scratch, void* stream);
/* 4 launches per round (carries of the kept positions over the blocks; cross^2 and the segment maximum; ties; winners kept) for
 * the rounds first_round .. first_round + n_rounds - 1, all within 0 .. max_rounds; round max_rounds is the probe. */
int insar_simplify_rounds(const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings, int64_t eps2q,
                          int32_t first_round, int32_t n_rounds, int32_t max_rounds, int32_t max_vertices, int32_t max_rings,
                          void* scratch, void* stream);
/* 6 launches (kept per block; one-work-group scan and the header; scatter; ring records; area2 and boxes; collapsed flags) */
int insar_simplify_finish(const int32_t* vertices, int32_t n_vertices, const void* rings, int32_t n_rings, int32_t max_rounds,
                          int32_t max_vertices, int32_t max_rings, void* scratch, void* table, int32_t* out_vertices,
                          int32_t* out_kept, void* stream);

/* ---- contour simplification (build-side addition; the reference has no post-processing): csrc/contour_simplify.hip ----------
 * Douglas-Peucker over the polylines of the contour lines, open lines and closed rings, in exact integers. A POSITION is an
 * index into the input vertex array; the kept set is a set of positions; every line is simplified on its own.
 *   input:     vertices int32 [n_vertices][2] as (Y, X) in 1/256 pixel, line after line, 0 <= Y, X <= 2^30 (the caller's
 *              promise: every bound below rests on it, and no kernel leaves its buffers if it is broken); `lines`:
 *              InsarContourLine [1 + n_lines] on the device (record 0 is a header and is not read; of a line start, count and
 *              closed are read, level and leader are copied), the lines contiguous and in order: start[0] = 0, start[r + 1] =
 *              start[r] + count[r], the counts adding up to n_vertices; an open line has 2 vertices or more, a ring 3 or more.
 *   tolerance: eps = the tolerance in 1/256 pixel (0 <= eps <= 262144 = 1024 pixels), eps2 = eps^2 <= 2^36.
 *   seeds:     an open line keeps its first and its last position. A ring keeps two: seed 1 is the position with the
 *              lexicographically smallest (Y, X), seed 2 the position with the largest squared distance from it, ties to the
 *              smallest (Y, X); both break a tie of equal coordinates by the smallest position (the contour lines never repeat a
 *              coordinate within a line; the rule makes the function total on other input). A ring whose vertices all coincide
 *              has one seed.
 *   round:     a segment (a, b) is a pair of consecutive kept positions of a line, cyclically in a ring (a ring with two seeds
 *              has two segments, one with one seed has the segment (a, a) of every other position). Among the positions strictly
 *              between them the winner has the largest |cross|, cross = (b - a) x (p - a) in int64, ties to the smallest
 *              (Y, X), then to the smallest position: one winner per segment. It is kept iff cross^2 > eps2 |b - a|^2, compared
 *              exactly. Where a and b carry the same coordinates, d^2 = |p - a|^2 takes the place of |cross| and the test is
 *              d^2 > eps2. Round r is recursion level r of the sequential algorithm; all segments of all lines take part in
 *              every round. With eps2 = 0 exactly the vertices off their chord survive: collinear vertices are dropped.
 *   bounds:    differences within +-2^30, products within 2^60, |cross| <= 2^60 and d^2 <= 2^61 in 64 bits; cross^2 <= 2^120
 *              against eps2 |b - a|^2 <= 2^97 as unsigned 128-bit integers.
 *   rounds:    as in the outline simplification: rounds 0 .. max_rounds - 1 keep their winners (1 <= max_rounds <= 4095), round
 *              max_rounds is a probe that only counts them, a round whose predecessor kept nothing returns at once. `rounds` is
 *              the number of rounds that kept a vertex; `converged` says that the probe found nothing to keep: otherwise the
 *              result is the sequential result truncated at depth max_rounds.
 *   output:    out_vertices int32 [n_vertices][2], out_kept int32 [n_vertices]: the kept vertices and their positions, in
 *              input order, compacted (the first `count` of the header are written). table: InsarContourLine [1 + n_lines],
 *              16-byte aligned. Record 0: level = n_lines, leader = rounds, start = converged, count = kept vertices, closed =
 *              n_vertices. Record 1 + r: level and leader of the input line, closed as 0 / 1; start and count in the compacted
 *              array; area2 the shoelace sum of the kept vertices of a ring (added modulo 2^64: exact wherever it fits an int64,
 *              as for every ring that does not overlap itself), 0 for an open line; y0 .. x1 the half-open box of the kept
 *              vertices; _pad = 1 where a ring collapsed (fewer than 3 kept vertices, or area2 == 0), 0 for every open line.
 *   scratch:   insar_contour_simplify_scratch_bytes(...) bytes, 16-byte aligned; setup clears what it needs. Its first 4096
 *              int32 are the per-round counters of kept vertices (slot max_rounds: the probe): a host that reads the counter of
 *              the last round it launched and finds 0 may stop launching rounds.
 * Guaranteed: every dropped vertex lies within the tolerance of the chord of the segment it ended in; the ends of an open line
 * stay; the kept set of a larger tolerance is a subset of that of a smaller one when both converged. NOT guaranteed: that two
 * lines, of different levels or of one, never cross at a large tolerance, nor that a hole stays inside its exterior.
 * Call setup, rounds (once, or in batches of consecutive rounds), finish in this order on one stream with the same counts and
 * capacities. 6 + 5 per round + 6 launches; no work-group waits on another, integer atomics only, nothing depends on launch
 * geometry. Every argument is checked before the device is touched (null pointers, counts against capacities, alignment, eps2,
 * the round numbers); the line table itself lives on the device and is the caller's promise, and no kernel leaves its buffers
 * whatever the table holds. */
/* host only: bytes of scratch and of the output table for these capacities (1 <= max_vertices <= 2^28, 1 <= max_lines <= 2^27) */
int insar_contour_simplify_scratch_bytes(int32_t max_vertices, int32_t max_lines, int64_t* scratch_bytes, int64_t* table_bytes);
/* host only: the launches of setup, `rounds` rounds (the probe counts as one) and finish: 12 + 5 rounds */
int insar_contour_simplify_launches(int32_t rounds);
/* 6 launches (clear; line of every vertex, open ends kept, smallest key per ring; largest distance and seed 1; its smallest key;
 * its smallest position; seeds kept). */
int insar_contour_simplify_setup(const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines,
                                 int32_t max_vertices, int32_t max_lines, void* scratch, void* stream);
/* 5 launches per round (carries of the kept positions over the blocks; |cross| and the segment maximum; ties by key; ties by
 * position; winners kept) for the rounds first_round .. first_round + n_rounds - 1, all within 0 .. max_rounds; round
 * max_rounds is the probe. */
int insar_contour_simplify_rounds(const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines, int64_t eps2,
                                  int32_t first_round, int32_t n_rounds, int32_t max_rounds, int32_t max_vertices,
                                  int32_t max_lines, void* scratch, void* stream);
/* 6 launches (kept per block; one-work-group scan and the header; scatter; line records; area2 and boxes; collapsed flags) */
int insar_contour_simplify_finish(const int32_t* vertices, int32_t n_vertices, const void* lines, int32_t n_lines,
                                  int32_t max_rounds, int32_t max_vertices, int32_t max_lines, void* scratch, void* table,
                                  int32_t* out_vertices, int32_t* out_kept, void* stream);

/* ---- polygon rasterisation (build-side addition; the reference reads ready-made masks): csrc/raster.hip ---------------------
 * The inverse of the region outlines: an edge table becomes a label map `out` [H][W] (row-major; uint8 with INSAR_RASTER_U8,
 * int32 with INSAR_RASTER_I32; H >= 1, 1 <= W <= 16384, H * W < 2^31) in exact integers, no floating point on the device.
 *   fixed point: coordinates are int32 in units of 1/256 pixel, X = 256 x, Y = 256 y; (0, 0) is the top-left corner of pixel
 *              (0, 0), the lattice of the region outlines; the centre of pixel (r, c) is (Y, X) = (256 r + 128, 256 c + 128).
 *              Every coordinate lies within +-2^24 (the caller's promise: every product below then fits int64; coordinates
 *              beyond it give an unspecified map, never an access outside the buffers). Vertices outside the scene are legal.
 *   edges:     int32 [n_edges][5] = (X0, Y0, X1, Y1, value), 4-byte aligned. An edge with Y0 == Y1 is ignored. Its sign is
 *              w = +1 when Y1 < Y0, else -1: a ring with the region on the right of its travel direction, as the exterior
 *              rings of the region outlines run, has +1 on its left flank. The caller orients holes the other way.
 *   crossing:  an edge crosses row r iff min(Y0, Y1) <= 256 r + 128 < max(Y0, Y1) (half-open: a vertex on a centre line counts
 *              once). With the endpoints ordered so that Y0 < Y1 (both directions of a shared edge then agree), its intercept
 *              is Xi = X0 + (X1 - X0) (256 r + 128 - Y0) / (Y1 - Y0), and it affects the columns c >= c0,
 *              c0 = ceil((Xi - 128) / 256) = ceil(((X0 - 128) (Y1 - Y0) + (X1 - X0) (256 r + 128 - Y0)) / (256 (Y1 - Y0))),
 *              one integer ceiling division, clamped to 0 .. W. The top-left rule: a centre exactly on a left flank is inside,
 *              on a right flank outside; polygons that share an edge tile the plane with no gap and no double cover.
 *   pixel:     over the crossings of its row with c0 <= c: cover = sum of w, vsum = sum of w * value (the caller keeps the sum of
 *              |value| over the edges that cross any one row below 2^31, so no partial sum leaves int32).
 *              (cover, vsum) == (0, 0): background, `fill`, or base[r][c] when `base` (same element type and shape, never
 *              written) is given; cover == 1 with vsum representable in the element type and != overlap_value: vsum;
 *              anything else: overlap_value (overlapping polygons, self-intersections, a hole outside its exterior).
 *   overlap_pixels: int64 on the device, 8-byte aligned: the number of pixels decided by the last case.
 *   scratch:   insar_raster_scratch_bytes(...) bytes, 16-byte aligned; nothing in it has to survive between calls or be cleared.
 *              max_crossings (0 .. 2^30) is the capacity of the record array: at least the number of pairs (edge, row in [0, H))
 *              that cross, which the caller counts exactly on the host. Records beyond it are dropped, never written.
 * Rows are filled in bands of insar_raster_band_rows(W) rows, one work-group per band with two int32 LDS planes of W + 1 columns
 * per row. 5 launches on the caller's stream whatever the table holds (clear, count, scan, emit, fill); no work-group waits on
 * another, no read-back; integer sums only, so the map is bitwise reproducible although the order of a band's records is not.
 * Four pixels per store (and per read of `base`) where W % 4 == 0 and the pointer is 4-byte (uint8) or 16-byte (int32) aligned,
 * guarded scalars otherwise: misalignment is no error. Every argument is checked before the device is touched. */
enum { INSAR_RASTER_U8 = 0, INSAR_RASTER_I32 = 1 };
/* host only: the rows of a band at scene width W: a power of two, 1 .. 32, the largest whose planes fit 136 KiB of LDS */
int insar_raster_band_rows(int32_t W);
/* host only: the launches of one call: 5 */
int insar_raster_launches(void);
/* host only: bytes of scratch for an H x W scene with room for max_crossings records */
int insar_raster_scratch_bytes(int32_t H, int32_t W, int64_t max_crossings, int64_t* scratch_bytes);
/* 5 launches. edges may be null when n_edges == 0 (0 .. 2^28); base is nullable; fill and overlap_value lie in 0 .. 255 for uint8. */
int insar_raster_polygons(const int32_t* edges, int32_t n_edges, int32_t H, int32_t W, int64_t max_crossings, int32_t elem_type,
                          int32_t fill, int32_t overlap_value, const void* base /*nullable*/, void* out, void* scratch,
                          int64_t* overlap_pixels, void* stream);

/* ---- overlaps of two label maps (build-side addition; the reference scores pixels only): csrc/overlap.hip ----------------
 * pred, gt int32 [H][W] (row-major, H * W < 2^31): 0 or a region id >= 1, as insar_regions_relabel writes them. voidmap uint8
 * [H][W], nullable: a pixel is dropped iff voidmap is given and voidmap[i] == void_value (0..255). Every remaining pixel with
 * (pred[i], gt[i]) != (0, 0) is counted under the key (pred[i], gt[i]); the rows (p, 0) and columns (0, g) are part of the
 * table, so the areas after voiding are its row and column sums. Call clear, count, compact in this order on one stream: one
 * launch each, no allocation, no synchronisation, no work-group waits on another. Every argument is checked before the device is
 * touched.
 *   table: insar_overlap_scratch_bytes(...) bytes, 16-byte aligned: a 16-byte header {int64 overflow, int64 reserved}, then
 *          `capacity` slots {uint64 key = pred << 32 | gt, int64 count}, capacity = the smallest power of two >= 2 * max_pairs;
 *          open addressing, key 0 = empty. A contribution that finds no slot within `capacity` probe steps sets `overflow` and
 *          is dropped.
 *   out:   16-byte aligned: a header {int64 n_keys, int64 overflow}, then InsarOverlap [max_pairs]. n_keys is the TRUE number of
 *          keys in the table, which may exceed max_pairs; records 0..min(n_keys, max_pairs) - 1 are written, in no specified
 *          order (sort them; the counts are integer sums, so the sorted table is bitwise reproducible). */
typedef struct InsarOverlap {
  int32_t pred, gt;
  int64_t count;
} InsarOverlap;
/* host only: bytes of the table and of the output for 1 <= max_pairs <= 2^24 */
int insar_overlap_scratch_bytes(int64_t max_pairs, int64_t* table_bytes, int64_t* out_bytes);
/* 1 launch: the table and the header of `out` zeroed. Once before every count + compact. */
int insar_overlap_clear(void* table, void* out, int64_t max_pairs, void* stream);
/* 1 launch: the counts added into the table; every access to the table is an agent-scope atomic. 16-byte loads of the label
 * maps where H * W % 4 == 0 and the pointers allow it (voidmap: 4-byte), guarded scalars otherwise: misalignment is no error. */
int insar_overlap_count(const int32_t* pred, const int32_t* gt, const uint8_t* voidmap /*nullable*/, int32_t void_value,
                        int32_t H, int32_t W, void* table, int64_t max_pairs, void* stream);
/* 1 launch: the non-empty slots written to `out`, its header filled in. */
int insar_overlap_compact(const void* table, int64_t max_pairs, void* out, void* stream);

/* ---- statistics of a raster over the regions of a label map (build-side addition; the reference has no post-processing):
 * csrc/zonal.hip ---------------------------------------------------------------------------------------------------------
 * labels int32 [H][W] (row-major, H * W < 2^31): a value <= 0 is background, the labels 1..max_regions are measured, a pixel
 * with a larger label is counted in the header and written nowhere. raster [channels][H][W], 1 <= channels <= 4, float32, uint8
 * or int32 (INSAR_ZONAL_*). Per pixel of a measured label and per channel:
 *   integer rasters: q = v. float32: d = (double)v * scale, clamped to +-(2^31 - 1); q = d rounded to nearest, ties to even. A
 *   product outside the clamp makes the pixel CLIPPED: it takes part with the clamped q. scale is positive and finite.
 *   A pixel is INVALID if it is not finite or (has_nodata) equals nodata in the raster's own type (float32: v == (float)nodata;
 *   integers: nodata must be an integer in int32). Invalid pixels are counted and take no other part. NaN nodata is refused.
 * Record l of channel c is InsarZonalStat number 1 + c * max_regions + (l - 1) of the table; record 0 is the header, whose
 * sum_q is the number of pixels with a label above max_regions. With bins > 0 (<= 256) the histograms follow the records:
 * uint32 [channels][max_regions][bins]; a valid pixel with q_lo <= q < q_hi goes to bin floor((q - q_lo) * bins / (q_hi - q_lo))
 * (int64 arithmetic), q < q_lo adds to `below`, q >= q_hi to `above`; -2^31 <= q_lo < q_hi <= 2^31.
 * Call clear, then accumulate, on one stream: one launch each whatever the map holds, no allocation, no read-back, no
 * synchronisation, no work-group waits on another. Integer atomics only (agent scope, relaxed), after folding per thread, per
 * wave run and, for the label a work-group sees most, per work-group in LDS: every field is independent of the order and the
 * table is bitwise reproducible. Every argument is checked before the device is touched. */
enum { INSAR_ZONAL_F32 = 0, INSAR_ZONAL_U8 = 1, INSAR_ZONAL_I32 = 2 };
typedef struct InsarZonalStat {
  int64_t sum_q;                     /*  0: sum of q over the valid pixels (header: pixels with a label above max_regions) */
  uint64_t sumsq_lo;                 /*  8: sum of the low 32 bits of q^2 */
  uint64_t sumsq_hi;                 /* 16: sum of q^2 >> 32; the square sum is sumsq_lo + (sumsq_hi << 32), exact, up to 93 bits */
  uint64_t min_key;                  /* 24: (uint32(q) ^ 2^31) << 32 | idx of the first pixel with the smallest q; all ones: none */
  uint64_t max_key;                  /* 32: (uint32(q) ^ 2^31) << 32 | uint32(~idx) of the first pixel with the largest q; 0: none */
  int32_t n, n_invalid, n_clipped;   /* 40: valid pixels; invalid ones; valid ones whose product was clamped */
  uint32_t below, above;             /* 52: valid pixels with q < q_lo, with q >= q_hi (bins > 0) */
  int32_t _pad;
} InsarZonalStat;
/* host only: bytes of the table for 1 <= max_regions <= 2^24, 0 <= bins <= 256, 1 <= channels <= 4 (a multiple of 16, monotone
 * in every argument) */
int insar_zonal_scratch_bytes(int32_t max_regions, int32_t bins, int32_t channels, int64_t* table_bytes);
/* 1 launch: the table zeroed, every min_key all ones. Once before every accumulate. table 16-byte aligned. */
int insar_zonal_clear(void* table, int32_t max_regions, int32_t bins, int32_t channels, void* stream);
/* 1 launch. 16-byte loads where H * W % 4 == 0 and the pointers allow it (uint8: 4-byte), guarded scalars otherwise:
 * misalignment is no error. The raster under background pixels is not read. labels and raster are never written. */
int insar_zonal_accumulate(const int32_t* labels, const void* raster, int32_t elem_type, int32_t channels, int32_t H, int32_t W,
                           double scale, int32_t has_nodata, double nodata, int32_t bins, int64_t q_lo, int64_t q_hi,
                           int32_t max_regions, void* table, void* stream);

/* ---- filtering rasters: NaN-aware smoothing, rank filters and slope (build-side addition; the reference has no
 * post-processing): csrc/focal.hip -------------------------------------------------------------------------------------------
 * Neighbourhood operations on a raster [planes][H][W] (row-major; INSAR_ZONAL_F32 / _U8 / _I32; H, W >= 1, H * W < 2^31, 1 <=
 * planes <= 65535; the planes are independent and go on the grid's z dimension). A pixel is VALID iff it lies inside the raster,
 * valid[y][x] != 0 (valid: uint8 [H][W], shared by the planes, nullable), it does not equal `nodata` in the raster's own type
 * (has_nodata; NaN is refused) and, in a float32 raster, it is finite. Outside the raster is invalid: there is no padding mode.
 * keep_invalid != 0: an output whose CENTRE pixel is invalid is invalid; 0: it is filled from its neighbours. An invalid output
 * is the quiet NaN 0x7fc00000 in float32 and `fill` in integer outputs (uint8: 0..255). out: the raster's layout (gradient:
 * float32 [planes][2][H][W]), never the raster itself; out_valid (nullable): uint8 [planes][H][W], 1 where the output is valid.
 * One launch per call on `stream`, no atomics, no work-group waits on another, nothing read back and no copy: the taps and
 * scalars are kernel arguments. Every output is bitwise defined (tests/focal_ref.py restates all of it). Every argument is
 * checked before the device is touched (INSAR_E_ARG, INSAR_E_SHAPE, INSAR_E_DTYPE, INSAR_E_ALIGN). */
enum { INSAR_FOCAL_MIN = 0, INSAR_FOCAL_MAX = 1, INSAR_FOCAL_MEDIAN = 2 };
/* host only: the rows and columns of outputs one work-group of the smoothing and min / max kernels computes at `radius` 0..15 */
int insar_focal_tile(int32_t radius, int32_t* rows, int32_t* cols);
/* Separable normalised convolution in exact integers. taps: HOST int32 [2 radius + 1], each >= 0, 1 <= sum S <= 4096, 0 <= radius
 * <= 15; tap i multiplies the pixel at offset i - radius (correlation, nothing is flipped); the same taps serve rows and columns.
 *   q:      integer rasters q = v; float32 q = rint(clamp((double)v * scale, +-(2^31 - 1))) to nearest even, the rule of
 *           insar_zonal_accumulate; m = 1 for a valid pixel, else 0.
 *   rows:   A[y][x] = sum_i k[i] m[y][x+i] q[y][x+i], Wr[y][x] = sum_i k[i] m[y][x+i]
 *   cols:   N = sum_j k[j] A[y+j][x], D = sum_j k[j] Wr[y+j][x]            (int64: |A| < 2^43, |N| < 2^55, D <= S^2)
 *   valid:  D >= threshold (1 <= threshold <= S^2; the host's max(1, ceil(min_coverage S^2))), and the keep_invalid rule
 *   value:  q_out = floor((2 N + D) / (2 D)), a floor division: ties go towards +infinity for both signs. float32 output
 *           (float)((double)q_out / scale); integer outputs hold q_out (a convex combination: in range). */
int insar_focal_smooth(const void* raster, int32_t elem_type, int32_t planes, int32_t H, int32_t W, const int32_t* taps, int32_t radius,
                       double scale, int32_t has_nodata, double nodata, const uint8_t* valid, int64_t threshold, int32_t keep_invalid,
                       int32_t fill, void* out, uint8_t* out_valid, void* stream);
/* op (INSAR_FOCAL_*) over the n valid pixels of the (2 radius + 1)^2 window, on the raw values. float32 values are ordered by the
 * key u = bits; u & 2^31 ? ~u : u ^ 2^31 (-0.0 directly below 0.0) and the output is the exact bit pattern of the chosen pixel;
 * integers use their own order. min, max: 1 <= radius <= 15. median: 1 <= radius <= 3, the LOWER median, element (n - 1) / 2 of
 * the sorted values; nothing is averaged. The output is valid iff n >= min_count (1 .. (2 radius + 1)^2), and the keep_invalid rule. */
int insar_focal_rank(const void* raster, int32_t elem_type, int32_t planes, int32_t H, int32_t W, int32_t op, int32_t radius,
                     int32_t has_nodata, double nodata, const uint8_t* valid, int32_t min_count, int32_t keep_invalid, int32_t fill,
                     void* out, uint8_t* out_valid, void* stream);
/* Slope of a float32 raster: out[p][0] = gy, out[p][1] = gx, float32 operations in this order, no fused multiply-add. Along x,
 * with v- , v0, v+ the pixels at x - 1, x, x + 1 (and unless keep_invalid refuses an invalid centre): both neighbours valid
 * (v+ - v-) * hx2; else centre and x + 1 valid (v+ - v0) * hx1; else centre and x - 1 valid (v0 - v-) * hx1; else NaN. y likewise
 * with hy1, hy2. h1 = (float)(1 / spacing), h2 = (float)(1 / (2 spacing)), computed by the host: positive and finite. out_valid
 * marks the pixels where BOTH components are valid. */
int insar_focal_gradient(const float* raster, int32_t planes, int32_t H, int32_t W, float hy1, float hy2, float hx1, float hx2,
                         int32_t has_nodata, double nodata, const uint8_t* valid, int32_t keep_invalid, float* out, uint8_t* out_valid,
                         void* stream);

/* ---- grey-scale reconstruction: fill sinks, h-domes, regional extrema (build-side addition; the reference has no
 * post-processing): csrc/reconstruct.hip -----------------------------------------------------------------------------------------
 * Reconstruction by dilation of a marker F under a mask G over a raster [planes][H][W] (layout, element types, limits and the
 * valid / nodata arguments as for the focal operations above): the pointwise limit of J <- min(G, max of J over the pixel and its
 * `connectivity` (4 or 8) neighbours) from J = min(F, G), on order-preserving 32-bit KEYS of the raw values: float32 u = bits;
 * u & 2^31 ? ~u : u ^ 2^31; int32 with the sign bit flipped; uint8 as it is. flip = 1 complements the keys: reconstruction by
 * erosion. A pixel is VALID iff it lies inside the raster, valid[y][x] != 0, its mask value is valid by the focal rule and its
 * marker value (INSAR_RECONSTRUCT_PLAIN) is neither NaN nor `nodata` (a marker of +-inf is taken as it is). An invalid pixel has
 * the mask key 0: it neither takes nor passes a value. `mode` names the marker:
 *   INSAR_RECONSTRUCT_PLAIN    `marker`, the mask's type and layout (every other mode: marker = NULL)
 *   INSAR_RECONSTRUCT_FILL     the mask at OUTLETS, key 0 elsewhere; an outlet is a valid pixel with a `connectivity` neighbour that
 *                              is invalid or outside the raster. flip = 1 fills sinks, flip = 0 fills domes.
 *   INSAR_RECONSTRUCT_HDOME    mask - h (flip = 0) or mask + h (flip = 1): one float32 operation, or a saturating integer one;
 *                              h > 0, finite in float32, an integer <= 2^31 - 1 for integer rasters
 *   INSAR_RECONSTRUCT_EXTREMA  the mask's key - 1, saturating at 0 (flip = 0: maxima, 1: minima)
 * scratch: insar_reconstruct_bytes(...) bytes, 16-byte aligned: two key planes of J, one of G, two tile-activity maps and the
 * (changed tiles, active tiles) int32 pair of every round, INSAR_RECONSTRUCT_MAX_ROUNDS + 1 of them, at the scratch's end. Nothing in
 * it has to survive between calls; prepare, rounds and finish of one call share it. No atomics on pixel data, no work-group
 * waits on another; the fixed point is unique, so the outputs and the number of rounds are bitwise defined
 * (tests/reconstruct_ref.py restates both). */
enum { INSAR_RECONSTRUCT_PLAIN = 0, INSAR_RECONSTRUCT_FILL = 1, INSAR_RECONSTRUCT_HDOME = 2, INSAR_RECONSTRUCT_EXTREMA = 3 };
#define INSAR_RECONSTRUCT_MAX_ROUNDS 65535
/* host only: the edge of the square tile one work-group of a round solves */
int insar_reconstruct_tile(int32_t* edge);
/* host only: the bytes of `scratch`; the counter pairs are its last 8 * (INSAR_RECONSTRUCT_MAX_ROUNDS + 1) bytes */
int insar_reconstruct_bytes(int32_t planes, int32_t H, int32_t W, int64_t* scratch_bytes);
/* ONE launch: the key planes G and J = min(F, G), every tile active, the counter pairs of rounds 0 .. max_rounds at 0; the rounds
 * of this call stay below max_rounds (1 .. INSAR_RECONSTRUCT_MAX_ROUNDS) */
int insar_reconstruct_prepare(const void* marker, const void* mask, int32_t elem_type, int32_t planes, int32_t H, int32_t W,
                              int32_t mode, int32_t flip, int32_t connectivity, double h, int32_t max_rounds, int32_t has_nodata,
                              double nodata, const uint8_t* valid, void* scratch, void* stream);
/* n_rounds launches, rounds first_round .. first_round + n_rounds - 1 (in order, from 0, at most INSAR_RECONSTRUCT_MAX_ROUNDS in
 * all). A round solves every ACTIVE tile to its local fixed point from the plane of the round before and writes the other
 * plane; a tile is active in round 0, and in round r + 1 iff it or one of its 8 neighbours changed in round r. Round r adds
 * to counter pair r. A round whose changed count is 0 has reached the fixed point; further rounds change nothing. */
int insar_reconstruct_rounds(int32_t planes, int32_t H, int32_t W, int32_t connectivity, int32_t first_round, int32_t n_rounds,
                             void* scratch, void* stream);
/* ONE launch, after `rounds_run` rounds. Every output is nullable (at least one is given) and [planes][H][W]:
 *   out        the mask's type: the reconstruction; an invalid pixel holds the quiet NaN 0x7fc00000 / `fill`; never marker or mask
 *   residue    float32 for a float32 raster, else int32: mask - reconstruction (flip = 0) or reconstruction - mask (flip = 1),
 *              never negative: one float32 subtraction, or an exact integer saturating at 2^31 - 1; invalid: NaN / 0
 *   extrema    uint8: 1 where the pixel is valid and its mask key exceeds the reconstruction's
 *   out_valid  uint8: 1 at valid pixels */
int insar_reconstruct_finish(const void* marker, const void* mask, int32_t elem_type, int32_t planes, int32_t H, int32_t W,
                             int32_t mode, int32_t flip, int32_t has_nodata, double nodata, const uint8_t* valid, int32_t rounds_run,
                             int32_t fill, void* scratch, void* out, void* residue, uint8_t* extrema, uint8_t* out_valid, void* stream);

/* ---- distance transform (build-side addition; the reference has no post-processing): csrc/distance.hip --------------------
 * The exact squared Euclidean distance from every pixel of a map m [B][H][W] (row-major; uint8 with INSAR_DIST_U8, int32 with
 * INSAR_DIST_I32; B, H, W >= 1, H, W <= 32767, B * H * W < 2^31, no tile-multiple requirement) to the nearest SITE of the same
 * image, and that site. Images of a batch never see each other. Sites by `site_mode` and `value`:
 *   INSAR_DIST_EQ    the pixels with m == value
 *   INSAR_DIST_NE    the pixels with m != value
 *   INSAR_DIST_EDGE  the pixels p with m[p] != value that have a 4-neighbour q inside the image with m[q] != value and
 *                    m[q] != m[p]: both sides of a class border, never the image border; `value` is the ignored value, < 0: none
 *   d2:      int32 [B][H][W]: the squared distance, 0 on sites; INSAR_DIST_FAR where it exceeds max_distance^2 (a pixel at
 *            exactly max_distance keeps its value) or the image has no site. max_distance <= 0: unbounded.
 *   nearest: int32 [B][H][W], nullable: the index y * W + x within the image of a nearest site, -1 where d2 is FAR. Of several
 *            nearest sites the one with the SMALLEST index: the outputs are bitwise defined.
 *   scratch: insar_dist_scratch_bytes(...) bytes: int16 [B][H][W], the row of the nearest site of each pixel's column. Nothing in
 *            it has to survive between calls or be cleared by the caller.
 * Integers only, no atomics, two launches (columns, rows) on the caller's stream. Every argument is checked before the device
 * is touched (null pointers, sizes, element type, site mode, alignment of the int32 buffers). */
enum { INSAR_DIST_U8 = 0, INSAR_DIST_I32 = 1 };
enum { INSAR_DIST_EQ = 0, INSAR_DIST_NE = 1, INSAR_DIST_EDGE = 2 };
#define INSAR_DIST_FAR 0x7fffffff
/* host only: bytes of scratch for a B x H x W map (a multiple of 16, monotone in every argument) */
int insar_dist_scratch_bytes(int32_t B, int32_t H, int32_t W, int64_t* scratch_bytes);
/* 2 launches. m is never written. */
int insar_dist_transform(const void* m, int32_t elem_type, int32_t B, int32_t H, int32_t W, int32_t site_mode, int32_t value,
                         int32_t max_distance, void* scratch, int32_t* d2, int32_t* nearest /*nullable*/, void* stream);
/* Boundary-band counts of two class maps pred, gt uint8 [H][W] with their EDGE transforms d2_pred, d2_gt: over the pixels
 * with gt != void_value (0..255, or -1: none), P_c = {pred == c and d2_pred <= r2}, G_c = {gt == c and d2_gt <= r2};
 * counts int64 [K][3] = (|P_c & G_c|, |P_c|, |G_c|), 2 <= K <= 8, r2 >= 0 (FAR is in no band). 2 launches (a clear, the counts);
 * integer adds, reduced per thread, wave and work-group before 3 K agent-scope atomics: independent of the launch geometry.
 * 16-byte loads where H * W % 4 == 0 and the pointers allow it, guarded scalars otherwise: misalignment is no error. */
int insar_dist_boundary_counts(const uint8_t* pred, const uint8_t* gt, const int32_t* d2_pred, const int32_t* d2_gt, int32_t H,
                               int32_t W, int64_t r2, int32_t K, int32_t void_value, int64_t* counts, void* stream);

/* ---- centre lines (build-side addition; the reference has no post-processing): csrc/skeleton.hip ---------------------------
 * labels int32 [H][W] (row-major, 1 <= H, W <= 32767): a value <= 0 is background, equal positive values form one region.
 * Thinning: Guo and Hall's two-subiteration parallel thinning (CACM 32(3), 1989) per region. A neighbour of p is SET iff it is
 * inside the image, still alive and carries p's label. With p2 = N, p3 = NE, p4 = E, p5 = SE, p6 = S, p7 = SW, p8 = W, p9 = NW:
 *   C = (!p2 & (p3|p4)) + (!p4 & (p5|p6)) + (!p6 & (p7|p8)) + (!p8 & (p9|p2))
 *   N = min((p9|p2) + (p3|p4) + (p5|p6) + (p7|p8), (p2|p3) + (p4|p5) + (p6|p7) + (p8|p9))
 *   m = (p6 | p7 | !p9) & p8 in the first sub-iteration, (p2 | p3 | !p5) & p4 in the second
 *   p is deleted iff it is alive and C == 1 and 2 <= N <= 3 and !m, every pixel decided from the image before the sub-iteration.
 * One iteration = first then second sub-iteration; max_iterations (1..32768) of them run; an iteration that deletes nothing
 * leaves a fixed point. Kind of a skeleton pixel on the final image, X = the number of k with p_k unset and p_{k+1} set going
 * cyclically round p2..p9: X = 0 isolated (1), 1 end (2), 2 line (3), >= 3 junction (4); 0 = not skeleton.
 *   skeleton: uint8 [H][W], the kinds.
 *   table:    InsarSkeletonStat [1 + max_regions], 16-byte aligned; record l belongs to label l. Record 0 is the header:
 *             n = iterations (those that deleted a pixel), n_end = converged (iterations < max_iterations), n_junction = the
 *             largest label in the map, n_orth = 1 iff a label above max_regions occurs. Pixels of such labels are thinned and
 *             classified like any other and enter no record; no kernel uses them as an index.
 *   d2:       nullable; int32 [H][W], the INSAR_DIST_EDGE transform of `labels` (no ignored value). Skeleton pixels with
 *             d2 == INSAR_DIST_FAR count into n_far and neither into sum_d2 nor max_d2; without d2 the three stay 0.
 *   scratch:  insar_skeleton_scratch_bytes(...) bytes, 16-byte aligned: ten bit planes of H * ceil(W / 64) 64-bit words (eight
 *             same-label link planes, the alive map twice), the tiles' change flags and max_iterations iteration flags. Nothing
 *             in it has to survive between calls or be cleared by the caller.
 * Call planes, then step for step = 0 .. ceil(max_iterations / 8) - 1, then stats, on one stream with the same H, W,
 * max_iterations: ONE launch per call, 2 + ceil(max_iterations / 8) in all whatever the map holds, no read-back, no
 * synchronisation, no work-group waits on another, integers only (bitwise reproducible). Every argument is checked before the
 * device is touched. */
typedef struct InsarSkeletonStat {
  int64_t sum_y, sum_x;            /* over the region's skeleton pixels (y down, x to the right) */
  int64_t sum_yy, sum_xx, sum_xy;
  int64_t sum_d2;                  /* over those whose d2 is not FAR */
  int32_t n, n_end, n_junction;    /* skeleton pixels; of kind end; of kind junction (header: iterations, converged, largest label) */
  int32_t n_orth;                  /* 4-adjacent pairs of skeleton pixels of the region, each once (header: overflow flag) */
  int32_t n_diag;                  /* diagonal pairs neither of whose two common 4-neighbours is a skeleton pixel of the region */
  int32_t n_far;                   /* skeleton pixels whose d2 is FAR */
  int32_t max_d2;                  /* the largest d2 that is not FAR */
  int32_t _pad;
} InsarSkeletonStat;
/* host only: bytes of scratch for an H x W map and max_iterations, and of a table of max_regions records */
int insar_skeleton_scratch_bytes(int32_t H, int32_t W, int32_t max_iterations, int32_t max_regions, int64_t* scratch_bytes,
                                 int64_t* table_bytes);
/* host only: the launches of one thinning: 2 + ceil(max_iterations / 8), plus the 2 of insar_dist_transform with `widths` */
int insar_skeleton_launches(int32_t H, int32_t W, int32_t max_iterations, int32_t widths);
/* 1 launch: the bit planes from the labels; the table and the iteration flags cleared. */
int insar_skeleton_planes(const int32_t* labels, int32_t H, int32_t W, int32_t max_iterations, int32_t max_regions, void* scratch,
                          void* table, void* stream);
/* 1 launch: iterations 8 step .. min(8 step + 8, max_iterations) - 1, one 96 x 384 pixel tile per work-group with a halo of 16
 * pixels in LDS; the alive map goes from one of its two copies to the other, written whole. */
int insar_skeleton_step(int32_t H, int32_t W, int32_t max_iterations, int32_t step, void* scratch, void* stream);
/* 1 launch: the kinds, the records (runs of equal labels folded per wave, then agent-scope integer atomics) and the header. */
int insar_skeleton_stats(const int32_t* labels, const int32_t* d2 /*nullable*/, int32_t H, int32_t W, int32_t max_iterations,
                         int32_t max_regions, void* scratch, void* table, uint8_t* skeleton, void* stream);

/* ---- augmentation and test-time augmentation (build-side addition; the reference resizes and normalises, nothing else):
 * csrc/augment.hip ------------------------------------------------------------------------------------------------------
 * A parameter table is a device array int32 [n][4], 16-byte aligned; row s = {int32 op, float gain, float bias, float sigma}
 * of sample s. D4 op codes 0..7 on an [H][W] plane a, in numpy terms: b = a.T if op & 4 else a; if op & 2: b = b[::-1, :];
 * if op & 1: b = b[:, ::-1] (rot90(a, 1) is op 6, rot90(a, 3) is op 5; every op is its own inverse except 5 <-> 6). The
 * kernels use op & 7 and, where H != W, clear bit 2: no content of a table makes them leave the planes.
 *   aug_hash64(key, i): z = key + 0x9E3779B97F4A7C15 * (i + 1); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                       z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)           (uint64, wrap-around)
 * Both validate every argument before they touch the device. */
enum { INSAR_AUG_MASK_NONE = 0, INSAR_AUG_MASK_U8 = 1, INSAR_AUG_MASK_I64 = 2 };
/* Fill the table for n samples. key = seed ^ (step * 0xD1B54A32D192ED03); h_j = aug_hash64(key, 4 s + j) >> 32, j = 0..3;
 * op = the (h_0 % popcount(ops_mask))-th set bit of ops_mask (1..255) counting from bit 0; u(h) = (float)(h >> 8) * 2^-24;
 * gain = gain_lo + (gain_hi - gain_lo) * u(h_1) in fp32, product and sum rounded separately; bias, sigma likewise from
 * h_2, h_3. lo <= hi, all bounds finite, sigma_lo >= 0. */
int insar_aug_draw(uint64_t seed, uint64_t step, int32_t n, int32_t ops_mask, float gain_lo, float gain_hi, float bias_lo,
                   float bias_hi, float sigma_lo, float sigma_hi, int32_t* table, void* stream);
/* x, xo fp32 [n][C][H][W]; m [n][H][W] uint8 or int64 (m_dtype), mo int64 [n][H][W]; either pair may be null, not both;
 * never in place; H, W <= 32768. With (i', j') the source index the op of sample s assigns to output (i, j):
 *   t = gain_s * x[s][c][i'][j']; t = t + bias_s; if sigma_s != 0: t = t + sigma_s * z; xo[s][c][i][j] = t
 *   mo[s][i][j] = (int64) m[s][i'][j']
 * z = (float)(S - 131070) * 0x1.bb67aep-16f, S = the sum of the four 16-bit fields of aug_hash64(noise_seed, lin),
 * lin = ((s * C + c) * H + i) * W + j the OUTPUT index: approximately unit normal, |z| < 3.47. Every product and sum above is
 * rounded on its own (no fused multiply-add). 16-byte accesses where W % 4 == 0 and the pointers are 16-byte aligned
 * (uint8 masks: 4-byte), element-wise ones otherwise: misalignment is not an error. */
int insar_aug_apply(const float* x, float* xo, int32_t C, const void* m, int32_t m_dtype /*INSAR_AUG_MASK_**/, int64_t* mo,
                    int32_t n, int32_t H, int32_t W, const int32_t* table, uint64_t noise_seed, void* stream);

/* ---- training from whole scenes: class-balanced crops drawn on the device (build-side addition; the reference trains from
 * pre-cut tiles): csrc/crops.hip ----------------------------------------------------------------------------------------------
 * labels: uint8 [H][W], H * W < 2^31. With a cell size g >= 1 (g <= H, W), Hc = H / g and Wc = W / g (floor: the ragged rows
 * and columns at the far edges belong to no cell) and K classes, 2 <= K <= 8, the TABLE is int32 [K + 1][Hc + 1][Wc + 1].
 * Plane p < K counts the pixels with label p; plane K counts the void pixels: label 255 and every other label >= K.
 * Integers only, no atomics, nothing read back: every output below is bitwise defined. Every argument is checked before the
 * device is touched (INSAR_E_ARG: null pointers, tries; INSAR_E_SHAPE: K, g, T, H, W; INSAR_E_DTYPE; INSAR_E_ALIGN). */
/* table[p][1 + i][1 + j] = the pixels of cell (i, j) (rows i g .. i g + g - 1, columns j g .. j g + g - 1) in plane p; row 0
 * and column 0 = 0. 1 launch. 16-byte loads where g is 1, 2, 4, 8 or 16, W % 16 == 0 and labels is 16-byte aligned, byte
 * loads otherwise: misalignment is no error. */
int insar_crops_cells(const uint8_t* labels, int32_t H, int32_t W, int32_t K, int32_t g, int32_t* table, void* stream);
/* In place: table[p][a][b] <- the sum of the cells (i, j) with i < a, j < b (the exclusive 2-D prefix sums), so that the
 * cells [a0, a1) x [b0, b1) hold table[p][a1][b1] - table[p][a0][b1] - table[p][a1][b0] + table[p][a0][b0] pixels of plane p.
 * 2 launches (rows, columns). Exact for any Hc, Wc >= 1 with (Hc + 1) * (Wc + 1) < 2^31. */
int insar_crops_sat(int32_t* table, int32_t K, int32_t Hc, int32_t Wc, void* stream);
/* Draw n tile origins from the summed table `sat` of a scene: T x T tiles, T % g == 0, T <= H, W; 1 <= tries <= 64;
 * cum: HOST array of K floats, the cumulative class probabilities (read before the launch); origins int32 [n][2] = (y0, x0);
 * info int32 [n][4] = {target class, accepted try or -1, pixels of that class in the chosen tile, void pixels in it}.
 * One wave per sample, lane t evaluates try t. With h(i) = aug_hash64(key, i) (below) sample s uses counter base b = s * 65.
 *   Target class: u = float32(h(b) >> 40) * 2^-24; the target is the first c with u < cum[c]; the last class is the default.
 *   Origin of try t: with r = h(b + 1 + t), ny = Hc - T/g + 1 and nx = Wc - T/g + 1:
 *     cy = ((r >> 32) * ny) >> 32, cx = ((r & 0xffffffff) * nx) >> 32, origin = (cy * g, cx * g).
 *   Acceptance: a try is accepted if its tile holds >= min_count pixels of the target class and <= max_void void pixels. The
 *     lowest accepted t wins (a ballot).
 *   Fallback when no try is accepted: the try with the most target-class pixels among those within the void cap; if no try is
 *     within the void cap, the try with the fewest void pixels. Ties go to the lowest t. The accepted-try field of info is -1.
 * 1 launch. */
int insar_crops_draw(uint64_t key, int32_t n, int32_t K, int32_t tries, const float* cum, int32_t min_count, int32_t max_void,
                     int32_t T, int32_t g, int32_t H, int32_t W, const int32_t* sat, int32_t* origins, int32_t* info, void* stream);
/* images float32 [n][1][T][T] <- the tiles of `scene` (uint8 or float32 [H][W], INSAR_SCENE_*) at `origins`, normalised as
 * insar_scene_gather does and bitwise equal to its result; masks [n][T][T], int64 or uint8 (INSAR_AUG_MASK_I64 / _U8) <- the
 * tiles of `labels` at the same origins, labels copied unchanged. Either output may be null (then its source may be too), not
 * both. T % 4 == 0, T <= H, W. A tile whose origin leaves the scene is zero-filled, its labels are 255. 1 launch. */
int insar_crops_gather(const void* scene, int32_t scene_dtype, const uint8_t* labels, int32_t H, int32_t W, const int32_t* origins,
                       int32_t n, int32_t T, float* images, void* masks, int32_t mask_dtype, void* stream);

/* ---- resampling rasters: fixed-point affine warp and multilook (build-side addition; the reference resizes tiles on the
 * host): csrc/warp.hip ------------------------------------------------------------------------------------------------------
 * A WARP is six int64 {a, b, c, d, e, f} in Q32 that take the pixel INDICES (x, y) of a destination h x w to a source H x W,
 * H * W < 2^31; an integer index is a pixel centre. Per destination pixel, in int64 with wrap-around:
 *   SXq = a x + b y + c, SYq = d x + e y + f;  sx = (SXq + 2^23) >> 24, sy = (SYq + 2^23) >> 24    (arithmetic shifts)
 * are the source position in 1/256 pixel. The pixel is INSIDE iff -128 <= sx < 256 W - 128 and -128 <= sy < 256 H - 128: its
 * centre lies on the source's pixel extent. Every other pixel is written as the fill value. For an inside pixel:
 *   nearest:  ix = (sx + 128) >> 8, iy = (sy + 128) >> 8; the value is src[iy][ix].
 *   bilinear: ix = sx >> 8, fx = sx & 255, iy = sy >> 8, fy = sy & 255; the taps v00 = src[y0][x0], v01 = src[y0][x1],
 *             v10 = src[y1][x0], v11 = src[y1][x1] with x0 = max(ix, 0), x1 = min(ix + 1, W - 1), y0, y1 likewise.
 *     uint8:   (v00 (256 - fx)(256 - fy) + v01 fx (256 - fy) + v10 (256 - fx) fy + v11 fx fy + 32768) >> 16, integers only.
 *     float32: ((v00 * (256 - fx) + v01 * fx) * (256 - fy) + (v10 * (256 - fx) + v11 * fx) * fy) * 2^-16, the weights
 *              converted to float32, every product and sum rounded to float32 in that order (no fused multiply-add). NaN
 *              and infinity follow IEEE: a NaN tap gives NaN, also where its weight is 0. A NaN result is stored as the
 *              quiet NaN 0x7fc00000, whatever payload the operations handed on.
 * Nothing is read back, there are no atomics: every output is bitwise defined (tests/warp_ref.py restates all of it). Every
 * argument is checked before the device is touched (INSAR_E_ARG, INSAR_E_SHAPE, INSAR_E_DTYPE, INSAR_E_ALIGN). */
enum { INSAR_WARP_U8 = 0, INSAR_WARP_I32 = 1, INSAR_WARP_F32 = 2 };
enum { INSAR_WARP_NEAREST = 0, INSAR_WARP_BILINEAR = 1 };
/* dst [n][C][h][w] of the source's dtype <- src [C][H][W] (1 <= C <= 4) through the n warps of the device table `matrices`
 * int64 [n][6]; h, w <= 32768. fill_bits: the fill value's bits (uint8: the low byte). valid (nullable): uint8 [n][h][w], 1
 * where inside, else 0. Bilinear on int32 is refused. 16-byte stores (uint8: 4-byte) where w % 4 == 0 and dst is aligned to
 * them, element-wise stores otherwise: misalignment is no error. 1 launch. */
int insar_warp_raster(const void* src, int32_t dtype /*INSAR_WARP_U8 ...*/, int32_t C, int32_t H, int32_t W, const int64_t* matrices,
                      int32_t n, int32_t h, int32_t w, int32_t mode /*INSAR_WARP_NEAREST ...*/, uint32_t fill_bits, void* dst,
                      uint8_t* valid /*nullable*/, void* stream);
/* The warped counterpart of insar_crops_gather, same arguments with the table of warps in place of the origins and T x T
 * outputs (T % 4 == 0, T <= 32768): images float32 [n][1][T][T] <- bilinear; a uint8 scene's interpolated integer v then
 * goes through x = v / 255; (x - 0.5) / 0.5 in float32 as insar_scene_gather does, a float32 scene's value is stored as it
 * is. masks <- nearest. Outside pixels: image `fill`, label 255. With warps {2^32, 0, x0 2^32, 0, 2^32, y0 2^32} of tiles
 * inside the scene the outputs equal insar_crops_gather's bit for bit (float32 scenes: finite values). 1 launch. */
int insar_warp_gather(const void* scene, int32_t scene_dtype, const uint8_t* labels, int32_t H, int32_t W, const int64_t* matrices,
                      int32_t n, int32_t T, float fill, float* images, void* masks, int32_t mask_dtype, void* stream);
/* matrices int64 [n][6] <- one random rotation and zoom per sample about the centre of the T x T tile at origins[i] = (y0, x0)
 * (device int32 [n][2], as insar_crops_draw writes them). angles: device int32 [1024][2], entry j = {rint(cos(2 pi j / 1024)
 * 2^30), rint(sin(2 pi j / 1024) 2^30)} computed by the host in float64. 0 <= amax <= 512; zoom in Q8, source pixels per
 * output pixel, 1 <= zoom_lo <= zoom_hi <= 4096. With r = aug_hash64(key ^ 0x9FB21C651E98DF25, i) (above):
 *   k = (((r >> 32) (2 amax + 1)) >> 32) - amax;  z = zoom_lo + (((r & 0xffffffff) (zoom_hi - zoom_lo + 1)) >> 32)
 *   (cs, sn) = angles[k & 1023];  a = e = (z cs + 32) >> 6;  b = (-(z sn) + 32) >> 6;  d = (z sn + 32) >> 6     (Q38 -> Q32)
 *   c = ((2 x0 + T - 1) << 31) - (((a + b) (T - 1)) >> 1);  f = ((2 y0 + T - 1) << 31) - (((d + e) (T - 1)) >> 1)
 * in int64 with wrap-around: the index x0 + (T - 1) / 2 of the tile's centre (x0 + T / 2 from the tile's corner) maps to
 * itself. amax = 0 with zoom_lo = zoom_hi = 256 gives {2^32, 0, x0 2^32, 0, 2^32, y0 2^32}. 1 launch. */
int insar_warp_draw(uint64_t key, const int32_t* origins, int32_t n, int32_t T, int32_t amax, int32_t zoom_lo, int32_t zoom_hi,
                    const int32_t* angles, int64_t* matrices, void* stream);
/* dst [C][h][w] <- the mean of src [C][H][W] (uint8 or float32, INSAR_WARP_U8 / _F32) over boxes of fy x fx pixels, 1 <= fy,
 * fx <= 16, h = H / fy, w = W / fx (floor: the remainder rows and columns are dropped).
 *   uint8:   (sum + n / 2) / n with n = fy fx, integers; count (nullable, int32 [C][h][w]) = n.
 *   float32: the values that are not NaN are added to a float32 sum that starts at +0, box rows top to bottom and each row left
 *            to right, every sum rounded to float32; the result is sum / (float32) count, or NaN where count < min_valid
 *            (1 <= min_valid <= fy fx); count = the number of values that are not NaN. Every NaN written is 0x7fc00000.
 * 1 launch. */
int insar_multilook(const void* src, int32_t dtype, int32_t C, int32_t H, int32_t W, int32_t fy, int32_t fx, int32_t min_valid,
                    void* dst, int32_t* count /*nullable*/, void* stream);

/* ---- detections through a stack of dates (build-side addition; the reference works on one tile of one date):
 * csrc/stack.hip ---------------------------------------------------------------------------------------------------------
 * State: two device tensors hit and valid, int64 [words][H][W], 1 <= words <= 4, H * W < 2^31, 8-byte aligned. Date t of
 * T = 64 words is bit t & 63 of plane t >> 6. A date is VALID at a pixel where it was observed, a HIT where it is valid and
 * a detection; readers take hit & valid, so a hit bit under a cleared valid bit counts for nothing. Everything is integers,
 * one launch per entry point on the caller's stream, loops bounded by T, no work-group waits on another, nothing is read
 * back. Every argument is checked before the device is touched. 16-byte accesses where H * W % 4 == 0 and the pointers allow
 * it, guarded scalars otherwise: misalignment beyond an element's own is no error. */
/* Dates t .. t + n - 1 <- mask uint8 [n][H][W] (n >= 1, t + n <= T; the dates may cross planes). Per pixel and date:
 *   valid bit = mask != ignore && (valid_in == NULL || valid_in != 0)          ignore in -1..255, -1: no value is ignored
 *   hit bit   = valid && class set holds mask && (conf == NULL || conf >= min_conf)       a NaN conf: valid, no hit
 * class set: classes_w0 .. w3, class c is bit c & 63 of word c >> 6. min_conf finite. Exactly the n bits are set or cleared;
 * every other bit of the words keeps its value. The n planes of every input are read once; a word whose 64 bits are all
 * written is not read. valid_in uint8 [n][H][W], conf float32 [n][H][W], both nullable. The inputs are never written. */
int insar_stack_push(const uint8_t* mask, const uint8_t* valid_in /*nullable*/, const float* conf /*nullable*/, float min_conf,
                     uint64_t classes_w0, uint64_t classes_w1, uint64_t classes_w2, uint64_t classes_w3, int32_t ignore, int32_t n,
                     int32_t t, int32_t words, int32_t H, int32_t W, int64_t* hit, int64_t* valid, void* stream);
/* The k >= 0 oldest dates dropped in place: bit t <- bit t + k across planes, the top k bits <- 0. k >= T clears the stack
 * without reading it; k = 0 is a launch that writes nothing. */
int insar_stack_shift(int64_t* hit, int64_t* valid, int32_t words, int32_t H, int32_t W, int32_t k, void* stream);
/* Per pixel over the window 0 <= t0 <= t1 <= T, defined by ONE scan over t = t0 .. t1 - 1 that skips the dates whose valid
 * bit is 0 (a missing observation neither breaks nor extends a run):
 *   n_valid, n_hit   int16   the valid dates, the hits among them
 *   longest_run      int16   the most consecutive hits among the valid dates
 *   run_start        int16   the date of the first hit of that run, of the earliest such run on ties; -1: no hit
 *   first_hit, last_hit  int16   dates, -1: no hit
 *   known            uint8   n_valid >= min_valid
 *   persistent       uint8   known && n_hit >= min_hits && longest_run >= min_run && n_hit * den >= num * n_valid
 * 0 <= min_hits, min_run, min_valid <= 32767; 0 <= num <= den, 1 <= den < 2^31 (int64 products). Every plane [H][W] is
 * nullable: a null one is neither computed into memory nor touched; all null is INSAR_E_ARG. An empty window gives 0 and -1.
 * The kernel walks the maximal runs of (hit | ~valid) inside the window and counts the hits under each: bitwise the scan. */
int insar_stack_summary(const int64_t* hit, const int64_t* valid, int32_t words, int32_t H, int32_t W, int32_t t0, int32_t t1,
                        int32_t min_hits, int32_t min_run, int32_t min_valid, int32_t num, int32_t den, int16_t* n_valid,
                        int16_t* n_hit, int16_t* longest_run, int16_t* run_start, int16_t* first_hit, int16_t* last_hit,
                        uint8_t* known, uint8_t* persistent, void* stream);
/* Per label of a map and per date of a window: the series table. labels int32 [H][W] as in insar_zonal_accumulate (<= 0
 * background, 1..max_regions counted, larger ones counted in the header and nothing else). With nt = t1 - t0 (0..256) the
 * table is int32: a header of four words (word 0: out_of_range), then max_regions rows of 1 + 2 nt words
 *   {area, hits[nt], valids[nt]}      area: pixels of the label; hits / valids: its pixels that are hits / valid at t0 + i
 * so the first `count` rows are one contiguous read. 1 <= max_regions <= 2^24. Call clear, then series, on one stream.
 * Agent-scope relaxed integer atomic adds only, after folding: each wave takes 4 x 64 consecutive pixels, one ballot per date
 * gives every run of equal labels its count (one add per run and date that is not 0); the label a work-group sees most (the
 * vote of csrc/zonal.hip) is summed without atomics in the lanes (lane i holds date i of a plane), added per work-group in
 * LDS when the vote changes and at the end, and sent to the table from there. hit / valid under background pixels are not
 * read. The table is bitwise reproducible. */
int insar_stack_series_bytes(int32_t max_regions, int32_t n_dates, int64_t* table_bytes);   /* host only; a multiple of 16 */
int insar_stack_series_clear(void* table, int32_t max_regions, int32_t n_dates, void* stream);
int insar_stack_series(const int64_t* hit, const int64_t* valid, int32_t words, const int32_t* labels, int32_t H, int32_t W,
                       int32_t t0, int32_t t1, int32_t max_regions, void* table, void* stream);

/* ---- optimizer: optim.Adam(lr=1e-4) (:466,346), multi-tensor ------------------------------------
 * table: int64[ntensors][5] = {param*, grad*, exp_avg*, exp_avg_sq*, numel}; chunks: int32[nchunks][2]
 * = {tensor index, chunk index}; each chunk covers `chunk_elems` elements. */
int insar_adam_step(const int64_t* table, const int32_t* chunks, int32_t nchunks, int32_t chunk_elems,
                    float lr, float beta1, float beta2, float eps, float bias_correction1,
                    float bias_correction2_sqrt, float grad_scale, void* stream);

/* ---- config 5: DeepLabV3-CA (DeepLabV3-ChannelAttention.py:83-162; backbone / ASPP arithmetic = torchvision's
 * resnet50(replace_stride_with_dilation=[False,True,True]) + DeepLabHead, restated: csrc/deeplab.hip) -----------------
 * Convolutions other than the stem run on insar_igemm (1x1 / 3x3, stride 1|2, dilation through the tap offsets with
 * INSAR_IGEMM_OOB_ZERO) and insar_wgrad with per-tap tables: */
int insar_pixel_table_taps(int32_t* tab /*[ntaps][Mpad]*/, int64_t Mpad, int32_t B, int32_t H, int32_t W, int32_t s,
                           int32_t Hb, int32_t Wb, int32_t ntaps, const int8_t* dy, const int8_t* dx, void* stream);
/* stem: Conv2d(1, 64, 7, stride 2, padding 3, bias=False) on the module input x (NCHW fp32 [B][1][H][W], :105-118).
 * stats: [insar_conv7x7s2_fwd_rows(B, H)][2][64] BatchNorm partial sums (nullable).
 * wgrad: part[insar_conv7x7s2_wgrad_blocks(B, H/2)][64*49] partial rows in torch (64,1,7,7) order. */
int insar_conv7x7s2_fwd_rows(int32_t B, int32_t H);
int insar_conv7x7s2_fwd(const float* x, int32_t H, int32_t W, const float* w, const InsarAct* y, float* stats, void* stream);
int insar_conv7x7s2_wgrad_blocks(int32_t B, int32_t Ho);
int insar_conv7x7s2_wgrad(const float* x, int32_t H, int32_t W, const InsarAct* dy, float* part, void* stream);
/* MaxPool2d(3, stride 2, padding 1) of the stem: arg[B][Ho][Wo][C] = window position ky*3+kx of the first maximum. */
int insar_maxpool3s2_fwd(const InsarAct* x, const InsarAct* y, uint8_t* arg, void* stream);
int insar_maxpool3s2_bwd(const InsarAct* dy, const uint8_t* arg, const InsarAct* dx, void* stream);
/* Bottleneck tail: dst = relu(y*scale + shift + res); and g = dout * (out > 0) (g may alias dout). */
int insar_bn_add_relu(const InsarAct* y, const float* scale, const float* shift, const InsarAct* res, const InsarAct* dst,
                      int32_t relu, void* stream);
int insar_relu_gate_bwd(const InsarAct* dout, const InsarAct* out, const InsarAct* g, void* stream);
/* SE-gated Bottleneck tail (FCN-ResNet50 with BottleneckWithSE): dst = relu(gate[n][c] * (y*scale + shift) + res), gate
 * fp32 [B][C] from insar_se_excite. C's 16-byte chunks (8 bf16 / 4 fp32 channels) must divide or be a multiple of 256. */
int insar_se_res_apply(const InsarAct* y, const float* scale, const float* shift, const float* gate, const InsarAct* res,
                       const InsarAct* dst, void* stream);
/* ASPP pooling branch: out (B,1,1,C) = factor * sum_hw x;  dst (B,H,W,C) (+)= factor * src (B,1,1,C). */
int insar_sum_hw(const InsarAct* x, const InsarAct* out, float factor, void* stream);
int insar_broadcast_hw(const InsarAct* src, const InsarAct* dst, float factor, int32_t accumulate, void* stream);
/* the same, storing zero where `gate` (dst's grid, channels and dtype) is <= 0: the ReLU mask of the residual block whose incoming
 * gradient dst is, applied by its last writer (ABI 4; InsarIgemm.gate is the GEMM writers' form) */
int insar_broadcast_hw_gate(const InsarAct* src, const InsarAct* dst, const InsarAct* gate, float factor, int32_t accumulate, void* stream);
/* Dropout(p): make_mask != 0 draws mask[B][H][W][c_len] from (seed, element index) and stores it; == 0 applies `mask`. */
int insar_dropout(const InsarAct* x, const InsarAct* dst, uint8_t* mask, uint64_t seed, const int64_t* counter /*nullable, device:
                  mixed into the seed so that every replay of a captured step draws a new mask*/, float p, int32_t make_mask, void* stream);
/* F_T.resize(x, size, BILINEAR) (:160): bilinear, align_corners = False, on `planes` fp32 maps; and its adjoint. */
int insar_bilinear_fwd(const float* in, float* out, int32_t planes, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, void* stream);
int insar_bilinear_bwd(const float* dout, float* din, int32_t planes, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, void* stream);

/* The same update with the step count and the bias corrections kept on the device: state = float[4] {t, 1-beta1^t,
 * sqrt(1-beta2^t), -}. The call first advances t by one (a one-thread launch), then updates the parameters; nothing
 * in the launch arguments changes from step to step, so a captured hipGraph of the training step can be replayed. */
int insar_adam_step_dev(const int64_t* table, const int32_t* chunks, int32_t nchunks, int32_t chunk_elems,
                        float lr, double beta1, double beta2, float eps, float* state, float grad_scale, void* stream);

/* ---- optimizer: AdamW with a global-norm clip, a learning-rate schedule and EMA weights (csrc/optim_w.hip; not in the
 * reference) --------------------------------------------------------------------------------------------------------
 * One step is insar_gradnorm_partials (only with clipping or the non-finite check) -> insar_optw_advance ->
 * insar_adamw_step on one stream. Every per-step scalar lives in an InsarOptwState in DEVICE memory, written by
 * insar_optw_advance and read by insar_adamw_step, so no launch argument changes from step to step.
 * table: int64[ntensors][8] = {param*, grad*, exp_avg*, exp_avg_sq*, ema* or 0, numel, bits of float weight_decay (low 32),
 * bits of float lr_mult (low 32)}; chunks / chunk_elems as for insar_adam_step.
 *
 * InsarOptwState (48 bytes, 8-byte aligned; zero-initialised = no step taken, with coef set to 1 by the first advance): */
typedef struct InsarOptwState {
  int64_t t;        /*  0: steps taken (skipped steps do not count) */
  int64_t skipped;  /*  8: steps skipped because the gradient norm was inf or NaN */
  float bc1;        /* 16: 1 - beta1^t */
  float bc2_sqrt;   /* 20: sqrt(1 - beta2^t) */
  float lr;         /* 24: base learning rate of step t (the schedule's value; a tensor uses lr * lr_mult) */
  float coef;       /* 28: clip coefficient of this step, min(1, max_norm / (norm + 1e-6)); exactly 1 when nothing is clipped */
  float grad_norm;  /* 32: global L2 norm of grad * grad_scale of this step (written only when the norm pass ran) */
  float ema_alpha;  /* 36: 1 - decay_t of this step */
  int32_t skip;     /* 40: 1: insar_adamw_step of this step returns without touching anything */
  int32_t _pad;     /* 44 */
} InsarOptwState;

enum { INSAR_SCHED_NONE = 0, INSAR_SCHED_CONSTANT = 1, INSAR_SCHED_COSINE = 2, INSAR_SCHED_POLY = 3 };

/* What is fixed per optimizer (host memory; copied into the launch). With s = t - 1 steps finished before step t:
 *   s <  warmup_steps: lr_t = lr * (warmup_start + (1 - warmup_start) * s / warmup_steps)
 *   CONSTANT: lr;  s >= total_steps: min_lr;  q = (s - warmup_steps) / (total_steps - warmup_steps)
 *   COSINE:   min_lr + (lr - min_lr) * (1 + cos(pi q)) / 2;   POLY: min_lr + (lr - min_lr) * (1 - q)^power
 * (NONE: lr_t = lr), evaluated in double and rounded to float once. */
typedef struct InsarOptwConfig {
  double lr;            /* base learning rate (the first parameter group's) */
  double beta1, beta2;
  double max_norm;      /* clip bound on the global gradient norm; < 0: no clipping */
  double warmup_start;  /* lr factor at s = 0 */
  double min_lr;
  double power;
  double ema_decay;     /* < 0: no EMA; decay_t = min(ema_decay, (1 + t) / (10 + t)) with ema_warmup, else ema_decay */
  int64_t warmup_steps;
  int64_t total_steps;
  int32_t schedule;     /* INSAR_SCHED_* */
  int32_t skip_nonfinite; /* 1: a step whose gradient norm is inf / NaN is skipped and counted */
  int32_t ema_warmup;
  int32_t _pad;
} InsarOptwConfig;

/* partials[c] = sum over chunk c of (grad * grad_scale)^2: fp32 per thread, wave shuffle, four waves through LDS; no atomics. */
int insar_gradnorm_partials(const int64_t* table, const int32_t* chunks, int32_t nchunks, int32_t chunk_elems,
                            float grad_scale, float* partials, void* stream);
/* One work-group: norm = sqrt(sum of the partials, fixed order, double); coef; then either marks the step skipped or advances
 * t, the bias corrections (double, as insar_adam_step_dev), lr and the EMA factor. nparts = 0: no norm pass, coef = 1. */
int insar_optw_advance(const InsarOptwConfig* cfg, const float* partials, int32_t nparts, InsarOptwState* state, void* stream);
/* g' = grad * (grad_scale * coef); decoupled: p -= (lr * lr_mult * wd) * p, else g' += wd * p; Adam's update of
 * insar_adam_step with g'; ema += (p_new - ema) * ema_alpha where the row has an EMA pointer. 16-byte accesses where
 * every pointer of the row is 16-byte aligned, element-wise otherwise. Nothing is written when state->skip is set. */
int insar_adamw_step(const int64_t* table, const int32_t* chunks, int32_t nchunks, int32_t chunk_elems, float beta1,
                     float beta2, float eps, float grad_scale, int32_t decoupled, const InsarOptwState* state, void* stream);

/* ---- small helpers ---------------------------------------------------------------------------- */
int insar_scale_f32(float* p, int64_t n, float s, void* stream);
/* out[i] = x[i] * *scale, the factor in DEVICE memory: backward of the loss entry points (criterion(...).backward() at :345
 * hands d loss as a device scalar; no host read-back, no framework kernel). out and x 16-byte aligned. */
int insar_mul_dev_f32(float* out, const float* x, int64_t n, const float* scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INSAR_HIP_H */
