// The epilogue the three tiled convolution kernels (igemm.hip, conv3x3_flat.hip, conv3x3_flat2.hip) share:
//   accumulators -> LDS tile [pixel][channel] -> 16-byte NHWC stores (+ per-channel sums) -> one statistics-slab row.
// The call sites keep the barriers and the -DINSAR_STAMPS boundaries between the pieces. igemm.hip has a store loop of its
// own (bias / add / gate, the mode-1 scatter offset, all chunks prefetched at once, sums over the values as stored) around
// the same sum steps.
#pragma once
#include "common.h"

// A wave's NT x MT accumulator tiles (MFMA A = weights, B = activations: a lane holds 4 consecutive channels of pixel r16 in
// tile (nt, mt)) into the LDS tile, rounded to T. row0 / col0: origin of the wave's sub-tile.
template <int ES, int PITCH, int NT, int MT, typename Acc>
__device__ __forceinline__ void acc_to_tile(char* tile, const Acc (&acc)[NT][MT], int row0, int col0, int r16, int kq) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = row0 + mt * 16 + r16;
      const int col = col0 + nt * 16 + kq * 4;
      char* p = tile + row * PITCH + col * ES;
      if constexpr (ES == 2) {
        uint2 v;
        v.x = pack2_bf16(acc[nt][mt][0], acc[nt][mt][1]);
        v.y = pack2_bf16(acc[nt][mt][2], acc[nt][mt][3]);
        *(uint2*)p = v;
      } else {
        *(Acc*)p = acc[nt][mt];
      }
    }
}

// One chunk's share of the BatchNorm partial sums (forward statistics): s1 += f, s2 += f^2
template <int CH>
__device__ __forceinline__ void sum_step(const float* f, float* s1, float* s2) {
#pragma unroll
  for (int j = 0; j < CH; ++j) { s1[j] += f[j]; s2[j] = fmaf(f[j], f[j], s2[j]); }
}
// ... of the consumer unit's BatchNorm-backward sums (InsarBstat): f is the gradient, yy the consumer's y at the same
// position, masked by the consumer's ReLU (y * scale + shift > 0): s1 += m, s2 += m * y
template <int CH>
__device__ __forceinline__ void bstat_sum_step(const float* f, const float* yy, const float* bsc, const float* bsh, float* s1, float* s2) {
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const float m = fmaf(yy[j], bsc[j], bsh[j]) > 0.f ? f[j] : 0.f;
    s1[j] += m; s2[j] = fmaf(m, yy[j], s2[j]);
  }
}

// The LDS tile (BM rows x BN channels) to global memory as 16-byte NHWC stores, rows with rowOut < 0 (halo pixels, rows beyond
// the image) skipped; the thread's sums over its chunk column cc = tid % CPR of the stored rows start at zero here. BS: the
// consumer unit's y at the output's positions, half of this thread's chunks requested at a time.
template <typename T, int BN, bool BS, int THREADS, int BM, int PITCH>
__device__ __forceinline__ void store_tile_rows(const char* tile, const long long* rowOut, char* y, int n0, int tid, const char* by,
                                                const float* bscale, const float* bshift, float* s1, float* s2) {
  constexpr int ES = sizeof(T), CH = Chunk<T>::N;
  constexpr int CPR = BN * ES / 16;               // 16-byte chunks per tile row
  constexpr int ITER = BM * CPR / THREADS;
  constexpr int RSTEP = THREADS / CPR;
  const int cc = tid % CPR;
  const long long col_off = n0 + cc * CH;
#pragma unroll
  for (int j = 0; j < CH; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  float bsc[BS ? CH : 1], bsh[BS ? CH : 1];
  if constexpr (BS) {
#pragma unroll
    for (int j = 0; j < CH; ++j) { bsc[j] = bscale[col_off + j]; bsh[j] = bshift[col_off + j]; }
  }
  constexpr int HALF = ITER / 2;
  static_assert(ITER % 2 == 0, "epilogue chunk batches");
#pragma unroll
  for (int i0 = 0; i0 < ITER; i0 += HALF) {
    uint4 yv[BS ? HALF : 1];
    if constexpr (BS) {
#pragma unroll
      for (int i = 0; i < HALF; ++i) {
        const long long ro = rowOut[(i0 + i) * RSTEP + tid / CPR];
        yv[i] = ro >= 0 ? *(const uint4*)(by + (ro + col_off) * ES) : make_uint4(0u, 0u, 0u, 0u);
      }
    }
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
      const int row = (i0 + i) * RSTEP + tid / CPR;
      const long long ro = rowOut[row];
      if (ro >= 0) {
        const uint4 u = *(const uint4*)(tile + row * PITCH + cc * 16);
        float f[CH];
        Chunk<T>::unpack(u, f);
        if constexpr (BS) {
          float yy[CH];
          Chunk<T>::unpack(yv[i], yy);
          bstat_sum_step<CH>(f, yy, bsc, bsh, s1, s2);
        } else {
          sum_step<CH>(f, s1, s2);
        }
        *(uint4*)(y + (ro + col_off) * ES) = u;
      }
    }
  }
}

// The threads' sums into one row of the statistics slab [rows][2][N]: lanes >= CPR hold other pixel rows of the same CPR
// chunk columns and are folded by shuffles, the waves' partials meet in sstat[wave][BN][2], and thread c < BN adds them into
// stats[row][.][col0 + c]. Per tile: row = the M tile, col0 = the N tile's first channel; sums carried over a persistent
// work-group's tiles: row = blockIdx.x, col0 = 0. The (retired) LDS store guard of common.h brackets the store.
template <int BN, int CH, int CPR, int NWAVES>
__device__ __forceinline__ void fold_tile_stats(float* s1, float* s2, float* sstat, float* stats, long long row, int N, int col0,
                                                int tid, int lane, int wave) {
#pragma unroll
  for (int j = 0; j < CH; ++j) {
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1) { s1[j] += __shfl_xor(s1[j], o, 64); s2[j] += __shfl_xor(s2[j], o, 64); }
  }
#pragma unroll
  for (int j = 0; j < CH; ++j) { LDS_PIN(s1[j]); LDS_PIN(s2[j]); }
  if (lane < CPR) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      sstat[(wave * BN + lane * CH + j) * 2 + 0] = s1[j];
      sstat[(wave * BN + lane * CH + j) * 2 + 1] = s2[j];
    }
  }
  LDS_DRAIN();               // see common.h: keep the store's source registers intact until it has drained
#pragma unroll
  for (int j = 0; j < CH; ++j) { LDS_KEEP(s1[j]); LDS_KEEP(s2[j]); }
  __syncthreads();
  if (tid < BN) {
    float v1 = 0.f, v2 = 0.f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) { v1 += sstat[(w * BN + tid) * 2 + 0]; v2 += sstat[(w * BN + tid) * 2 + 1]; }
    stats[(row * 2 + 0) * N + col0 + tid] = v1;
    stats[(row * 2 + 1) * N + col0 + tid] = v2;
  }
}
