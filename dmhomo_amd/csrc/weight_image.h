// The arithmetic of a conv weight's fp16-piece image, stated once: every kernel that standardises a weight row, picks an
// output channel's scale or writes an image element — alone or table-driven, in whichever translation unit — calls these.
// tests/test_gpu_weight_image.py pins the routes to each other and the element order to its numpy restatement.
#pragma once
#include "common.h"

// N1 for one output channel: out = (wr - mean) * rsqrt(var + eps) over its K weights, two passes, by one 256-thread block.
// (explicit fmaf, nothing else a compiler could contract: the same bits from every translation unit)
__device__ __forceinline__ void ws_standardize_row(const float* __restrict__ wr, float* __restrict__ out, int K, float eps) {
  __shared__ float red[8];
  float s = 0.f;
  for (int i = threadIdx.x; i < K; i += 256) s += wr[i];
  for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)K;
  float q = 0.f;
  for (int i = threadIdx.x; i < K; i += 256) {
    const float d = wr[i] - mean;
    q = fmaf(d, d, q);
  }
  for (int off = 32; off; off >>= 1) q += __shfl_xor(q, off);
  if ((threadIdx.x & 63) == 0) red[4 + (threadIdx.x >> 6)] = q;
  __syncthreads();
  const float var = (red[4] + red[5] + red[6] + red[7]) / (float)K;
  const float rstd = 1.0f / sqrtf(var + eps);
  for (int i = threadIdx.x; i < K; i += 256) out[i] = (wr[i] - mean) * rstd;
}

// m: this lane's share of max |w| over a row, one wave per row -> the row's 2^-k, where max |w| * 2^k lies in [2^14, 2^15)
// (1 for an all-zero or padded row)
__device__ __forceinline__ float f16x3_row_scale(float m) {
  for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if (!(m > 0.f && m < 3.0e38f)) return 1.f;
  int e;
  frexpf(m, &e);  // m = f * 2^e, f in [0.5, 1)  ->  m * 2^(15 - e) in [2^14, 2^15)
  return ldexpf(1.f, min(max(e - 15, -100), 100));
}

// fp16 element index: ((((((nt * nchunks + ch) * NTAPS + tap) * 2 + nh) * 2 + nb) * 2 + plane) * 64 + lane) * 8 + j
//   -> plane (g1, g2) of w[o = nt*64 + nh*32 + nb*16 + (lane & 15)][K slot k = (lane >> 4)*8 + j of chunk ch][tap] * 2^k
struct F16x3Slot {
  int ch, tap, plane, o, k;
};
__device__ __forceinline__ F16x3Slot f16x3_slot(int64_t idx, int NTAPS, int nchunks) {
  F16x3Slot s;
  const int j = idx % 8, lane = (idx >> 3) % 64;
  s.plane = (idx >> 9) & 1;
  const int nb = (idx >> 10) & 1, nh = (idx >> 11) & 1;
  int64_t r = idx >> 12;
  s.tap = r % NTAPS;
  r /= NTAPS;
  s.ch = r % nchunks;
  s.o = (int)(r / nchunks) * 64 + nh * 32 + nb * 16 + (lane & 15);
  s.k = (lane >> 4) * 8 + j;
  return s;
}

// the two pieces of a scaled weight: g1 = fp16(ws), g2 = fp16(ws - g1)
__device__ __forceinline__ _Float16 f16x3_piece(float ws, int plane) {
  const _Float16 g1 = (_Float16)ws;
  return plane == 0 ? g1 : (_Float16)(ws - (float)g1);
}
