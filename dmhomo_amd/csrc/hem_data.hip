// HEM training batches from sampled pairs (the consumer contract of the DGM output): the per-item work of
// DGMTrainData.__getitem__ / data_aug (HEM/dataset/data_loader.py:121-255) on the device, a whole batch per launch.  The
// reference builds every item in DataLoader workers with OpenCV and float64 numpy:
//
//   img1, img2 = cv2.resize(.., (W, H))  on the uint8 record, when its size differs from ori_size          data_loader.py:138-143
//   imgs_rgb_full  = cat(img1, img2) / 255.                                                                 data_loader.py:145-146
//   imgs_gray_full = mean_c((img - mean_I) / std_I)  in float64, stored as fp32                             data_loader.py:240-250
//   flow_gt_full   = cat(homo_convert_to_flow(homo_inv), homo_convert_to_flow(homo))                        data_loader.py:202,232-233
//   *_patch        = the window [y:y+ph, x:x+pw] of the grey and flow tensors                               data_loader.py:229-237
//
// Here one thread owns four consecutive output pixels of one row: it resizes the six source planes, and writes the twelve
// full-size planes and — where its pixels fall inside the sample's crop — the six patch planes from the same registers, so a
// patch is bit for bit the window of the full tensor.  The source is a uint8 image of 6 bytes per pixel that stays in cache;
// by its bytes the launch should be bound by the 48 B per output pixel (+ 24 B per patch pixel) it writes — expected, not
// established: it also does 12 float64 divides per output pixel (8 grey, 4 mapping); tools/bench_hem_batch.py measures it.
//
// The resize restates cv2's 8-bit INTER_LINEAR path (resize.cpp: coefficients rounded to shorts of 11 fractional bits,
// horizontal pass in int32, vertical pass ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2; the horizontal
// fraction is clamped with its index, the vertical one is not: only the two row indices are clipped).  It is integer
// arithmetic, so the device and the numpy restatement in tests/hem_ref.py agree bit for bit; OpenCV is not in the build image
// and parity with cv2 itself is UNPINNED.  The float kernel of dataset.hip is cv2's float path (the
// condition dataset resizes float images) and cannot stand in for this one.
#include "common.h"
#include "geometry_dev.h"

#pragma clang fp contract(off)

namespace {
constexpr int kCoefBits = 11;  // cv2 INTER_RESIZE_COEF_BITS; the coefficients are shorts scaled by 2048

// source index and the two short coefficients of one output coordinate d of n_dst over n_src source pixels
__device__ __forceinline__ void hem_tap(int d, int n_src, int n_dst, bool clamp_fraction, int& s, int& c0, int& c1) {
  float f = (float)(((double)d + 0.5) * (double)n_src / (double)n_dst - 0.5);
  const float fl = floorf(f);
  s = (int)fl;
  f -= fl;
  if (clamp_fraction) {
    if (s < 0) {
      s = 0;
      f = 0.f;
    }
    if (s >= n_src - 1) {
      s = n_src - 1;
      f = 0.f;
    }
  }
  c0 = (int)rintf((1.f - f) * (float)(1 << kCoefBits));  // round half to even, as cvRound
  c1 = (int)rintf(f * (float)(1 << kCoefBits));
}

// four values of one row of a plane: one 16-byte store where the row is aligned (W % 4 == 0), else one by one
__device__ __forceinline__ void put_row4(float* __restrict__ p, const float (&v)[4], int n, bool vec) {
  if (vec) {
    st4(p, make_float4(v[0], v[1], v[2], v[3]));
  } else {
    for (int j = 0; j < n; ++j) p[j] = v[j];
  }
}

struct HemStats {
  double mean[3], std[3];
};
}  // namespace

// grid (ceil(H * ceil(W / 4) / 256), B)
__global__ __launch_bounds__(256) void hem_batch_kernel(const unsigned char* __restrict__ img12, const double* __restrict__ homo,
                                                        const double* __restrict__ homo_inv, const int32_t* __restrict__ start,
                                                        HemStats st, int h, int w, int H, int W, int ph, int pw,
                                                        float* __restrict__ gray_full, float* __restrict__ rgb_full,
                                                        float* __restrict__ flow_full, float* __restrict__ gray_patch,
                                                        float* __restrict__ flow_patch) {
  const int b = blockIdx.y;
  const int W4 = (W + 3) >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= H * W4) return;
  const int dy = q / W4, dx0 = (q - dy * W4) * 4;
  const int n = min(4, W - dx0);
  const bool vec = (W & 3) == 0;
  const bool resize = h != H || w != W;

  // ---- the six resized uint8 planes of the thread's pixels
  int sy0 = dy, sy1 = dy, b0 = 0, b1 = 0;
  if (resize) {
    int sy;
    hem_tap(dy, h, H, false, sy, b0, b1);
    sy0 = min(max(sy, 0), h - 1);
    sy1 = min(max(sy + 1, 0), h - 1);
  }
  const unsigned char* src = img12 + (size_t)b * 6 * h * w;
  int u8[6][4];
  for (int j = 0; j < 4; ++j) {
    const int dx = min(dx0 + j, W - 1);  // lanes past the row repeat its last pixel and are not stored
    int sx = dx, sx1 = dx, a0 = 0, a1 = 0;
    if (resize) {
      hem_tap(dx, w, W, true, sx, a0, a1);
      sx1 = min(sx + 1, w - 1);
    }
    for (int c = 0; c < 6; ++c) {
      const unsigned char* pl = src + (size_t)c * h * w;
      if (resize) {
        const int S0 = (int)pl[(size_t)sy0 * w + sx] * a0 + (int)pl[(size_t)sy0 * w + sx1] * a1;
        const int S1 = (int)pl[(size_t)sy1 * w + sx] * a0 + (int)pl[(size_t)sy1 * w + sx1] * a1;
        u8[c][j] = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
      } else {
        u8[c][j] = pl[(size_t)dy * w + dx];
      }
    }
  }

  // ---- the crop of this sample: device data.  A start outside the image poisons the sample's patch tensors
  const int px = start[2 * b], py = start[2 * b + 1];
  const bool crop_ok = px >= 0 && px <= W - pw && py >= 0 && py <= H - ph;
  const size_t HW = (size_t)H * W, PP = (size_t)ph * pw;
  const size_t row = (size_t)dy * W + dx0;
  const bool in_rows = crop_ok && dy >= py && dy < py + ph;
  auto put_patch = [&](float* __restrict__ plane, const float (&v)[4]) {
    if (in_rows) {
      for (int j = 0; j < n; ++j) {
        const int tx = dx0 + j - px;
        if (tx >= 0 && tx < pw) plane[(size_t)(dy - py) * pw + tx] = v[j];
      }
    } else if (!crop_ok && dy < ph) {
      for (int j = 0; j < n; ++j)
        if (dx0 + j < pw) plane[(size_t)dy * pw + dx0 + j] = __builtin_nanf("");
    }
  };

  float v[4];
  // imgs_rgb_full: resized uint8 / 255
  for (int c = 0; c < 6; ++c) {
    for (int j = 0; j < 4; ++j) v[j] = (float)u8[c][j] / 255.f;
    put_row4(rgb_full + ((size_t)b * 6 + c) * HW + row, v, n, vec);
  }
  // imgs_gray_*: float64 normalisation and channel mean, np.mean's order ((g0 + g1) + g2) / 3
  for (int i = 0; i < 2; ++i) {
    for (int j = 0; j < 4; ++j) {
      const double g0 = ((double)u8[3 * i][j] - st.mean[0]) / st.std[0];
      const double g1 = ((double)u8[3 * i + 1][j] - st.mean[1]) / st.std[1];
      const double g2 = ((double)u8[3 * i + 2][j] - st.mean[2]) / st.std[2];
      v[j] = (float)(((g0 + g1) + g2) / 3.0);
    }
    put_row4(gray_full + ((size_t)b * 2 + i) * HW + row, v, n, vec);
    put_patch(gray_patch + ((size_t)b * 2 + i) * PP, v);
  }
  // flow_gt_*: planes 0-1 backward (homo_inv), planes 2-3 forward (homo)
  for (int i = 0; i < 2; ++i) {
    const double* Hm = (i == 0 ? homo_inv : homo) + (size_t)b * 9;
    float fu[4], fv[4];
    for (int j = 0; j < 4; ++j) hem_flow_pixel(Hm, dx0 + j, dy, fu[j], fv[j]);
    put_row4(flow_full + ((size_t)b * 4 + 2 * i) * HW + row, fu, n, vec);
    put_row4(flow_full + ((size_t)b * 4 + 2 * i + 1) * HW + row, fv, n, vec);
    put_patch(flow_patch + ((size_t)b * 4 + 2 * i) * PP, fu);
    put_patch(flow_patch + ((size_t)b * 4 + 2 * i + 1) * PP, fv);
  }
}

// homo_convert_to_flow alone: homo [B][9] f64 -> flow [B][2][H][W]
__global__ __launch_bounds__(256) void hem_flow_kernel(const double* __restrict__ homo, float* __restrict__ flow, int H, int W) {
  const int b = blockIdx.y;
  const int W4 = (W + 3) >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= H * W4) return;
  const int dy = q / W4, dx0 = (q - dy * W4) * 4;
  const int n = min(4, W - dx0);
  const bool vec = (W & 3) == 0;
  float fu[4], fv[4];
  for (int j = 0; j < 4; ++j) hem_flow_pixel(homo + (size_t)b * 9, dx0 + j, dy, fu[j], fv[j]);
  const size_t HW = (size_t)H * W, row = (size_t)dy * W + dx0;
  put_row4(flow + ((size_t)b * 2) * HW + row, fu, n, vec);
  put_row4(flow + ((size_t)b * 2 + 1) * HW + row, fv, n, vec);
}

// sizes for which the launch geometry and the int arithmetic of hem_batch_kernel cannot overflow (its largest tensor has six
// planes); B is a grid y dimension
static bool hem_dims_ok(int B, int H, int W) {
  return dmh_dims_ok({B, H, W}, 1, 1 << 16) && B <= 65535 && (long long)B * 6 * H * W < (1LL << 31);
}

extern "C" int dmh_hem_batch(const unsigned char* img12, const double* homo, const double* homo_inv, const int32_t* start,
                             const double* mean, const double* std, int B, int h, int w, int H, int W, int ph, int pw,
                             float* imgs_gray_full, float* imgs_rgb_full, float* flow_gt_full, float* imgs_gray_patch,
                             float* flow_gt_patch, void* stream) {
  DMH_REQUIRE(img12 && homo && homo_inv && start && mean && std && imgs_gray_full && imgs_rgb_full && flow_gt_full &&
                  imgs_gray_patch && flow_gt_patch,
              "dmh_hem_batch: null pointer");
  DMH_REQUIRE(hem_dims_ok(B, H, W) && hem_dims_ok(B, h, w), "dmh_hem_batch: B=%d, source %dx%d, output %dx%d (B*6*H*W < 2^31)", B,
              h, w, H, W);
  DMH_REQUIRE(ph > 0 && pw > 0 && ph <= H && pw <= W, "dmh_hem_batch: crop %dx%d does not fit the output %dx%d", ph, pw, H, W);
  DMH_REQUIRE((((uintptr_t)imgs_gray_full | (uintptr_t)imgs_rgb_full | (uintptr_t)flow_gt_full) & 15) == 0,
              "dmh_hem_batch: the full-size outputs must be 16-byte aligned");
  HemStats st;
  for (int c = 0; c < 3; ++c) {
    st.mean[c] = mean[c];
    st.std[c] = std[c];
  }
  hipLaunchKernelGGL(hem_batch_kernel, dim3(cdiv(H * ((W + 3) / 4), 256), B), dim3(256), 0, (hipStream_t)stream, img12, homo,
                     homo_inv, start, st, h, w, H, W, ph, pw, imgs_gray_full, imgs_rgb_full, flow_gt_full, imgs_gray_patch,
                     flow_gt_patch);
  DMH_CHECK_LAUNCH("dmh_hem_batch");
  return DMH_OK;
}

extern "C" int dmh_hem_flow(const double* homo, int B, int H, int W, float* flow, void* stream) {
  DMH_REQUIRE(homo && flow, "dmh_hem_flow: null pointer");
  DMH_REQUIRE(dmh_dims_ok({B, H, W}, 1, 1 << 16) && B <= 65535 && (long long)B * 2 * H * W < (1LL << 31),
              "dmh_hem_flow: B=%d H=%d W=%d (B <= 65535, B*2*H*W < 2^31)", B, H, W);
  DMH_REQUIRE(((uintptr_t)flow & 15) == 0, "dmh_hem_flow: flow must be 16-byte aligned");
  hipLaunchKernelGGL(hem_flow_kernel, dim3(cdiv(H * ((W + 3) / 4), 256), B), dim3(256), 0, (hipStream_t)stream, homo, flow, H, W);
  DMH_CHECK_LAUNCH("dmh_hem_flow");
  return DMH_OK;
}
