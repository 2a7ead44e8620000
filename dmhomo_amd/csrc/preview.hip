// Sample preview sheets (DDP:1489-1555, 1871-1935, 1972-2019): postProcess's four-panel buffers in one launch, the same panels
// fused with the BGR swap, torchvision's make_grid layout and save_image's quantisation into uint8 sheets, and the
// homography warp of postProcess_cv2.  The warp and flow panels use the device functions of geometry.hip (geometry_dev.h), so
// they are bit for bit dmh_flow_warp / dmh_flow_to_image.
#include "geometry_dev.h"

#pragma clang fp contract(off)

#define DMH_PREVIEW_MAX_FLOW 256.f   // visulize_flow calls flow_to_image with its default max_flow (DDP:1495, 1471)

// the four panels of one pixel, for both buffers (DDP:1505-1517):
//   row1 = [img1 | img1 | mask | flow_vis],  row2 = [img2 | flow_warp(img2, flow) | mask | flow_vis]   (3 channels each)
struct PreviewPixel {
  float img1[3], img2[3], warp[3], flo[3], mask;
};
__device__ __forceinline__ PreviewPixel preview_pixel(const float* __restrict__ img, const float* __restrict__ mask,
                                                      const float* __restrict__ flow, int b, int yi, int xi, int H, int W) {
  PreviewPixel q;
  const size_t hw = (size_t)H * W, p = (size_t)yi * W + xi;
  const float* ib = img + (size_t)b * 6 * hw;
  const float fu = flow[((size_t)b * 2 + 0) * hw + p], fv = flow[((size_t)b * 2 + 1) * hw + p];
  const FlowWarpTaps t = flow_warp_taps(fu, fv, xi, yi, H, W);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    q.img1[c] = ib[c * hw + p];
    q.img2[c] = ib[(3 + c) * hw + p];
    q.warp[c] = flow_warp_sample(ib + (3 + c) * hw, t, W);
  }
  q.mask = mask[(size_t)b * hw + p];
  flow_pixel_to_rgb(fu, fv, DMH_PREVIEW_MAX_FLOW, q.flo[0], q.flo[1], q.flo[2]);
  return q;
}

// ---------------------------------------------------------------------------------------------
// postProcess: buf1, buf2 [B][3][H][4W] fp32.  One thread per source pixel: 9 floats in (+ the 12 warp taps), 24 out.
__global__ __launch_bounds__(256) void post_process_kernel(const float* __restrict__ img, const float* __restrict__ mask,
                                                           const float* __restrict__ flow, float* __restrict__ buf1,
                                                           float* __restrict__ buf2, int H, int W) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int yi = p / W, xi = p % W;
  const PreviewPixel q = preview_pixel(img, mask, flow, b, yi, xi, H, W);
  const size_t W4 = (size_t)4 * W;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t o = (((size_t)b * 3 + c) * H + yi) * W4 + xi;
    buf1[o] = q.img1[c];
    buf1[o + W] = q.img1[c];
    buf1[o + 2 * (size_t)W] = q.mask;
    buf1[o + 3 * (size_t)W] = q.flo[c];
    buf2[o] = q.img2[c];
    buf2[o + W] = q.warp[c];
    buf2[o + 2 * (size_t)W] = q.mask;
    buf2[o + 3 * (size_t)W] = q.flo[c];
  }
}

// ---------------------------------------------------------------------------------------------
// torchvision.utils.save_image's quantisation: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) — two roundings, truncation
__device__ __forceinline__ unsigned quantise_u8(float x) {
  const float v = __fadd_rn(__fmul_rn(x, 255.f), 0.5f);
  return (unsigned)fminf(fmaxf(v, 0.f), 255.f);
}

// sheet1, sheet2 [Hs][Ws][3] uint8: make_grid(buf[:, [2,1,0]] if bgr else buf, nrow, padding, pad_value=0) quantised.
//   xmaps = min(nrow, B), ymaps = ceil(B / xmaps); Hs = ymaps*(H+p)+p, Ws = xmaps*(4W+p)+p; image k at row
//   (k / xmaps)*(H+p)+p, column (k % xmaps)*(4W+p)+p.  B == 1: the image alone (Hs = H, Ws = 4W; xmaps = 0 says so here).
// Thread i owns bytes [4i, 4i+4) of both sheets (one dword store each); a pixel's panels are evaluated once per thread that
// touches it (4 bytes span at most 2 pixels).
__global__ __launch_bounds__(256) void preview_sheet_kernel(const float* __restrict__ img, const float* __restrict__ mask,
                                                            const float* __restrict__ flow, unsigned char* __restrict__ sheet1,
                                                            unsigned char* __restrict__ sheet2, int B, int H, int W, int xmaps,
                                                            int pad, int Ws, long long total, int bgr) {
  const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (first >= total) return;
  const int W4 = 4 * W, cellh = H + pad, cellw = W4 + pad;
  unsigned w1 = 0, w2 = 0;
  long long cur = -1;           // the sheet pixel whose values v1 / v2 hold
  float v1[3], v2[3];
  const int nb = total - first < 4 ? (int)(total - first) : 4;
  for (int j = 0; j < nb; ++j) {
    const long long e = first + j;
    const long long pix = e / 3;
    const int ch = (int)(e - pix * 3);
    if (pix != cur) {
      cur = pix;
      const int sy = (int)(pix / Ws), sx = (int)(pix - (long long)sy * Ws);
      int k, ry, rx;
      if (xmaps == 0) {
        k = 0, ry = sy, rx = sx;
      } else {
        const int ky = sy / cellh, kx = sx / cellw;
        ry = sy - ky * cellh - pad;
        rx = sx - kx * cellw - pad;
        k = kx < xmaps ? ky * xmaps + kx : B;
      }
      if (ry < 0 || rx < 0 || k >= B) {
        v1[0] = v1[1] = v1[2] = v2[0] = v2[1] = v2[2] = 0.f;      // pad_value
      } else {
        const int panel = rx / W, xi = rx - panel * W;
        const PreviewPixel q = preview_pixel(img, mask, flow, k, ry, xi, H, W);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int s = bgr ? 2 - c : c;
          v1[c] = panel == 0 || panel == 1 ? q.img1[s] : panel == 2 ? q.mask : q.flo[s];
          v2[c] = panel == 0 ? q.img2[s] : panel == 1 ? q.warp[s] : panel == 2 ? q.mask : q.flo[s];
        }
      }
    }
    const float a = ch == 0 ? v1[0] : ch == 1 ? v1[1] : v1[2];
    const float c2 = ch == 0 ? v2[0] : ch == 1 ? v2[1] : v2[2];
    w1 |= quantise_u8(a) << (8 * j);
    w2 |= quantise_u8(c2) << (8 * j);
  }
  if (nb == 4) {
    *reinterpret_cast<unsigned*>(sheet1 + first) = w1;
    *reinterpret_cast<unsigned*>(sheet2 + first) = w2;
  } else {                      // the last 1-3 bytes of a sheet whose size is not a multiple of 4
    for (int j = 0; j < nb; ++j) {
      sheet1[first + j] = (unsigned char)(w1 >> (8 * j));
      sheet2[first + j] = (unsigned char)(w2 >> (8 * j));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// cv2.warpPerspective(src, M, (Wd, Hd)) without WARP_INVERSE_MAP: dst(x, y) = src(M^-1 (x, y, 1)), bilinear, constant border 0
// applied per neighbour.  DELIBERATE DEVIATION: cv2 interpolates with fixed-point coefficient tables that quantise the
// fraction to 1/32 (INTER_TAB_SIZE) — not installed here, so not pinnable; the contract of this kernel is the EXACT bilinear
// result: inverse, coordinates and weights in float64, only the result rounded to fp32.
__global__ __launch_bounds__(256) void homography_warp_kernel(const float* __restrict__ src, const double* __restrict__ Hm,
                                                              float* __restrict__ dst, int H, int W, int Hd, int Wd) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= Hd * Wd) return;
  const int yi = p / Wd, xi = p % Wd;
  double inv[9];
  double sx, sy;
  homography_inverse(Hm + (size_t)b * 9, inv);      // geometry_dev.h: the three pieces are shared with relabel.hip
  homography_warp_source(inv, xi, yi, sx, sy);
  const HomographyWarpTaps t = homography_warp_taps(sx, sy, H, W);
  const size_t hw = (size_t)H * W, hwd = (size_t)Hd * Wd;
  for (int c = 0; c < 3; ++c)
    dst[((size_t)b * 3 + c) * hwd + p] = homography_warp_sample(src + ((size_t)b * 3 + c) * hw, t, W);
}

// ---------------------------------------------------------------------------------------------
// sizes: every dimension in [1, 2^16] and the largest tensor of the call below 2^31 elements, so that the int pixel counts of
// the launch geometry and the kernels cannot overflow; B is a grid y dimension (<= 65535)
static bool preview_dims_ok(int B, int H, int W) {
  return dmh_dims_ok({B, H, W}, 1, 1 << 16) && B <= 65535 && H > 1 && W > 1 &&
         (long long)B * 3 * H * 4 * W < (1LL << 31);
}

extern "C" int dmh_post_process(const float* img, const float* mask, const float* flow, float* buf1, float* buf2, int B, int H,
                                int W, void* stream) {
  DMH_REQUIRE(img && mask && flow && buf1 && buf2, "dmh_post_process: null pointer");
  DMH_REQUIRE(preview_dims_ok(B, H, W), "dmh_post_process: B=%d H=%d W=%d (H, W >= 2; B*3*H*4W < 2^31)", B, H, W);
  hipLaunchKernelGGL(post_process_kernel, dim3(cdiv(H * W, 256), B), dim3(256), 0, (hipStream_t)stream, img, mask, flow, buf1,
                     buf2, H, W);
  DMH_CHECK_LAUNCH("dmh_post_process");
  return DMH_OK;
}

extern "C" int dmh_preview_sheet(const float* img, const float* mask, const float* flow, unsigned char* sheet1,
                                 unsigned char* sheet2, int B, int H, int W, int nrow, int padding, int bgr, void* stream) {
  DMH_REQUIRE(img && mask && flow && sheet1 && sheet2, "dmh_preview_sheet: null pointer");
  DMH_REQUIRE(((uintptr_t)sheet1 & 3) == 0 && ((uintptr_t)sheet2 & 3) == 0, "dmh_preview_sheet: the sheets must be 4-byte aligned");
  DMH_REQUIRE(preview_dims_ok(B, H, W), "dmh_preview_sheet: B=%d H=%d W=%d (H, W >= 2; B*3*H*4W < 2^31)", B, H, W);
  DMH_REQUIRE(dmh_dims_ok({nrow}, 1, 1 << 16) && dmh_dims_ok({padding}, 0, 1 << 16), "dmh_preview_sheet: nrow=%d padding=%d",
              nrow, padding);
  long long Hs = H, Ws = 4LL * W;
  int xmaps = 0;                                   // B == 1: make_grid returns the image itself
  if (B > 1) {
    xmaps = nrow < B ? nrow : B;
    const long long ymaps = (B + xmaps - 1) / xmaps;
    Hs = ymaps * (H + padding) + padding;
    Ws = xmaps * (4LL * W + padding) + padding;
  }
  const long long total = Hs * Ws * 3;
  DMH_REQUIRE(Ws < (1LL << 30) && total < (1LL << 31), "dmh_preview_sheet: a sheet of %lld x %lld pixels is too large", Hs, Ws);
  hipLaunchKernelGGL(preview_sheet_kernel, dim3((unsigned)cdiv64(total, 1024)), dim3(256), 0, (hipStream_t)stream, img, mask,
                     flow, sheet1, sheet2, B, H, W, xmaps, padding, (int)Ws, total, bgr != 0);
  DMH_CHECK_LAUNCH("dmh_preview_sheet");
  return DMH_OK;
}

extern "C" int dmh_homography_warp(const float* src, const double* homos, float* dst, int B, int H, int W, int Hd, int Wd,
                                   void* stream) {
  DMH_REQUIRE(src && homos && dst, "dmh_homography_warp: null pointer");
  DMH_REQUIRE(dmh_dims_ok({B, H, W, Hd, Wd}, 1, 1 << 16) && B <= 65535 && (long long)B * 3 * H * W < (1LL << 31) &&
                  (long long)B * 3 * Hd * Wd < (1LL << 31),
              "dmh_homography_warp: B=%d, src %dx%d, dst %dx%d (each tensor below 2^31 elements)", B, H, W, Hd, Wd);
  hipLaunchKernelGGL(homography_warp_kernel, dim3(cdiv(Hd * Wd, 256), B), dim3(256), 0, (hipStream_t)stream, src, homos, dst,
                     H, W, Hd, Wd);
  DMH_CHECK_LAUNCH("dmh_homography_warp");
  return DMH_OK;
}
